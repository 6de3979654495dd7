"""N3p on the host: the three entry points of the bf16-compute posterior chain under grad are exported, declared and refuse bad
arguments before any launch; `LatentModel.chain_grad_compute` and the `SlacAlgorithm` keyword; `chain_form` is what it was; and the
helper tests/chain_grad_bf16_ref.py, which tests/test_chain_grad_bf16_gpu.py relies on, restates N3m's forward bitwise and gives the
same gradients in fp32 and in fp64."""
import ctypes
import inspect
import os
import types

import pytest
import torch

import chain_bf16_ref as C
import chain_grad_bf16_ref as G
import slac_latent_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_versioned():
    from s2p_amd import _lib
    header = open(os.path.join(ROOT, "include", "s2p_hip.h")).read()
    L = _lib.lib()
    for name in (G.FWD, G.BWD, G.PACK):
        assert name in _lib.SIGNATURES and "int %s(" % name in header and hasattr(L, name)
    S = _lib.SIGNATURES
    assert S[G.FWD][:6] + S[G.FWD][7:] == S["s2p_posterior_chain_fwd_save"][:6] + S["s2p_posterior_chain_fwd_save"][7:]
    assert S[G.FWD][6] == S["s2p_posterior_chain_fwd_bf16"][6]
    assert S[G.BWD][:8] + S[G.BWD][9:] == S["s2p_posterior_chain_bwd"][:8] + S["s2p_posterior_chain_bwd"][9:]
    assert "} s2p_chain_mlp_bwd_bf16;" in header and "} s2p_bf16_pack_job;" in header
    assert L.s2p_version() == 125
    assert ctypes.sizeof(_lib.ChainMlpBwdBf16) == 3 * 8 + 2 * 4 and ctypes.sizeof(_lib.Bf16PackJob) == 3 * 8 + 5 * 4 + 4
    for name in ("posterior_chain_fwd_save_bf16", "posterior_chain_bwd_bf16", "chain_mlp_bwd_bf16", "chain_pack_bf16"):
        from s2p_amd import ops
        assert callable(getattr(ops, name))


@pytest.mark.parametrize("name", [G.FWD, G.BWD])
def test_chain_refusals_and_no_ops_without_a_device(name):
    from s2p_amd import _lib
    n = G.check(_lib, name)
    print(name, n, "refusals")
    assert n == len(G.cases(name)) and n >= (30 if name == G.BWD else 50)


def test_the_order_of_the_checks_is_the_documented_one():
    """A call that breaks several conditions gets the first one's message: mlps before the state, the state before the grads."""
    from s2p_amd import _lib
    L = _lib.lib()
    for name, edit, text in ((G.FWD, dict(mlp=(3, "w3", None), state=("xz", None)), "z2_prior: null operand"),
                             (G.FWD, dict(eps_pitch=100, state=None), "a pitch is below its row"),
                             (G.BWD, dict(mlp=(1, "k1", 256), state=("h1a", None)), "z2_prior: the first layer's K is 256"),
                             (G.BWD, dict(state=("h1a", None), grads=("dxz", None)), "state: a chain buffer"),
                             (G.BWD, dict(dz_pitch=287, mlp=(0, "w1t", None)), "a pitch is below its row")):
        assert getattr(L, name)(*G.args(_lib, name, **edit)) < 0 and text in L.s2p_last_error().decode(), (name, edit)


def test_pack_refusals_and_no_ops_without_a_device():
    from s2p_amd import _lib
    L = _lib.lib()
    fn = L.s2p_chain_pack_bf16
    assert fn(None, 0, None) == 0                                                # no job: no pointer is looked at
    for empty in (dict(rows=0, src=None, dst=None, dst_t=None), dict(cols=0, src=None, dst=None, dst_t=None, src_pitch=0)):
        assert fn((_lib.Bf16PackJob * 1)(G.pack_job(_lib, **empty)), 1, None) == 0, empty
    assert fn(None, -1, None) < 0 and b"negative size" in L.s2p_last_error()
    assert fn(None, 2, None) < 0 and b"null pointer" in L.s2p_last_error()
    for edit, text in G.PACK_CASES:
        for jobs in ([G.pack_job(_lib, **edit)], [G.pack_job(_lib, rows=0), G.pack_job(_lib, **edit)]):      # alone; behind an empty job
            rc = fn((_lib.Bf16PackJob * len(jobs))(*jobs), len(jobs), None)
            msg = L.s2p_last_error().decode()
            assert rc < 0 and "s2p_chain_pack_bf16:" in msg and text in msg, (edit, rc, msg)


# ---- the attribute and the keyword --------------------------------------------------------------------------------------------------------
def test_the_attribute_and_the_keyword_default_to_fp32():
    from s2p_amd.slac import LatentModel, _chain_grad_compute
    from s2p_amd.slac_algo import SlacAlgorithm
    assert inspect.signature(SlacAlgorithm.__init__).parameters["chain_grad_compute"].default == "fp32"
    assert "self.latent.chain_grad_compute = chain_grad_compute" in inspect.getsource(SlacAlgorithm.__init__)
    assert "chain_grad_compute" not in inspect.signature(LatentModel.__init__).parameters
    assert 'self.chain_grad_compute = "fp32"' in inspect.getsource(LatentModel.__init__)
    obj = types.SimpleNamespace(chain_grad_compute="fp32")
    assert _chain_grad_compute(obj) == "fp32"
    obj.chain_grad_compute = "bf16"
    assert _chain_grad_compute(obj) == "bf16"
    for bad in ("fp16", "BF16", None, True):
        obj.chain_grad_compute = bad
        with pytest.raises(ValueError, match="chain_grad_compute is 'fp32' or 'bf16'"):
            _chain_grad_compute(obj)


def test_chain_form_is_what_it_was():
    """The four answers, on objects that have the three older attributes only; the new attribute is not read there."""
    from s2p_amd.slac import LatentModel
    form = lambda keep, **kw: LatentModel.chain_form(types.SimpleNamespace(**kw), keep)
    for grad in ("fp32", "bf16", "nonsense", None):
        extra = {} if grad is None else dict(chain_grad_compute=grad)
        for fc in (False, True):
            for cc in ("fp32", "bf16"):
                assert form(True, fused_chain=fc, fused_chain_grad=True, chain_compute=cc, **extra) == "fused_save"
                assert form(True, fused_chain=fc, fused_chain_grad=False, chain_compute=cc, **extra) == "layers"
                want = "layers" if not fc else "fused_bf16" if cc == "bf16" else "fused"
                assert form(False, fused_chain=fc, fused_chain_grad=True, chain_compute=cc, **extra) == want
    with pytest.raises(ValueError):
        form(False, fused_chain=True, fused_chain_grad=False, chain_compute="fp16")
    assert form(True, fused_chain=True, fused_chain_grad=True, chain_compute="fp16") == "fused_save"


# ---- the helper ----------------------------------------------------------------------------------------------------------------------------
def test_helper_forward_is_the_rule_of_the_no_grad_chains_bitwise():
    A = 6
    p = R.make_params(A)
    for B, T in ((5, 3), (2, 1)):
        feat, action, noise = C.random_inputs(B, T, A)
        for dtype in (torch.float64, torch.float32):
            want, got = C.posterior(p, feat, action, noise, dtype), G.posterior(p, feat, action, noise, dtype)
            assert all(torch.equal(a, b) for a, b in zip(want, got)), (B, T, dtype)


def test_helper_layer_rounds_forward_and_input_gradient_but_not_the_weight_gradient():
    g = torch.Generator().manual_seed(3)
    x, w, dy = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((7, 64), (32, 64), (7, 32)))
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = G._Layer.apply(xr, wr, None)
    dx, dw = torch.autograd.grad(y, [xr, wr], grad_outputs=dy)
    assert torch.equal(y, C.bf(x) @ C.bf(w).t()) and torch.equal(dx, C.bf(dy) @ C.bf(w)) and torch.equal(dw, dy.t() @ x)
    assert not torch.equal(dx, dy @ w) and not torch.equal(y, x @ w.t())


def test_helper_fp32_run_agrees_with_its_fp64_run():
    """B 8, T 3, A 6, the shapes of the end-to-end GPU test, per batch row of dfeat and daction (a row's chain is its own).  Where no
    rounding of an operand falls the other way in fp32 than in fp64, the two runs differ by fp32 summation error: within 4e-6 (4 x
    the 1e-6 floor of the project's rule), and that must be the ordinary case -- at least half the rows.  A flip moves one operand by
    one bf16 unit, 2^-8 of its value, and can move a LeakyReLU derivative from 0.2 to 1 for one of 256 units: such a row is allowed 4
    bf16 units on the max-normalised scale, 2^-6; a row beyond that is a wrong formula, not a flip."""
    A, B, T = 6, 8, 3
    p = R.make_params(A)
    rows, worst = [], 0.0
    for seed in (0, 1, 2):
        feat, action, noise = C.random_inputs(B, T, A, seed)
        w = G.loss_weights(B, T, seed)
        ref = G.gradients(p, feat, action, noise, w, torch.float64)
        assert set(ref) == set(["dfeat", "daction"] + G.param_keys()) and len(ref) == 26
        for gen in (None, torch.Generator().manual_seed(9 + seed)):
            got = G.gradients(p, feat, action, noise, w, torch.float32, gen)
            dev = G.deviation(got, ref)
            worst = max(worst, max(dev.values()))
            for k in ("dfeat", "daction"):
                rows += ((got[k].double() - ref[k]).abs().amax((1, 2)) / ref[k].abs().max()).tolist()
            print("seed %d order %s: worst %.3e (%s)" % (seed, "permuted" if gen else "plain", max(dev.values()), max(dev, key=dev.get)))
    tight = sum(r <= 4e-6 for r in rows)
    print("%d of %d rows within 4e-6, worst row %.3e, worst gradient %.3e" % (tight, len(rows), max(rows), worst))
    assert 2 * tight >= len(rows) and max(rows) < 2.0 ** -6 and worst < 2.0 ** -6
    # and the rule is not the unrounded chain's gradient: every operand rounded to 2^-9 of its value moves it visibly
    q = {k: v.double() for k, v in p.items()}
    feat, action, noise = C.random_inputs(B, T, A, 0)
    f, a = feat.double().requires_grad_(True), action.double().requires_grad_(True)
    m, s, z1, z2 = R.sample_posterior(q, f, a, noise.double())
    w = G.loss_weights(B, T, 0)
    plain = torch.autograd.grad((m * w[0]).sum() + (s * w[1]).sum() + (torch.cat([z1, z2], -1) * w[2]).sum(), f)[0]
    ref = G.gradients(p, feat, action, noise, w, torch.float64)["dfeat"]
    far = float((plain - ref).abs().max() / ref.abs().max())
    print("distance of the rule from the unrounded fp64 gradient (dfeat): %.3e" % far)
    assert far > 1e-3
