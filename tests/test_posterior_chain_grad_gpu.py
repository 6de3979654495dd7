"""N3k -- the posterior chain under grad as one launch forward (s2p_posterior_chain_fwd_save) and one launch backward
(s2p_posterior_chain_bwd), `LatentModel.fused_chain_grad`, against the per-layer path it replaces.

The acceptance is BITWISE: both paths run the same MFMA sequence per element and the same epilogues, so every comparison with the
per-layer path -- outputs, every saved tensor, every gradient -- is torch.equal, at the smallest shapes that reach every code path
(a partial 16-row tile, exactly one tile, one row more, three workgroups; T = 1 without a chain step, one step, the workload's nine;
action widths 6 and 1).  The one toleranced check is against the recorded reference (tests/golden/slac_latent_golden_v1.npz) under
the project's rule: err <= K_TOL x max(ref32_err, 1e-6), K_TOL = 4."""
import os

import numpy as np
import pytest
import torch

import slac_buffer_ref as SB
import slac_latent_ref as R
from guard_region import Region
from slac_chain_util import build_model, count_calls, model_cache

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
K_TOL, FLOOR = 4.0, 1e-6
Z1, Z2, Z, FEAT, HID = 32, 256, 288, 256, 256
BS, TS, AS = (1, 15, 16, 17, 33), (1, 2, 9), (6, 1)
FWD, BWD = "s2p_posterior_chain_fwd_save", "s2p_posterior_chain_bwd"
HEADS = ("z2_prior_init", "z1_prior", "z2_prior", "z1_posterior_init", "z1_posterior", "reward")
CHAIN_HEADS = ("z1_posterior_init", "z2_prior_init", "z1_posterior", "z2_prior")
LN2 = 0.6931472


@pytest.fixture(scope="module")
def models(hip_device):
    """action width -> a LatentModel with the seeded weights of tests/slac_latent_ref.py; built once, left with both switches off."""
    return model_cache()


def _inputs(B, T, A, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 100 * T + A)
    feat, action, noise = torch.randn(33, T, FEAT, generator=g), torch.randn(33, T - 1, A, generator=g), torch.randn(33, T, Z, generator=g)
    gout = [torch.randn(33, T, c, generator=g) for c in (Z1, Z1, Z1, Z2)]               # dL/d(mean, std, z1, z2)
    return feat[:B].cuda(), action[:B].cuda(), noise[:B].cuda(), [t[:B].cuda() for t in gout]  # row b is the same whatever B is


def _head_params(m, heads=HEADS):
    named = dict(m.named_parameters())
    keys = [k for k in named if k.split(".")[0] in heads]
    return keys, [named[k] for k in keys]


def _flat(saved):
    out = []
    for t in saved:
        out += _flat(t) if isinstance(t, (tuple, list)) else [t] if t is not None else []
    return out


def _run(m, on, feat, action, noise, gout, only_z=False, heads=CHAIN_HEADS):
    """A grad-mode sample_posterior and its backward on the given grad_outputs -> (outputs, saved tensors, {name: gradient})."""
    m.fused_chain_grad = on
    try:
        feat, action = feat.clone().requires_grad_(True), action.clone().requires_grad_(True)
        mean, std, z1, z2 = m.sample_posterior(feat, action, noise)
        node = mean.grad_fn
        assert node is not None and m.chain_state_bytes > 0 and bool(node.fused) == on
        saved = [t.clone() for t in _flat(node.saved)]
        assert m.chain_state_bytes == sum(t.numel() * 4 for t in _flat(node.saved[3:]))
        keys, params = _head_params(m, heads)
        outs, gs = ([z1, z2], gout[2:]) if only_z else ([mean, std, z1, z2], gout)
        m.fused_chain_grad = not on                              # the backward follows what the forward did, not the attribute
        grads = torch.autograd.grad(outs, [feat, action] + params, grad_outputs=gs, allow_unused=True)
        torch.cuda.synchronize()
        named = dict(zip(["dfeat", "daction"] + keys, grads))
        return [t.detach().clone() for t in (mean, std, z1, z2)], saved, {k: v.clone() for k, v in named.items() if v is not None}
    finally:
        m.fused_chain_grad = False


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(a, b), (what, int((a.view(torch.int32) != b.view(torch.int32)).sum()), a.numel())


def _compare(want, got, T, what):
    for name, a, b in zip(("mean", "std", "z1", "z2"), got[0], want[0]):
        _same(a, b, what + (name,))
    assert len(got[1]) == len(want[1]) == (10 if T == 1 else 18)
    for i, (a, b) in enumerate(zip(got[1], want[1])):
        if T == 1 and i == 3:                                    # xz of a chain without a step: allocated, written by neither path
            assert a.shape == b.shape
            continue
        _same(a, b, what + ("saved", i))
    assert set(got[2]) == set(want[2])
    for k in want[2]:
        _same(got[2][k], want[2][k], what + (k,))


# ---- 1, 2. forward, saved state and backward, bitwise ---------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("A", AS)
def test_forward_state_and_gradients_equal_the_per_layer_path_bitwise(models, A, T):
    m = models(A)
    for B in BS:
        args = _inputs(B, T, A)
        want, got = _run(m, False, *args), _run(m, True, *args)
        _compare(want, got, T, (A, T, B))
        # T == 1: no action, no chain step -- the chain heads' gradients are zeros there, in both paths
        live = [k for k in want[2] if T > 1 or k.split(".")[0] in ("dfeat", "z1_posterior_init", "z2_prior_init")]
        assert len(want[2]) == (26 if T > 1 else 25) and len(live) == (26 if T > 1 else 13)
        for k in live:
            assert bool(torch.isfinite(got[2][k]).all()) and float(got[2][k].abs().max()) > 0, (A, T, B, k)


def test_all_36_head_gradients_through_the_losses_heads(models):
    """z1_prior and the reward head hang behind the chain: their gradients, and the part of the chain's gradient that arrives through
    them, on random grad_outputs at every output."""
    A, B, T = 6, 17, 9
    m = models(A)
    feat, action, noise, gout = _inputs(B, T, A, seed=2)
    g = torch.Generator().manual_seed(77)
    more = [torch.randn(B, T, Z1, generator=g).cuda(), torch.randn(B, T, Z1, generator=g).cuda(), torch.randn(B, T - 1, generator=g).cuda(),
            torch.randn(B, T - 1, generator=g).cuda()]
    keys, params = _head_params(m)
    assert len(keys) == 36
    res = {}
    try:
        for on in (False, True):
            m.fused_chain_grad = on
            f, a = feat.clone().requires_grad_(True), action.clone().requires_grad_(True)
            mean, std, z1, z2 = m.sample_posterior(f, a, noise)
            z = torch.cat([z1, z2], dim=-1)
            outs = [mean, std, z1, z2, *m.sample_prior(a, z2), *m.predict_reward(z[:, 0], z[:, 1:], a)]
            grads = torch.autograd.grad(outs, [f, a] + params, grad_outputs=gout + more)
            torch.cuda.synchronize()
            res[on] = dict(zip(["dfeat", "daction"] + keys, [t.clone() for t in grads]))
    finally:
        m.fused_chain_grad = False
    for k in res[False]:
        _same(res[True][k], res[False][k], k)
        assert bool(torch.isfinite(res[True][k]).all()) and float(res[True][k].abs().max()) > 0, k


def test_only_z_has_a_gradient(models):
    A, B, T = 6, 17, 9
    m = models(A)
    args = _inputs(B, T, A, seed=1)
    want, got = _run(m, False, *args, only_z=True), _run(m, True, *args, only_z=True)
    _compare(want, got, T, ("only z",))
    assert all(float(v.abs().max()) > 0 for v in got[2].values())


# ---- 3. row independence of the backward ---------------------------------------------------------------------------------------------
def test_backward_rows_do_not_depend_on_their_tile(models):
    A, T = 6, 9
    m = models(A)
    feat, action, noise, gout = _inputs(33, T, A)
    full = _run(m, True, feat, action, noise, gout)[2]
    for row in (0, 32):                                      # the first row of the first tile, the only row of the last one
        r = slice(row, row + 1)
        alone = _run(m, True, feat[r], action[r], noise[r], [t[r] for t in gout])[2]
        for k in ("dfeat", "daction"):
            _same(alone[k][0], full[k][row], (row, k))
    bad = 16                                                 # the first row of the second tile; rows 17..31 share its tile
    gnan = [t.clone() for t in gout]
    gnan[2][bad] = float("nan")
    gnan[3][bad] = float("nan")
    got = _run(m, True, feat, action, noise, gnan)[2]
    others = [r for r in range(33) if r != bad]
    assert bool(torch.isnan(got["dfeat"][bad]).all())
    for k in ("dfeat", "daction"):
        _same(got[k][others], full[k][others], ("nan", k))


# ---- 4. only the declared outputs are written ------------------------------------------------------------------------------------------
def _v3(t, B, T):
    return t.as_strided((B, T, t.shape[1]), (T * t.stride(0), t.stride(0), 1))


def _per_layer_chain_bwd(m, noise, dmean, dstd, dz, sv, xz, B, S):
    """The loop of _PosteriorFn.backward out of the existing entry points -> drawa, dh2a, dh1a, drawb, dh2b, dh1b, dxz."""
    from s2p_amd import ops
    from s2p_amd._lib import ACT_LRELU, ACT_NONE
    g1, g2 = m.z1_posterior, m.z2_prior
    p1, p2 = g1.packed(), g2.packed()
    h1a, h2a, rawa, h1b, h2b, rawb = sv
    f = lambda *s: torch.full(s, float("nan"), device="cuda")
    drawa, dh2a, dh1a, drawb, dh2b, dh1b, dxz = f(S, B, 64), f(S, B, HID), f(S, B, HID), f(S, B, 512), f(S, B, HID), f(S, B, HID), f(S, B, Z)
    for t in range(S, 0, -1):
        s = t - 1
        ops.gauss_head_bwd(rawb[s], Z2, drawb[s], eps=noise[:, t, Z1:], dz=dz[:, t, Z1:], dz2=dxz[t][:, Z1:] if t < S else None)
        ops.linear_add_bwd(drawb[s], None, 512, ACT_NONE, w_bwd=p2["w3t"], dx=dh2b[s])
        ops.linear_add_bwd(dh2b[s], h2b[s], HID, ACT_LRELU, 0.2, w_bwd=p2["w2t"], dx=dh1b[s])
        ops.linear_add_bwd(dh1b[s], h1b[s], HID, ACT_LRELU, 0.2, w_bwd=p2["g1"][0][1], dx=dxz[s])
        ops.gauss_head_bwd(rawa[s], Z1, drawa[s], eps=noise[:, t, :Z1], dmean=dmean[:, t], dstd=dstd[:, t], dz=dz[:, t, :Z1], dz2=dxz[s][:, :Z1])
        ops.linear_add_bwd(drawa[s], None, 64, ACT_NONE, w_bwd=p1["w3t"], dx=dh2a[s])
        ops.linear_add_bwd(dh2a[s], h2a[s], HID, ACT_LRELU, 0.2, w_bwd=p1["w2t"], dx=dh1a[s])
        ops.linear_add_bwd(dh1a[s], h1a[s], HID, ACT_LRELU, 0.2, w_bwd=p1["g1"][0][1], dx=dxz[s][:, Z1:], accumulate=True)
    torch.cuda.synchronize()
    return drawa, dh2a, dh1a, drawb, dh2b, dh1b, dxz


def test_only_the_declared_outputs_are_written(models):
    from s2p_amd import ops
    from s2p_amd.slac import _PosteriorFn
    A, B, T = 6, 17, 9
    S = T - 1
    m = models(A)
    feat, action, noise, gout = _inputs(B, T, A)
    want_out, want_saved, _ = _run(m, False, feat, action, noise, gout)
    packs = [getattr(m, h).packed() for h in CHAIN_HEADS]
    ra, rb = _PosteriorFn._hoisted(feat, action, packs[2], packs[3])[2:]
    # forward: eps, mean, std, z with odd pitches and offsets, every state buffer dense between two guard bands
    eps = Region(B * T, Z, pitch=Z + 12, off=8, fill=noise.reshape(B * T, Z))
    mean, std, z = Region(B * T, Z1, pitch=40, off=4), Region(B * T, Z1, pitch=36, off=0), Region(B * T, Z, pitch=320, off=16)
    dense = lambda rows, w: Region(rows, w, pitch=w, off=0)
    a0, b0 = [dense(B, HID), dense(B, HID), dense(B, 64)], [dense(B, HID), dense(B, HID), dense(B, 512)]
    chain = [dense(S * B, HID), dense(S * B, HID), dense(S * B, 64), dense(S * B, HID), dense(S * B, HID), dense(S * B, 512), dense(S * B, Z)]
    state = ops.chain_state([r.v for r in a0], [r.v for r in b0], [r.v for r in chain])
    ins = [feat, ra, rb, eps.buf] + [p.detach() for p in m._chain_params()]
    ins0 = [t.clone() for t in ins]
    ops.posterior_chain_fwd_save(feat[:, 0], ra, rb, _v3(eps.v, B, T), [ops.chain_mlp(p) for p in packs], _v3(mean.v, B, T),
                                 _v3(std.v, B, T), _v3(z.v, B, T), state)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ins, ins0))
    zb = z.bits("z").view(B, T, Z)
    for name, a, b in zip(("mean", "std", "z1", "z2"), (mean.bits("mean").view(B, T, Z1), std.bits("std").view(B, T, Z1), zb[..., :Z1], zb[..., Z1:]),
                          want_out):
        _same(a, b.cpu(), ("direct", name))
    # want_saved: feat, noise, z, xz, a0 (3), b0 (3), xa, xb, h1a, h2a, rawa, h1b, h2b, rawb
    for name, r, w in zip(("a0.h1", "a0.h2", "a0.raw", "b0.h1", "b0.h2", "b0.raw"), a0 + b0, want_saved[4:10]):
        _same(r.bits(name).view(w.shape), w.cpu(), ("state", name))
    for name, r, w in zip(("h1a", "h2a", "rawa", "h1b", "h2b", "rawb", "xz"), chain, want_saved[12:18] + [want_saved[3]]):
        _same(r.bits(name).view(w.shape), w.cpu(), ("state", name))
    # backward: dz, dmean, dstd with odd pitches and offsets, the seven outputs dense between guard bands
    dz = Region(B * T, Z, pitch=Z + 20, off=12, fill=torch.cat(gout[2:], dim=-1).reshape(B * T, Z))
    dmean = Region(B * T, Z1, pitch=44, off=8, fill=gout[0].reshape(B * T, Z1))
    dstd = Region(B * T, Z1, pitch=33, off=1, fill=gout[1].reshape(B * T, Z1))
    outs = [dense(S * B, 64), dense(S * B, HID), dense(S * B, HID), dense(S * B, 512), dense(S * B, HID), dense(S * B, HID), dense(S * B, Z)]
    sv = [r.v.view(S, B, -1) for r in chain[:6]]
    want = _per_layer_chain_bwd(m, noise, gout[0].contiguous(), gout[1].contiguous(), torch.cat(gout[2:], dim=-1), sv, None, B, S)
    bufs = [r.buf for r in a0 + b0 + chain] + [dz.buf, dmean.buf, dstd.buf, eps.buf]
    bufs0 = [t.clone() for t in bufs]
    ops.posterior_chain_bwd(_v3(eps.v, B, T), _v3(dmean.v, B, T), _v3(dstd.v, B, T), _v3(dz.v, B, T),
                            [ops.chain_mlp_bwd(packs[2]), ops.chain_mlp_bwd(packs[3])], state, [r.v.view(S, B, -1) for r in outs])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs, bufs0))                   # gradients in, noise and the saved state: unchanged
    assert all(torch.equal(a, b) for a, b in zip(ins, ins0))                     # ... and the weights
    for name, r, w in zip(("drawa", "dh2a", "dh1a", "drawb", "dh2b", "dh1b", "dxz"), outs, want):
        got = r.bits(name).view(w.shape)
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0, name
        _same(got, w.cpu(), ("grads", name))


# ---- 5. both gauss_sigmoid / softplus branches -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,D", [(("z1_posterior_init", "z1_posterior"), Z1), (("z2_prior_init", "z2_prior"), Z2)])
@pytest.mark.parametrize("bias", [30.0, -30.0])
def test_both_sigmoid_branches(hip_device, bias, heads, D):
    """raw_std = +-30 + O(1): gauss_sigmoid is 1 / (1 + e) on one side and e / (1 + e) ~ 1e-13 on the other, softplus likewise (see
    test_posterior_chain_gpu.py::test_both_softplus_branches).  softplus(0) = ln 2 separates the runs."""
    A, B, T = 6, 17, 2
    m = build_model(A)
    with torch.no_grad():
        for h in heads:
            getattr(m, h).net._modules["4"].bias[D:] = bias
    args = _inputs(B, T, A, seed=4)
    want, got = _run(m, False, *args), _run(m, True, *args)
    _compare(want, got, T, (bias, D))
    assert all(bool(torch.isfinite(t).all()) for t in got[0] + list(got[2].values()))
    # the t = 0 head sees inputs of O(1): every raw_std is on the branch of its bias.  The chain head of a +-30 run sees z of that
    # size and its raw_std spreads, so there the branch is only required to occur.
    first, chain = (got[1][i][..., D:2 * D] for i in ((6, 14) if D == Z1 else (9, 17)))
    assert (float(first.min()) > 0 and bool((chain > 0).any())) if bias > 0 else (float(first.max()) < 0 and bool((chain < 0).any()))
    if D == Z1:
        sd = got[0][1]
        print("bias %+.0f: z1 std in [%.6e, %.6e]" % (bias, float(sd.min()), float(sd.max())))
        assert (float(sd.min()) > LN2) if bias > 0 else (float(np.float32(1e-5)) <= float(sd.min()) and float(sd.max()) < LN2)


# ---- 6. call counts ------------------------------------------------------------------------------------------------------------------------
def test_one_call_per_direction_replaces_the_per_layer_calls(hip_device):
    A, B, T = 6, 17, 9
    S = T - 1
    m = build_model(A)                                       # a model whose switch no test has touched
    feat, action, noise, gout = _inputs(B, T, A)
    params = _head_params(m, CHAIN_HEADS)[1]

    def counts(on):
        if on is not None:
            m.fused_chain_grad = on
        box = {}

        def fwd():
            f, a = feat.clone().requires_grad_(True), action.clone().requires_grad_(True)
            box["in"], box["out"] = [f, a], m.sample_posterior(f, a, noise)
        cf = count_calls(fwd)
        cb = count_calls(lambda: torch.autograd.grad(box["out"], box["in"] + params, grad_outputs=gout))
        torch.cuda.synchronize()
        return cf, cb
    never = counts(None)
    on, off = counts(True), counts(False)
    print("library calls, forward: per-layer", off[0], " fused", on[0])
    print("library calls, backward: per-layer", off[1], " fused", on[1])
    assert never == off and all(FWD not in c and BWD not in c for c in off)
    assert on[0].get(FWD) == 1 and BWD not in on[0] and on[1].get(BWD) == 1 and FWD not in on[1]
    assert "s2p_gauss_head_fwd" not in on[0] and "s2p_linear_add_fwd" not in on[0] and set(on[0]) <= {FWD, "s2p_linear_fwd"}
    assert on[0].get("s2p_linear_fwd") == 2 and off[0]["s2p_gauss_head_fwd"] == 2 * T
    assert off[1]["s2p_gauss_head_bwd"] == 2 * T and on[1]["s2p_gauss_head_bwd"] == 2
    assert off[1]["s2p_linear_add_bwd"] - on[1]["s2p_linear_add_bwd"] == 6 * S
    rest = lambda c: {k: v for k, v in c.items() if k not in (BWD, "s2p_gauss_head_bwd", "s2p_linear_add_bwd")}
    assert rest(on[1]) == rest(off[1])


# ---- 7. pinned parity ------------------------------------------------------------------------------------------------------------------------
def test_fused_grad_path_matches_the_recorded_reference(models, capsys):
    """calculate_loss + backward on the inputs of tests/slac_latent_ref.py against the recorded reference, the rule of
    tests/test_slac_latent.py.  Measured on an MI355X, deviation / max(ref32_err, 1e-6), worst per group, identical with the switch
    on and off: losses (KL, reward) 0.289, samples 0.665, head gradients 1.902 (the bound is 4).  The image loss VALUE ends in one atomicAdd per workgroup (gauss.hip) and may differ in its
    last bits between two calls of ONE path, so the equality of the two paths is asserted on everything else."""
    G = np.load(os.path.join(HERE, "golden", "slac_latent_golden_v1.npz"))
    m = models(R.A)
    state_u8, action, reward, done, noise = R.make_inputs()
    state = (state_u8.double() / 255.0).float()
    keys = _head_params(m)[0]
    assert len(keys) == 36
    worst, calls = {}, {}
    try:
        for on in (False, True):
            m.fused_chain_grad = on
            m.zero_grad(set_to_none=True)
            ratios = {}

            def note(group, err, ref, what):
                ref = max(float(ref), FLOOR)
                ratios[group] = max(ratios.get(group, 0.0), err / ref)
                assert err <= K_TOL * ref, (on, group, what, err, K_TOL * ref)

            def step():
                mid = m.sample_posterior(m.encoder(state), action, noise)            # grad mode: the chain keeps its state
                assert mid[0].grad_fn is not None
                losses = m.calculate_loss(state, action, reward, done, noise)
                sum(losses).backward()
                return mid, losses
            box = {}
            calls[on] = count_calls(lambda: box.setdefault("r", step()))
            torch.cuda.synchronize()
            mid, losses = box["r"]
            for i, name in enumerate(("kld", "image", "reward")):
                err = abs(float(losses[i]) - float(G["losses"][i])) / abs(float(G["losses"][i]))
                note("losses" if name != "image" else "image loss", err, G["losses_ref32_err"][i], name)
            for k, v in zip(("post_mean", "post_std", "z1", "z2"), mid):
                note("samples", R.rel_max(v.detach(), G["mid." + k]), G["mid.%s.ref32_err" % k], k)
            named = dict(m.named_parameters())
            for k in keys:
                errs = R.grad_measures(named[k].grad, float(G["grad.%s.sum" % k]), float(G["grad.%s.l2" % k]), G["grad.%s.samp" % k])
                for e, r, w in zip(errs, G["grad.%s.ref32_err" % k], ("l2", "sum", "samp")):
                    note("head gradients", e, r, k + ":" + w)
            worst[on] = ratios
    finally:
        m.fused_chain_grad = False
        m.zero_grad(set_to_none=True)
    with capsys.disabled():
        print("\nworst deviation / max(ref32_err, 1e-6): per-layer %s, fused %s" % (
            {k: round(v, 6) for k, v in worst[False].items()}, {k: round(v, 6) for k, v in worst[True].items()}))
    assert calls[True].get(FWD) == 2 and calls[True].get(BWD) == 1 and FWD not in calls[False]
    for group in ("losses", "samples", "head gradients"):
        assert worst[True][group] == worst[False][group], group
    assert max(v for k, v in worst[True].items() if k != "image loss") == max(v for k, v in worst[False].items() if k != "image loss")


# ---- 8. end to end ---------------------------------------------------------------------------------------------------------------------------
def test_two_update_latent_steps_train_the_same_model(hip_device):
    from s2p_amd.slac_algo import SlacAlgorithm

    def train(on):
        a = SlacAlgorithm((3, 100, 100), (SB.A,), 1, hip_device, seed=0, batch_size_latent=2, buffer_size=32, num_sequences=SB.S,
                          frame_capacity=128, fused_chain_grad=on)
        assert a.latent.fused_chain_grad is on and a.latent.fused_chain is False
        a.latent.load_state_dict(R.full_state_dict(R.make_params(SB.A)), strict=True)
        a.load_data_in_buffer(SB.real_dataset(2, 12, 100, 100), **dict(SB.LOAD_ARGS["real"], data_num=24))
        np.random.seed(5)
        torch.manual_seed(5)
        torch.cuda.manual_seed(5)
        calls = count_calls(lambda: [a.update_latent() for _ in range(2)])
        torch.cuda.synchronize()
        assert calls.get(FWD, 0) == (2 if on else 0) and calls.get(BWD, 0) == (2 if on else 0)
        return {k: v.detach().clone() for k, v in a.latent.named_parameters()}, R.full_state_dict(R.make_params(SB.A))
    (off, start), (on, _), (again, _) = train(False), train(True), train(True)
    assert len(off) == 60
    for k in off:
        assert bool(torch.isfinite(on[k]).all()) and not torch.equal(on[k].cpu(), torch.as_tensor(start[k], dtype=torch.float32)), k
        _same(on[k], off[k], ("on / off", k))
        _same(again[k], on[k], ("on / on", k))
