"""N3n -- the bf16 compute mode of the fused closed-loop imagination chain (csrc/gauss_chain_bf16.hip: s2p_imagine_chain_fwd_bf16,
`LatentModel.imagine(..., compute="bf16")`, `TanhGaussianPolicy.packed_bf16`).

As for N3m (tests/test_chain_bf16_gpu.py) a free-running comparison against an fp64 run is no test of this chain: rounding flips at the
bf16 boundaries travel down the rollout.  The kernel is tied down from three sides instead:
  * POLICY half, EXACT data (tests/imagine_bf16_ref.py: every operand and hidden activation a bf16 number, every fp32 sum exact):
    a(0) is bitwise the a(0) of the fp32 per-layer `imagine`;
  * LATENT half, random data: `predict` in N3m's mode (s2p_prior_chain_fwd_bf16, verified there) on the launch's own actions and the
    same noise returns its z1_mean, z1_std and z BITWISE -- which also pins the fp32 action terms to the hoisted GEMM's bits;
  * POLICY half, RANDOM data, teacher-forced: a(h) against the fp64 rule on the kernel's own z(h); every (row, step) within the LOOSE
    bound = 4 x the largest deviation of the helper's own fp32 runs (two summation orders), at most 5 % of the pairs outside 4e-6.
Shapes: B in {1, 15, 16, 17, 33} (a partial tile, one tile, one row more, three workgroups), H in {1, 2, 8}, A in {6, 1, 8} (both
paddings of the action chunk, the widest), W in {128, 384, 1024} (one column tile per wave, an odd tile count, the LDS ceiling)."""
import pytest
import torch

import chain_bf16_ref as C
import imagine_bf16_ref as IB
import slac_imagine_ref as IM
from guard_region import Region
from slac_chain_util import count_calls, model_cache

pytestmark = pytest.mark.gpu
Z1, Z2, Z = 32, 256, 288
BS, HS, AS, WS = (1, 15, 16, 17, 33), (1, 2, 8), (6, 1, 8), (128, 384, 1024)
NAME = IB.NAME
OUT = ("actions", "mean", "std", "z")


def _make_policy(W, A, sd=None):
    from s2p_amd.offline_rl import TanhGaussianPolicy
    hid = list(W) if isinstance(W, (tuple, list)) else [W, W]
    return TanhGaussianPolicy(hidden_sizes=hid, obs_dim=Z, action_dim=A).load_state_dict(sd if sd is not None else IM.make_policy_params(W, A))


@pytest.fixture(scope="module")
def models(hip_device):
    """action width -> a LatentModel with the seeded weights of tests/slac_latent_ref.py; left with fused_chain False, chain_compute fp32."""
    return model_cache()


@pytest.fixture(scope="module")
def policies(hip_device):
    cache = {}

    def get(W, A):
        if (W, A) not in cache:
            cache[W, A] = _make_policy(W, A)
        return cache[W, A]
    return get


def _inputs(B, H, seed=0):
    g = torch.Generator().manual_seed(4100 + seed)
    z0, noise = torch.randn(33, Z, generator=g), torch.randn(33, 8, Z, generator=g)      # row b, step h are the same whatever B and H are
    return z0[:B].cuda().contiguous(), noise[:B, :H].cuda().contiguous()


def _imagine(m, po, z0, noise, fused=True, chain_compute="fp32", **kw):
    m.fused_chain, m.chain_compute = fused, chain_compute
    try:
        with torch.enable_grad():
            out = m.imagine(po, z0, noise.shape[1], noise, **kw)
        torch.cuda.synchronize()
        assert all(t.grad_fn is None for t in out)
        return [t.clone() for t in out]
    finally:
        m.fused_chain, m.chain_compute = False, "fp32"


def _bf16(m, po, z0, noise):
    return _imagine(m, po, z0, noise, compute="bf16")


def _predict_bf16(m, z0, actions, noise):
    m.fused_chain, m.chain_compute = True, "bf16"
    try:
        out = m.predict(z0, actions, noise)
        torch.cuda.synchronize()
        return [t.clone() for t in out]
    finally:
        m.fused_chain, m.chain_compute = False, "fp32"


# ---- 1. the switch -----------------------------------------------------------------------------------------------------------------------------
def test_the_switch(models, policies):
    A, B, H = 6, 17, 2
    m, po = models(A), policies(128, A)
    z0, noise = _inputs(B, H)
    per_layer = _imagine(m, po, z0, noise, fused=False)
    got, calls = {}, {}
    for cc in ("fp32", "bf16"):                              # `chain_compute` does not reach imagine
        for fused in (False, True):
            for kw in ({}, {"compute": "fp32"}):
                key = (cc, fused, bool(kw))
                calls[key] = count_calls(lambda: got.__setitem__(key, _imagine(m, po, z0, noise, fused, cc, **kw)))
                assert calls[key] == ({"s2p_imagine_chain_fwd": 1} if fused else
                                      {"s2p_linear_fwd": 9 * H, "s2p_linear_add_fwd": 2 * H, "s2p_gauss_head_fwd": 2 * H}), key
                assert all(torch.equal(a, b) for a, b in zip(got[key], per_layer)), key
        calls[cc] = count_calls(lambda: got.__setitem__(cc, _imagine(m, po, z0, noise, True, cc, compute="bf16")))
        assert calls[cc] == {NAME: 1}
    assert all(torch.equal(a, b) for a, b in zip(got["fp32"], got["bf16"]))
    act, mean, std, z = got["bf16"]
    assert [tuple(t.shape) for t in got["bf16"]] == [(B, H, A), (B, H, Z1), (B, H, Z1), (B, H, Z)]
    assert all(bool(torch.isfinite(t).all()) for t in got["bf16"]) and float(act.abs().max()) <= 1 and float(std.min()) > 0
    differ = float((z != per_layer[3]).float().mean())
    print("%.1f %% of z differs from the fp32 chain; max |dz| %.3e" % (100 * differ, float((z - per_layer[3]).abs().max())))
    assert differ > 0.5
    with pytest.raises(ValueError, match="fused"):
        _imagine(m, po, z0, noise, fused=False, compute="bf16")
    with pytest.raises(ValueError, match="compute"):
        _imagine(m, po, z0, noise, compute="fp16")
    with pytest.raises(ValueError, match="compute"):
        _imagine(m, po, z0, noise, fused=False, compute=None)
    for bad in (_make_policy(192, A), _make_policy((256, 128), A, {**IM.make_policy_params(256, A), **_tail(256, 128, A)})):
        with pytest.raises(ValueError, match="128"):
            _imagine(m, bad, z0, noise, compute="bf16")
    # empty batches and horizons: no launch
    assert count_calls(lambda: _imagine(m, po, z0[:0], noise[:0], compute="bf16")) == {}
    assert [tuple(t.shape) for t in _imagine(m, po, z0, noise[:, :0], compute="bf16")] == [(B, 0, A), (B, 0, Z1), (B, 0, Z1), (B, 0, Z)]
    # sample False: the mean rollout, noise unused
    a, b = _imagine(m, po, z0, noise, compute="bf16", sample=False), _bf16(m, po, z0, torch.zeros_like(noise))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(a[3][:, 0, :Z1], a[1][:, 0])


def _tail(w0, w1, a):
    g = torch.Generator().manual_seed(17)
    return {"fc1.weight": (torch.rand(w1, w0, generator=g) * 2 - 1) / w0 ** 0.5, "fc1.bias": torch.randn(w1, generator=g) * 0.05,
            "last_fc.weight": (torch.rand(a, w1, generator=g) * 2 - 1) * 7.0 / w1 ** 0.5,
            "last_fc_log_std.weight": (torch.rand(a, w1, generator=g) * 2 - 1) * 1e-3}


# ---- 2. policy half, exact data ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,A", [(128, 6), (384, 1), (1024, 8), (384, 6)])
def test_policy_on_exact_data_is_the_fp32_policy_bitwise(models, W, A):
    m = models(A)
    sd, z0 = IB.exact_policy(W, A), IB.exact_z0(33)
    IB.assert_exact_premises(sd, z0)
    po = _make_policy(W, A, sd)
    noise = torch.zeros(33, 1, Z).cuda()
    want = _imagine(m, po, z0.cuda(), noise, fused=False)[0][:, 0]           # the fp32 per-layer path, once, at B = 33
    assert len(torch.unique(want)) > 4
    for B in BS:
        got = _bf16(m, po, z0[:B].cuda(), noise[:B])[0][:, 0]
        diff = int((got.view(torch.int32) != want[:B].contiguous().view(torch.int32)).sum())
        print("W %d A %d B %2d: a(0) elements that differ from the fp32 policy's: %d of %d" % (W, A, B, diff, got.numel()))
        assert torch.equal(got, want[:B]), (W, A, B, diff)


# ---- 3. latent half, random data -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,A", [(128, 6), (384, 1), (1024, 8)])
def test_predict_in_bf16_mode_under_the_imagined_actions_is_bitwise_the_rollout(models, policies, W, A):
    m, po = models(A), policies(W, A)
    for H in HS:
        for B in BS if W != 1024 else (17,):
            z0, noise = _inputs(B, H)
            act, mean, std, z = _bf16(m, po, z0, noise)
            got = _predict_bf16(m, z0, act, noise)
            for name, a, b in zip(OUT[1:], got, (mean, std, z)):
                assert torch.equal(a, b), (W, A, B, H, name, int((a != b).sum()))
            assert float(act.abs().max()) > 0.3 and float(act.abs().max()) <= 1


# ---- 4. policy half, random data, teacher-forced ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [128, 1024])
def test_policy_teacher_forced_on_random_data(models, W, capsys):
    """Measured on an MI355X, 297 (row, step) pairs each: W 128: 0 pairs outside 4e-6, worst 1.060e-07, loose bound 4 x 1.053e-04;
    W 1024: 5 pairs (1.68 %) outside, worst 1.946e-04 (a rounding flip of a hidden activation), worst of the others 1.700e-06, loose
    bound 4 x 1.294e-03.  The rule's own fp32 runs on the CPU leave 1 (W 128) and 6 to 9 (W 1024) pairs outside (tests/test_imagine_bf16.py)."""
    A, B, H = 6, 33, 3
    m = models(A)
    loose, devs = 0.0, []
    for seed in (0, 1, 2):
        sd, z0, noise = IB.random_case(W, seed, B, H, A)
        po = _make_policy(W, A, sd)
        act, _, _, z = [t.cpu() for t in _bf16(m, po, z0.cuda(), noise.cuda())]
        x = IB.rollout_inputs(z0, z)                                          # the kernel's own z(h): what its policy read
        ref = IB.policy_rule(sd, x, torch.float64)
        for gen in (None, torch.Generator().manual_seed(9 + seed)):
            loose = max(loose, float(IB.action_deviation(IB.policy_rule(sd, x, torch.float32, gen), ref).max()))
        devs.append(IB.action_deviation(act, ref))
    dev = torch.cat(devs)
    miss = int((dev > IB.TIGHT).sum())
    clean = float(dev[dev <= IB.TIGHT].max())
    with capsys.disabled():
        print("\nW %d teacher-forced: %d (row, step) pairs, %d (%.2f %%) not tight, worst %.3e, worst tight %.3e; loose bound 4 x %.3e = %.3e"
              % (W, dev.numel(), miss, 100.0 * miss / dev.numel(), float(dev.max()), clean, loose, IB.K_TOL * loose))
    assert dev.numel() == 297
    assert float(dev.max()) <= IB.K_TOL * loose
    assert miss <= IB.CAP * dev.numel()


# ---- 5. rows and determinism -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [128, 384])
def test_rows_do_not_depend_on_their_tile_and_calls_repeat(models, policies, W):
    m, po = models(6), policies(W, 6)
    z0, noise = _inputs(33, 8)
    full, again = _bf16(m, po, z0, noise), _bf16(m, po, z0, noise)
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    for row in (0, 32):                                      # the first row of the first tile, the only row of the last one
        alone = _bf16(m, po, z0[row:row + 1], noise[row:row + 1])
        for name, a, b in zip(OUT, alone, full):
            assert torch.equal(a[0], b[row]), (row, name)
    bad = 16                                                 # the first row of the second tile; rows 17..31 share its tile
    z0_nan = z0.clone()
    z0_nan[bad] = float("nan")
    got = _bf16(m, po, z0_nan, noise)
    others = [r for r in range(33) if r != bad]
    for name, a, b in zip(OUT, got, full):
        assert torch.equal(a[others], b[others]), name
        if name != "actions":                                # relu(NaN) = 0, as in the fp32 chain: the poisoned row's actions are finite
            assert bool(torch.isnan(a[bad]).all()), name


# ---- 6. nothing else is written ----------------------------------------------------------------------------------------------------------------------
def _v3(t, B, T):
    return t.as_strided((B, T, t.shape[1]), (T * t.stride(0), t.stride(0), 1))


@pytest.mark.parametrize("layout", ["aligned", "odd"])
@pytest.mark.parametrize("W,A", [(128, 6), (384, 1)])
def test_only_the_four_outputs_are_written(models, policies, layout, W, A):
    """aligned: pitches and offsets that are multiples of 4 floats (the kernel's 16-byte loads of eps and stores of mean, std, z);
    odd: neither (its 4-byte ones).  z0 is 16-byte aligned in both: the entry point requires it."""
    from s2p_amd import ops
    B, H = 17, 2
    m, po = models(A), policies(W, A)
    z0, noise = _inputs(B, H)
    want = _bf16(m, po, z0, noise)
    odd = layout == "odd"
    z0r = Region(B, Z, pitch=300, off=4, fill=z0)
    eps = Region(B * H, Z, pitch=Z + 12 + odd, off=8 - odd, fill=noise.reshape(B * H, Z))
    act = Region(B * H, A, pitch=12 - odd, off=4 - odd)      # exactly A columns are written, not pad4(A)
    mean, std = Region(B * H, Z1, pitch=40 + odd, off=4 - odd), Region(B * H, Z1, pitch=36 + odd, off=odd)
    z = Region(B * H, Z, pitch=320 + odd, off=16 - 3 * odd)
    packs = [m.z1_prior.packed_bf16(k1=Z2), m.z2_prior.packed_bf16()]
    wc, wb = m.z1_prior.packed_cols(Z2, Z2 + A), m.z2_prior.packed()["g1"][1][0]
    pk = po.packed_bf16()
    snap = lambda: [t.clone() for q in packs for t in (q["w1"], q["b1"], q["w2"], q["b2"], q["w3"], q["b3"])] + \
        [t.clone() for t in pk["w"]] + [wc.clone(), wb.clone(), po.flat.clone(), z0r.buf.clone(), eps.buf.clone()] + \
        [q.detach().clone() for q in m.z1_prior.layer_params() + m.z2_prior.layer_params()]
    before = snap()
    ops.imagine_chain_fwd_bf16(z0r.v, _v3(eps.v, B, H), [ops.chain_mlp_bf16(q) for q in packs], wc, wb, A, ops.policy_mlp_bf16(po),
                               _v3(act.v, B, H), _v3(mean.v, B, H), _v3(std.v, B, H), _v3(z.v, B, H))
    torch.cuda.synchronize()
    assert po.packed_bf16() is pk
    assert all(torch.equal(a, b) for a, b in zip(before, snap()))
    got = [act.bits("actions").view(B, H, A), mean.bits("mean").view(B, H, Z1), std.bits("std").view(B, H, Z1), z.bits("z").view(B, H, Z)]
    for name, a, b in zip(OUT, got, want):
        assert torch.equal(a, b.cpu()), (layout, name)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_their_messages(models, policies):
    from s2p_amd import _lib, ops
    assert IB.check_refusals(_lib) == len(IB.REFUSALS)
    # through the wrappers: a refusal is a RuntimeError carrying the message, and nothing was written
    A, B, H = 6, 17, 2
    m, po = models(A), policies(128, A)
    z0, noise = _inputs(B, H)
    outs = [Region(B * H, w) for w in (A, Z1, Z1, Z)]
    mlps = [ops.chain_mlp_bf16(m.z1_prior.packed_bf16(k1=Z2)), ops.chain_mlp_bf16(m.z2_prior.packed_bf16())]
    wc, wb = m.z1_prior.packed_cols(Z2, Z2 + A), m.z2_prior.packed()["g1"][1][0]
    call = lambda z0_, mlps_, pol: ops.imagine_chain_fwd_bf16(z0_, _v3(noise.reshape(B * H, Z), B, H), mlps_, wc, wb, A, pol,
                                                              *[_v3(r.v, B, H) for r in outs])
    with pytest.raises(RuntimeError, match="z0 must be 16-byte aligned"):
        call(torch.zeros(B, Z + 1, device="cuda")[:, 1:], mlps, ops.policy_mlp_bf16(po))
    with pytest.raises(RuntimeError, match="first layer's K is 288, 256 is built"):
        call(z0, mlps[::-1], ops.policy_mlp_bf16(po))
    bad = ops.policy_mlp_bf16(po)
    bad.width = 192
    with pytest.raises(RuntimeError, match="hidden width 192"):
        call(z0, mlps, bad)
    assert all(r.untouched() for r in outs)


# ---- 8. no stale pack ------------------------------------------------------------------------------------------------------------------------------------
def test_the_policy_pack_follows_the_parameters(models, hip_device):
    from s2p_amd.offline_rl import _Adam
    A, W = 6, 128
    m = models(A)
    z0, noise = _inputs(17, 2)
    po = _make_policy(W, A)
    pk = po.packed_bf16()
    assert po.packed_bf16() is pk                                                   # not re-made while no parameter changed
    assert [tuple(w.shape) for w in pk["w"]] == [(W, Z), (W, W), (2 * A, W)] and all(w.dtype == torch.bfloat16 and w.is_contiguous() for w in pk["w"])
    for li in range(3):
        assert torch.equal(pk["w"][li], po.packed.w(po.flat, li).to(torch.bfloat16))
        assert pk["b"][li].dtype == torch.float32 and pk["b"][li].data_ptr() == po.packed.b(po.flat, li).data_ptr()
    first = _bf16(m, po, z0, noise)
    other = IM.make_policy_params(W, A, seed=77)
    po.load_state_dict(other)
    assert po.packed_bf16() is not pk
    got, fresh = _bf16(m, po, z0, noise), _bf16(m, _make_policy(W, A, other), z0, noise)
    assert all(torch.equal(a, b) for a, b in zip(got, fresh)) and not torch.equal(got[0], first[0])
    # the trainers' optimizer writes `flat` in a launch of its own: the pack follows that too
    pk = po.packed_bf16()
    po.grad.fill_(1.0)
    _Adam(po.flat, po.grad, lr=1e-2).step()
    torch.cuda.synchronize()
    new = po.packed_bf16()
    assert new is not pk and torch.equal(new["w"][1], po.packed.w(po.flat, 1).to(torch.bfloat16)) and not torch.equal(new["w"][1], pk["w"][1])
