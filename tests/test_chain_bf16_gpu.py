"""N3m -- the bf16 compute mode of the two fused no-grad latent chains (csrc/gauss_chain_bf16.hip, `LatentModel.chain_compute`).

A free-running comparison against an fp64 run under the project's "4 x ref32_err" rule is no test of this chain: an fp32 activation
next to a bf16 rounding boundary rounds the other way than its fp64 twin, such flips are frequent and travel down the chain, and the
reference's own fp32 error (2 to 5e-3) is as large as the distance of the bf16 mode from the fp32 chain.  Two tests replace it:
  1. EXACT data (tests/chain_bf16_ref.py: every fp32 sum is exact in any order, so no flip exists): mean and z are torch.equal to the
     rule's fp64 run, std is within 4 ulp of it (the device's and the host's softplus differ by ulps on the same raw).
  2. RANDOM data, teacher-forced: each of the 2 T MLP evaluations is recomputed in fp64 from the kernel's own fp32 z and the hoisted
     terms it was given.  Per (row, MLP): every row within the LOOSE bound = 4 x the largest deviation of the helper's own fp32 runs
     (two summation orders) from its fp64 run on the same cases, and at most 5 % of the rows, pooled, outside the TIGHT bound 4e-6
     (K_TOL x the 1e-6 floor); tests/test_chain_bf16.py holds the helper's fp32 runs to half of that."""
import numpy as np
import pytest
import torch

import chain_bf16_ref as C
import iql_ref as IR
import slac_buffer_ref as SB
import slac_imagine_ref as IM
import slac_latent_ref as R
from guard_region import Region
from slac_chain_util import count_calls, model_cache

pytestmark = pytest.mark.gpu
Z1, Z2, Z, FEAT = 32, 256, 288, 256
BS, TS, HS, AS = (1, 15, 16, 17, 33), (1, 2, 9), (1, 2, 8), (6, 1)
POST, PRIOR = "s2p_posterior_chain_fwd_bf16", "s2p_prior_chain_fwd_bf16"
TIGHT, CAP, K_TOL = 4e-6, 0.05, 4.0
NAMES = ("mean", "std", "z1", "z2")


@pytest.fixture(scope="module")
def models(hip_device):
    """action width -> a LatentModel with the seeded weights of tests/slac_latent_ref.py; left with fused_chain False, chain_compute fp32."""
    return model_cache()


@pytest.fixture(scope="module")
def exact_models(hip_device):
    """action width -> (a LatentModel that loaded C.exact_params(A) through load_state_dict, those parameters)."""
    from s2p_amd.slac import LatentModel
    cache = {}

    def get(A):
        if A not in cache:
            p = C.exact_params(A)
            m = LatentModel((3, 100, 100), (A,), image_size=100)
            m.load_state_dict(R.full_state_dict(p), strict=True)
            cache[A] = (m, p)
        return cache[A]
    return get


def _run(m, compute, fn, fused=True):
    m.fused_chain, m.chain_compute = fused, compute
    try:
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
        assert all(t.grad_fn is None for t in out)
        return [t.clone() for t in out]
    finally:
        m.fused_chain, m.chain_compute = False, "fp32"


def _posterior(m, compute, feat, action, noise, fused=True):
    return _run(m, compute, lambda: m.sample_posterior(feat, action, noise), fused)


def _predict(m, compute, z0, actions, noise, fused=True):
    mean, std, z = _run(m, compute, lambda: m.predict(z0, actions, noise), fused)
    return [mean, std, z[..., :Z1], z[..., Z1:]]


def _ulps(a, b):
    return int((a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs().max())


def _check_exact(tag, got, ref):
    """got: (mean, std, z1, z2) of the device; ref: (mean, std, z) of the rule in fp64."""
    want = [ref[0].float(), ref[1].float(), ref[2][..., :Z1].float(), ref[2][..., Z1:].float()]
    for name, a, b in zip(NAMES, got, want):
        a = a.cpu()
        assert a.shape == b.shape, (tag, name)
        if name == "std":
            print(tag, "std: at most %d ulp from the host's softplus" % _ulps(a, b))
            assert _ulps(a, b) <= 4, (tag, name)
        else:
            assert torch.equal(a, b), (tag, name, int((a != b).sum()), a.numel())


# ---- 1. exact data, bitwise ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("A", AS)
def test_posterior_on_exact_data_is_the_rule_bitwise(exact_models, A, T):
    m, p = exact_models(A)
    feat, action, noise = C.exact_inputs(33, T, A)
    ref = C.posterior(p, feat, action, noise, torch.float64)           # once, at B = 33: a row does not depend on B
    unrounded = _posterior(m, "fp32", feat.cuda(), action.cuda(), noise.cuda())
    for B in BS:
        got = _posterior(m, "bf16", feat[:B].cuda(), action[:B].cuda(), noise[:B].cuda())
        _check_exact("A %d T %d B %2d" % (A, T, B), got, [t[:B] for t in ref])
    differ = float((got[3] != unrounded[3]).float().mean())
    print("A %d T %d: %.1f %% of z2 differs from the fp32 chain" % (A, T, 100 * differ))
    assert differ > 0.9                                                # real rounding is exercised


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("A", AS)
def test_predict_on_exact_data_is_the_rule_bitwise(exact_models, A, H):
    m, p = exact_models(A)
    g = torch.Generator().manual_seed(31 + 10 * H + A)
    z0 = torch.randint(0, 512, (33, Z), generator=g).float() / 256
    actions = torch.randint(0, 8, (33, H, A), generator=g).float() / 4
    noise = torch.zeros(33, H, Z)
    ref = C.prior(p, z0, actions, noise, torch.float64)
    for B in BS:
        got = _predict(m, "bf16", z0[:B].cuda(), actions[:B].cuda(), noise[:B].cuda())
        _check_exact("A %d H %d B %2d" % (A, H, B), got, [t[:B] for t in ref])


# ---- 2. random data, teacher-forced ----------------------------------------------------------------------------------------------------------
def _hoisted(m, feat, action):
    from s2p_amd.slac import _PosteriorFn
    B, T, _ = feat.shape
    _, _, ra, rb = _PosteriorFn._hoisted(feat, action, m.z1_posterior.packed(), m.z2_prior.packed())
    return ra.view(T - 1, B, 256).cpu(), rb.view(T - 1, B, 256).cpu()


def test_posterior_teacher_forced_on_random_data(models, capsys):
    A, B, T = 6, 33, 3
    m, p = models(A), R.make_params(A)
    loose, devs = 0.0, []
    for seed in (0, 1, 2):
        feat, action, noise = C.random_inputs(B, T, A, seed)
        mean, std, z1, z2 = _posterior(m, "bf16", feat.cuda(), action.cuda(), noise.cuda())
        z = torch.cat([z1, z2], -1).cpu()
        ra, rb = _hoisted(m, feat.cuda(), action.cuda())               # the fp32 terms the kernel was given
        ref = C.posterior(p, feat, action, noise, torch.float64, ra=ra, rb=rb, z_given=z)
        for gen in (None, torch.Generator().manual_seed(9 + seed)):
            own = C.posterior(p, feat, action, noise, torch.float32, gen=gen, ra=ra, rb=rb, z_given=z)
            loose = max(loose, float(C.row_deviation(own, ref).max()))
        devs.append(C.row_deviation((mean.cpu(), std.cpu(), z), ref))
    dev = torch.cat(devs)
    miss = int((dev > TIGHT).sum())
    clean = float(dev[dev <= TIGHT].max())
    with capsys.disabled():
        print("\nteacher-forced: %d (row, MLP) pairs, %d (%.2f %%) not tight, worst %.3e, worst tight %.3e; loose bound 4 x %.3e = %.3e"
              % (dev.numel(), miss, 100.0 * miss / dev.numel(), float(dev.max()), clean, loose, K_TOL * loose))
    assert dev.numel() == 594
    assert float(dev.max()) <= K_TOL * loose
    assert miss <= CAP * dev.numel()


# ---- 3. rows, determinism ------------------------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_their_tile_and_calls_repeat(models):
    A, T = 6, 9
    m = models(A)
    feat, action, noise = [t.cuda() for t in C.random_inputs(33, T, A)]
    full = _posterior(m, "bf16", feat, action, noise)
    again = _posterior(m, "bf16", feat, action, noise)
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    for row in (0, 32):                                      # the first row of the first tile, the only row of the last one
        alone = _posterior(m, "bf16", feat[row:row + 1], action[row:row + 1], noise[row:row + 1])
        for name, a, b in zip(NAMES, alone, full):
            assert torch.equal(a[0], b[row]), (row, name)
    bad = 16                                                 # the first row of the second tile; rows 17..31 share its tile
    feat_nan = feat.clone()
    feat_nan[bad] = float("nan")
    got = _posterior(m, "bf16", feat_nan, action, noise)
    others = [r for r in range(33) if r != bad]
    for name, a, b in zip(NAMES, got, full):
        assert bool(torch.isnan(a[bad]).all()), name
        assert torch.equal(a[others], b[others]), name
    z0, H = torch.cat(full[2:], -1)[:, 0].contiguous(), 8
    pa = [z0, action, noise[:, :H].contiguous()]
    pfull, pagain = _predict(m, "bf16", *pa), _predict(m, "bf16", *pa)
    assert all(torch.equal(a, b) for a, b in zip(pfull, pagain))
    for row in (0, 32):
        alone = _predict(m, "bf16", *[t[row:row + 1] for t in pa])
        assert all(torch.equal(a[0], b[row]) for a, b in zip(alone, pfull)), row


# ---- 4. nothing else is written ------------------------------------------------------------------------------------------------------------
def _v3(t, B, T):
    return t.as_strided((B, T, t.shape[1]), (T * t.stride(0), t.stride(0), 1))


def _snapshot(packs):
    return [t.clone() for pk in packs for t in (pk["w1"], pk["b1"], pk["w2"], pk["b2"], pk["w3"], pk["b3"])]


@pytest.mark.parametrize("layout", ["aligned", "odd"])
def test_only_the_three_outputs_are_written(models, layout):
    """aligned: pitches and offsets that are multiples of 4 floats (the kernel's 16-byte loads of eps and stores of mean, std, z);
    odd: neither (its 4-byte ones)."""
    from s2p_amd import ops
    A, B, T = 6, 17, 9
    m = models(A)
    feat, action, noise = [t.cuda() for t in C.random_inputs(B, T, A)]
    want = _posterior(m, "bf16", feat, action, noise)
    ra, rb = [t.cuda().view((T - 1) * B, 256).contiguous() for t in _hoisted(m, feat, action)]
    odd = layout == "odd"
    regions = lambda n: (Region(B * n, Z, pitch=Z + 12 + odd, off=8 - odd, fill=noise[:, :n].reshape(B * n, Z)),
                         Region(B * n, Z1, pitch=40 + odd, off=4 - odd), Region(B * n, Z1, pitch=36 + odd, off=odd),
                         Region(B * n, Z, pitch=320 + odd, off=16 - 3 * odd))
    # the posterior chain
    eps, mean, std, z = regions(T)
    packs = [g.packed_bf16() for g in (m.z1_posterior_init, m.z2_prior_init, m.z1_posterior, m.z2_prior)]
    before = [feat.clone(), ra.clone(), rb.clone(), eps.buf.clone()] + _snapshot(packs) + [q.detach().clone() for q in m._chain_params()]
    ops.posterior_chain_fwd_bf16(feat[:, 0], ra, rb, _v3(eps.v, B, T), [ops.chain_mlp_bf16(pk) for pk in packs], _v3(mean.v, B, T),
                                 _v3(std.v, B, T), _v3(z.v, B, T))
    after = [feat, ra, rb, eps.buf] + _snapshot(packs) + [q.detach() for q in m._chain_params()]
    got = [mean.bits("mean").view(B, T, Z1), std.bits("std").view(B, T, Z1), z.bits("z").view(B, T, Z)]
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert torch.equal(got[0], want[0].cpu()) and torch.equal(got[1], want[1].cpu())
    assert torch.equal(got[2][..., :Z1], want[2].cpu()) and torch.equal(got[2][..., Z1:], want[3].cpu())
    # the prior chain: z2(0) read in place from a [B, 288] z(0)
    H = T - 1
    z0 = torch.cat(want[2:], -1)[:, 0].contiguous()
    pwant = _predict(m, "bf16", z0, action, noise[:, :H].contiguous())
    from s2p_amd.slac import _action_term
    rc, rb2 = _action_term(action, m.z1_prior.packed_cols(Z2, Z2 + A))[1], _action_term(action, m.z2_prior.packed()["g1"][1][0])[1]
    eps, mean, std, z = regions(H)
    packs = [m.z1_prior.packed_bf16(k1=Z2), m.z2_prior.packed_bf16()]
    before = [z0.clone(), rc.clone(), rb2.clone(), eps.buf.clone()] + _snapshot(packs)
    ops.prior_chain_fwd_bf16(z0[:, Z1:], rc, rb2, _v3(eps.v, B, H), [ops.chain_mlp_bf16(pk) for pk in packs], _v3(mean.v, B, H),
                             _v3(std.v, B, H), _v3(z.v, B, H))
    got = [mean.bits("mean").view(B, H, Z1), std.bits("std").view(B, H, Z1), z.bits("z").view(B, H, Z)]
    assert all(torch.equal(a, b) for a, b in zip(before, [z0, rc, rb2, eps.buf] + _snapshot(packs)))
    assert torch.equal(got[0], pwant[0].cpu()) and torch.equal(got[1], pwant[1].cpu())
    assert torch.equal(got[2][..., :Z1], pwant[2].cpu()) and torch.equal(got[2][..., Z1:], pwant[3].cpu())


# ---- 5. the switch ---------------------------------------------------------------------------------------------------------------------------
def test_the_mode_acts_only_in_the_fused_no_grad_chains(models):
    A, B, T = 6, 17, 9
    m = models(A)
    feat, action, noise = [t.cuda() for t in C.random_inputs(B, T, A)]
    calls = {}
    per_layer = _posterior(m, "fp32", feat, action, noise, fused=False)
    for compute in ("fp32", "bf16"):
        calls[compute] = count_calls(lambda: calls.__setitem__("out_" + compute, _posterior(m, compute, feat, action, noise)))
    print("library calls, fp32:", calls["fp32"], " bf16:", calls["bf16"])
    # a bf16-mode sample_posterior: 3 library calls, one of them the _bf16 entry
    assert calls["bf16"] == {"s2p_linear_fwd": 2, POST: 1}
    # default and "fp32": bitwise today's results, and no _bf16 entry is named
    assert calls["fp32"] == {"s2p_linear_fwd": 2, "s2p_posterior_chain_fwd": 1}
    assert all(torch.equal(a, b) for a, b in zip(calls["out_fp32"], per_layer))
    m.fused_chain = True
    try:
        with torch.no_grad():
            default = [t.clone() for t in m.sample_posterior(feat, action, noise)]
    finally:
        m.fused_chain = False
    assert m.chain_compute == "fp32" and all(torch.equal(a, b) for a, b in zip(default, per_layer))
    assert not any(torch.equal(a, b) for a, b in zip(calls["out_bf16"], per_layer))
    # the per-layer path does not read the attribute
    assert all(torch.equal(a, b) for a, b in zip(_posterior(m, "bf16", feat, action, noise, fused=False), per_layer))
    # predict
    z0, H = torch.cat(per_layer[2:], -1)[:, 0].contiguous(), T - 1
    pcalls = {c: count_calls(lambda: calls.__setitem__("p_" + c, _predict(m, c, z0, action, noise[:, :H].contiguous()))) for c in ("fp32", "bf16")}
    assert pcalls["bf16"] == {"s2p_linear_fwd": 2, PRIOR: 1} and pcalls["fp32"] == {"s2p_linear_fwd": 2, "s2p_prior_chain_fwd": 1}
    assert all(torch.equal(a, b) for a, b in zip(calls["p_fp32"], _predict(m, "fp32", z0, action, noise[:, :H].contiguous(), fused=False)))
    assert not torch.equal(calls["p_bf16"][3], calls["p_fp32"][3])
    # an unknown mode raises where it is read
    with pytest.raises(ValueError, match="chain_compute"):
        _posterior(m, "fp16", feat, action, noise)
    with pytest.raises(ValueError, match="chain_compute"):
        _predict(m, "fp16", z0, action, noise[:, :H].contiguous())


def test_grad_mode_and_imagine_ignore_the_mode(models):
    from s2p_amd.iql import TanhGaussianPolicy
    A, B, T = 6, 5, 3
    m = models(A)
    feat, action, noise = [t.cuda() for t in C.random_inputs(B, T, A)]
    outs, grads, calls = {}, {}, {}
    heads = [k for k, _ in m.named_parameters() if k.startswith(("z1_posterior", "z2_prior"))]
    try:
        for compute in ("fp32", "bf16"):
            m.fused_chain, m.chain_compute = True, compute
            m.zero_grad(set_to_none=True)

            def step():
                out = m.sample_posterior(feat, action, noise)
                assert out[3].grad_fn is not None and m.chain_state_bytes > 0
                sum(t.sum() for t in out).backward()
                outs[compute] = [t.detach().clone() for t in out]
            calls[compute] = count_calls(step)
            named = dict(m.named_parameters())
            grads[compute] = {k: named[k].grad.clone() for k in heads}
    finally:
        m.fused_chain, m.chain_compute = False, "fp32"
        m.zero_grad(set_to_none=True)
    assert calls["bf16"] == calls["fp32"] and not any(k.endswith("_bf16") for k in calls["bf16"])
    assert all(torch.equal(a, b) for a, b in zip(outs["bf16"], outs["fp32"]))
    assert all(torch.equal(grads["bf16"][k], grads["fp32"][k]) and float(grads["fp32"][k].abs().max()) > 0 for k in heads)
    # imagine stays fp32 whatever the attribute says
    po = TanhGaussianPolicy(hidden_sizes=[128, 128], obs_dim=Z, action_dim=A).load_state_dict(IM.make_policy_params(128, A))
    z0, eps = torch.cat(outs["fp32"][2:], -1)[:, 0].contiguous(), noise[:, :2].contiguous()
    im = {c: count_calls(lambda: outs.__setitem__("im_" + c, _run(m, c, lambda: m.imagine(po, z0, 2, eps)))) for c in ("fp32", "bf16")}
    assert im["bf16"] == im["fp32"] and im["bf16"].get("s2p_imagine_chain_fwd") == 1
    assert all(torch.equal(a, b) for a, b in zip(outs["im_bf16"], outs["im_fp32"]))


def test_the_bf16_pack_follows_the_parameters(hip_device):
    from s2p_amd.slac import Gaussian
    g = Gaussian(Z2 + 6, Z1).to(hip_device)
    pz = g.packed_bf16(k1=Z2)
    assert g.packed_bf16(k1=Z2) is pz                                              # not re-made while no parameter changed
    w1, w2, w3 = (g.net._modules[i].weight.detach() for i in ("0", "2", "4"))
    assert pz["w1"].dtype == torch.bfloat16 and pz["w1"].shape == (256, Z2) and pz["w1"].is_contiguous()
    assert torch.equal(pz["w1"], w1[:, :Z2].to(torch.bfloat16)) and torch.equal(pz["w2"], w2.to(torch.bfloat16))
    assert torch.equal(pz["w3"], w3.to(torch.bfloat16)) and pz["w3"].shape == (2 * Z1, 256)
    assert pz["b1"] is g.packed()["b1"] and pz["b3"].dtype == torch.float32
    with pytest.raises(ValueError):
        g.packed_bf16()                                                            # all 262 columns: not a multiple of 8
    with torch.no_grad():
        g.net._modules["2"].weight.mul_(1.5)                                       # an in-place update, as an optimizer step is
    new = g.packed_bf16(k1=Z2)
    assert new is not pz and torch.equal(new["w2"], g.net._modules["2"].weight.detach().to(torch.bfloat16))
    assert not torch.equal(new["w2"], pz["w2"]) and g.packed_bf16(k1=Z2) is new


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------------------------
def test_three_iql_steps_on_cached_features(hip_device, capsys):
    """Recorded, not asserted beyond finiteness: the losses of three frozen-SLAC IQL steps on a FeatureBatch in both modes."""
    from s2p_amd.iql import CriticSLAC, IQLTrainer, Qfunction, TanhGaussianPolicy, Vfunction
    from s2p_amd.slac_algo import SlacAlgorithm
    from s2p_amd.slac_buffer import FeatureBatch
    S, A = SB.S, SB.A
    PIN = S * FEAT + (S - 1) * A
    idxes = np.array([0, 3, 7, 8, 3])
    sd = IR.init_params(Z, A, 64, PIN, seed=5, last_scale=30.0)
    losses, calls = {}, {}
    algo = SlacAlgorithm((3, 100, 100), (A,), 1, hip_device, seed=0, batch_size_latent=2, buffer_size=32, num_sequences=S,
                         frame_capacity=128, fused_chain=True, chain_compute="bf16")
    assert algo.latent.chain_compute == "bf16" and algo.latent.fused_chain is True
    algo.latent.load_state_dict(R.full_state_dict(R.make_params(A)), strict=True)
    algo.load_data_in_buffer(SB.real_dataset(2, 12, 100, 100), **dict(SB.LOAD_ARGS["real"], data_num=24))
    algo.cache_features()
    for compute in ("fp32", "bf16"):
        algo.latent.chain_compute = compute
        q = [Qfunction(hidden_sizes=[64, 64], output_size=1, input_size=Z + A) for _ in range(4)]
        critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=[64, 64], output_size=1, input_size=Z), device=hip_device)
        policy = TanhGaussianPolicy(hidden_sizes=[64, 64], obs_dim=PIN, action_dim=A, device=hip_device)
        critic.load_state_dict(sd[0], strict=True)
        policy.load_state_dict(sd[1], strict=True)
        tr = IQLTrainer(None, policy, critic=critic, slac_algo=algo, freeze_slac=True, discount=0.99, policy_lr=1e-4, qf_lr=3e-4,
                        reward_scale=1, soft_target_tau=0.005, beta=0.1, quantile=0.7, clip_score=100, target_update_period=2)
        torch.manual_seed(123)
        rows = []

        def steps():
            for _ in range(3):
                batch = algo.buffer.random_batch(len(idxes), idxes=idxes, frames="features")
                assert isinstance(batch["observations"], FeatureBatch)
                rows.append(tr.train_from_torch(batch).cpu().clone())
        calls[compute] = count_calls(steps)
        losses[compute] = torch.stack(rows)
    with capsys.disabled():
        for compute in ("fp32", "bf16"):
            print("\n%s chain, IQL losses of steps 0..2:" % compute, [[round(float(v), 6) for v in r] for r in losses[compute]])
    assert calls["bf16"].get(POST) == 3 and POST not in calls["fp32"] and calls["fp32"].get("s2p_posterior_chain_fwd") == 3
    assert bool(torch.isfinite(losses["bf16"]).all()) and bool(torch.isfinite(losses["fp32"]).all())
