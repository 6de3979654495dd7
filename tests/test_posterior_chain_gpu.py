"""N3h -- the fused no-grad posterior chain (csrc/gauss_chain.hip, `LatentModel.fused_chain`) against the per-layer path it replaces.

The acceptance is BITWISE: both paths run the same MFMA sequence per output element and the same epilogues, so every comparison with
the unfused path is torch.equal, at the smallest shapes that reach every code path (a partial 16-row tile, exactly one tile, one row
more, three workgroups; T = 1 without a chain, one chain step, the workload's nine; action widths 6 and 1 for the padded K of the
hoisted groups).  The one toleranced check is against the recorded reference (tests/golden/slac_latent_golden_v1.npz) under the
project's rule: err <= K_TOL x max(ref32_err, 1e-6), K_TOL = 4, where ref32_err is the deviation of the reference's own fp32 run from
its fp64 run."""
import os

import numpy as np
import pytest
import torch

import iql_ref as IR
import slac_buffer_ref as SB
import slac_latent_ref as R
from guard_region import Region
from slac_chain_util import count_calls, model_cache

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
K_TOL, FLOOR = 4.0, 1e-6
Z1, Z2, Z, FEAT = 32, 256, 288, 256
BS, TS, AS = (1, 15, 16, 17, 33), (1, 2, 9), (6, 1)
NAME = "s2p_posterior_chain_fwd"
LN2 = 0.6931472


@pytest.fixture(scope="module")
def models(hip_device):
    """action width -> a LatentModel with the seeded weights of tests/slac_latent_ref.py; built once, left with fused_chain False."""
    return model_cache()


def _inputs(B, T, A, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 100 * T + A)
    feat, action, noise = torch.randn(33, T, FEAT, generator=g), torch.randn(33, T - 1, A, generator=g), torch.randn(33, T, Z, generator=g)
    return feat[:B].cuda(), action[:B].cuda(), noise[:B].cuda()          # row b is the same whatever B is


def _posterior(m, fused, feat, action, noise):
    m.fused_chain = fused
    try:
        with torch.no_grad():
            out = m.sample_posterior(feat, action, noise)
        torch.cuda.synchronize()
        assert m.chain_state_bytes == 0 and all(t.grad_fn is None for t in out)
        return [t.clone() for t in out]
    finally:
        m.fused_chain = False


# ---- 1. bitwise against the unfused path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("A", AS)
def test_fused_equals_unfused_bitwise(models, A, T):
    m = models(A)
    for B in BS:
        args = _inputs(B, T, A)
        want, got = _posterior(m, False, *args), _posterior(m, True, *args)
        for name, a, b in zip(("mean", "std", "z1", "z2"), got, want):
            assert a.shape == b.shape == (B, T, Z2 if name == "z2" else Z1)
            assert bool(torch.isfinite(b).all()) and float(b.abs().max()) > 0
            diff = int((a.view(torch.int32) != b.view(torch.int32)).sum())
            print("A %d T %d B %2d %-4s elements that differ: %d of %d" % (A, T, B, name, diff, a.numel()))
            assert torch.equal(a, b), (A, T, B, name, diff)


# ---- 2. row independence -------------------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_their_tile(models):
    A, T = 6, 9
    m = models(A)
    feat, action, noise = _inputs(33, T, A)
    full = _posterior(m, True, feat, action, noise)
    for row in (0, 32):                                      # the first row of the first tile, the only row of the last one
        alone = _posterior(m, True, feat[row:row + 1], action[row:row + 1], noise[row:row + 1])
        for name, a, b in zip(("mean", "std", "z1", "z2"), alone, full):
            assert torch.equal(a[0], b[row]), (row, name)
    bad = 16                                                 # the first row of the second tile; rows 17..31 share its tile
    feat_nan = feat.clone()
    feat_nan[bad] = float("nan")
    got = _posterior(m, True, feat_nan, action, noise)
    others = [r for r in range(33) if r != bad]
    for name, a, b in zip(("mean", "std", "z1", "z2"), got, full):
        assert bool(torch.isnan(a[bad]).all()), name
        assert torch.equal(a[others], b[others]), name


# ---- 3. nothing else is written --------------------------------------------------------------------------------------------------------
def _direct(m, feat, action, eps_view, mean, std, z):
    """The entry point itself on [B*T, C] views with any pitch; -> (ra, rb) it was given."""
    from s2p_amd import ops
    from s2p_amd.slac import _PosteriorFn
    B, T, _ = feat.shape
    packs = [g.packed() for g in (m.z1_posterior_init, m.z2_prior_init, m.z1_posterior, m.z2_prior)]
    ra = rb = None
    if T > 1:
        _, _, ra, rb = _PosteriorFn._hoisted(feat, action, packs[2], packs[3])
    v3 = lambda t: t.view(B, T, t.shape[1]) if t.is_contiguous() else t.as_strided((B, T, t.shape[1]), (T * t.stride(0), t.stride(0), 1))
    ops.posterior_chain_fwd(feat[:, 0], ra, rb, v3(eps_view), [ops.chain_mlp(p) for p in packs], v3(mean), v3(std), v3(z))
    torch.cuda.synchronize()
    return ra, rb


def test_only_the_three_outputs_are_written(models):
    A, B, T = 6, 17, 9
    m = models(A)
    feat, action, noise = _inputs(B, T, A)
    want = _posterior(m, False, feat, action, noise)
    eps = Region(B * T, Z, pitch=Z + 12, off=8, fill=noise.reshape(B * T, Z))
    mean, std = Region(B * T, Z1, pitch=40, off=4), Region(B * T, Z1, pitch=36, off=0)
    z = Region(B * T, Z, pitch=320, off=16)                  # a slice of a wider buffer
    from s2p_amd.slac import _PosteriorFn
    packs = [g.packed() for g in (m.z1_posterior, m.z2_prior)]
    ra0, rb0 = _PosteriorFn._hoisted(feat, action, *packs)[2:]
    feat0, eps0 = feat.clone(), eps.buf.clone()
    weights0 = [p.detach().clone() for p in m._chain_params()]
    ra, rb = _direct(m, feat, action, eps.v, mean.v, std.v, z.v)
    assert torch.equal(ra, ra0) and torch.equal(rb, rb0) and torch.equal(feat, feat0) and torch.equal(eps.buf, eps0)
    assert all(torch.equal(p.detach(), w) for p, w in zip(m._chain_params(), weights0))
    got = [mean.bits("mean"), std.bits("std"), z.bits("z")]
    assert torch.equal(got[0].view(B, T, Z1), want[0].cpu()) and torch.equal(got[1].view(B, T, Z1), want[1].cpu())
    assert torch.equal(got[2].view(B, T, Z)[..., :Z1], want[2].cpu()) and torch.equal(got[2].view(B, T, Z)[..., Z1:], want[3].cpu())


# ---- 4. both softplus branches -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,D", [(("z1_posterior_init", "z1_posterior"), Z1), (("z2_prior_init", "z2_prior"), Z2)])
@pytest.mark.parametrize("bias", [30.0, -30.0])
def test_both_softplus_branches(hip_device, bias, heads, D):
    """raw_std = +-30 + O(1): softplus is r + log1p(exp(-r)) on one side and log1p(exp(r)) ~ 1e-13 on the other, where std is the
    1e-5 floor.  The z1 heads' std is an output; the z2 heads' std shows in z2 = mean + eps * std, so eps = 1 against eps = 0.
    softplus(0) = ln 2 separates the branches: every std of a +30 run is above it, every std of a -30 run below."""
    from s2p_amd.slac import LatentModel
    A, B, T = 6, 17, 2
    m = LatentModel((3, 100, 100), (A,), image_size=100)
    m.load_state_dict(R.full_state_dict(R.make_params(A)), strict=True)
    with torch.no_grad():
        for h in heads:
            getattr(m, h).net._modules["4"].bias[D:] = bias
    feat, action, noise = _inputs(B, T, A, seed=4)
    outs = {}
    for e in (None, 0.0, 1.0):
        eps = noise.clone()
        if e is not None:
            lo, hi = (Z1, Z) if D == Z2 else (0, Z1)
            eps[..., lo:hi] = e
        want = _posterior(m, False, feat, action, eps)          # the composition of the existing entry points
        mean, std, z = (torch.full((B, T, c), float("nan"), device=hip_device) for c in (Z1, Z1, Z))
        _direct(m, feat, action, eps.view(B * T, Z), mean.view(B * T, Z1), std.view(B * T, Z1), z.view(B * T, Z))
        got = [mean, std, z[..., :Z1], z[..., Z1:]]
        for name, a, b in zip(("mean", "std", "z1", "z2"), got, want):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()), (name, e)
        assert float(std.min()) > 0
        outs[e] = got
    if D == Z1:
        sd = outs[None][1]
        print("bias %+.0f: z1 std in [%.6e, %.6e]" % (bias, float(sd.min()), float(sd.max())))
        assert (float(sd.min()) > LN2) if bias > 0 else (float(np.float32(1e-5)) <= float(sd.min()) and float(sd.max()) < LN2)
    else:
        step = outs[1.0][3][:, 0] - outs[0.0][3][:, 0]         # t = 0: the same mean in both runs, so this is std up to a rounding
        print("bias %+.0f: z2(eps 1) - z2(eps 0) in [%.6e, %.6e]" % (bias, float(step.min()), float(step.max())))
        assert float(step.min()) > 0 and ((float(step.min()) > LN2) if bias > 0 else float(step.max()) < LN2)


# ---- 5. pinned parity ----------------------------------------------------------------------------------------------------------------------
def test_fused_matches_the_recorded_reference(models, capsys):
    G = np.load(os.path.join(HERE, "golden", "slac_latent_golden_v1.npz"))
    m = models(R.A)
    state_u8, action, _, _, noise = R.make_inputs()
    with torch.no_grad():
        feat = m.encoder((state_u8.double() / 255.0).float())
    worst = {}
    for fused in (False, True):
        out = _posterior(m, fused, feat, action.cuda(), noise.cuda())
        ratios = []
        for k, v in zip(("post_mean", "post_std", "z1", "z2"), out):
            err, ref = R.rel_max(v, G["mid." + k]), max(float(G["mid.%s.ref32_err" % k]), FLOOR)
            ratios.append(err / ref)
            if fused:
                assert err <= K_TOL * ref, (k, err, K_TOL * ref)
        worst[fused] = max(ratios)
    with capsys.disabled():
        print("\nworst deviation / max(ref32_err, 1e-6): unfused %.6f, fused %.6f" % (worst[False], worst[True]))
    assert worst[True] == worst[False]


# ---- 6. grad mode is untouched -------------------------------------------------------------------------------------------------------------
def test_grad_mode_runs_the_per_layer_path(models):
    m = models(R.A)
    state_u8, action, reward, done, noise = R.make_inputs()
    state = (state_u8.double() / 255.0).float()
    heads = [k for k, _ in m.named_parameters() if not k.startswith(("encoder.", "decoder."))]
    assert len(heads) == 36
    grads, calls = {}, {}
    try:
        for fused in (False, True):
            m.fused_chain = fused
            m.zero_grad(set_to_none=True)

            def step():
                z = m.sample_posterior(m.encoder(state), action, noise)[3]
                assert z.grad_fn is not None and m.chain_state_bytes > 0
                sum(m.calculate_loss(state, action, reward, done, noise)).backward()
            calls[fused] = count_calls(step)
            torch.cuda.synchronize()
            named = dict(m.named_parameters())
            grads[fused] = {k: named[k].grad.clone() for k in heads}
    finally:
        m.fused_chain = False
        m.zero_grad(set_to_none=True)
    assert NAME not in calls[True] and calls[True] == calls[False]
    assert all(torch.equal(grads[True][k], grads[False][k]) and float(grads[True][k].abs().max()) > 0 for k in heads)


# ---- 7. launch count -------------------------------------------------------------------------------------------------------------------------
def test_one_chain_call_replaces_the_per_layer_calls(models):
    m = models(6)
    args = _inputs(17, 9, 6)
    unfused, fused = count_calls(lambda: _posterior(m, False, *args)), count_calls(lambda: _posterior(m, True, *args))
    print("library calls, unfused:", unfused, " fused:", fused)
    assert fused.get(NAME) == 1 and NAME not in unfused
    assert "s2p_linear_add_fwd" not in fused and "s2p_gauss_head_fwd" not in fused and fused.get("s2p_linear_fwd", 0) <= 2
    assert unfused["s2p_linear_add_fwd"] == 16 and unfused["s2p_gauss_head_fwd"] == 18 and unfused["s2p_linear_fwd"] == 2 + 6 + 32
    assert set(fused) <= {NAME, "s2p_linear_fwd"}


# ---- 8. consumers ----------------------------------------------------------------------------------------------------------------------------
S, A8 = SB.S, SB.A
P = S * FEAT + (S - 1) * A8
IDXES = np.array([0, 3, 7, 8, 3])


@pytest.fixture(scope="module")
def algo(hip_device):
    """A SlacAlgorithm on 9 windows / 25 frames of the small real dataset (as tests/test_feature_cache_gpu.py builds it)."""
    from s2p_amd.slac_algo import SlacAlgorithm
    a = SlacAlgorithm((3, 100, 100), (A8,), 1, hip_device, seed=0, batch_size_latent=2, buffer_size=32, num_sequences=S, frame_capacity=128)
    assert a.latent.fused_chain is False
    a.latent.load_state_dict(R.full_state_dict(R.make_params(A8)), strict=True)
    a.load_data_in_buffer(SB.real_dataset(2, 12, 100, 100), **dict(SB.LOAD_ARGS["real"], data_num=24))
    a.cache_features()
    return a


def _fused(algo, on):
    algo.latent.fused_chain = on


@pytest.mark.parametrize("form", ["packed", "features"])
def test_prepare_batch_and_an_iql_step(hip_device, algo, form):
    from s2p_amd.iql import CriticSLAC, IQLTrainer, Qfunction, TanhGaussianPolicy, Vfunction
    from s2p_amd.slac_buffer import FeatureBatch, FrameBatch
    buf = algo.buffer
    noise = torch.randn(len(IDXES), S + 1, Z, generator=torch.Generator().manual_seed(41)).to(hip_device)
    sd = IR.init_params(Z, A8, 64, P, seed=5, last_scale=30.0)
    outs, losses, calls = {}, {}, {}
    try:
        for on in (False, True):
            _fused(algo, on)
            batch = buf.random_batch(len(IDXES), idxes=IDXES, frames=form)
            assert isinstance(batch["observations"], FeatureBatch if form == "features" else FrameBatch)
            calls[on] = count_calls(lambda: outs.__setitem__(on, [t.clone() for t in algo.prepare_batch(batch["observations"], batch["actions"], noise)]))
            q = [Qfunction(hidden_sizes=[64, 64], output_size=1, input_size=Z + A8) for _ in range(4)]
            critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=[64, 64], output_size=1, input_size=Z), device=hip_device)
            policy = TanhGaussianPolicy(hidden_sizes=[64, 64], obs_dim=P, action_dim=A8, device=hip_device)
            critic.load_state_dict(sd[0], strict=True)
            policy.load_state_dict(sd[1], strict=True)
            tr = IQLTrainer(None, policy, critic=critic, slac_algo=algo, freeze_slac=True, discount=0.99, policy_lr=1e-4, qf_lr=3e-4,
                            reward_scale=1, soft_target_tau=0.005, beta=0.1, quantile=0.7, clip_score=100, target_update_period=2)
            torch.manual_seed(123)
            losses[on] = tr.train_from_torch(buf.random_batch(len(IDXES), idxes=IDXES, frames=form)).cpu().clone()
    finally:
        _fused(algo, False)
    assert calls[True].get(NAME) == 1 and NAME not in calls[False]
    assert len(outs[True]) == 5 and all(torch.equal(a, b) for a, b in zip(outs[True], outs[False]))
    print(form, "IQL step-0 losses:", losses[True].tolist())
    assert bool(torch.isfinite(losses[True]).all()) and torch.equal(losses[True], losses[False])


def test_latent_z_actor_on_a_replayed_environment(hip_device, algo):
    from s2p_amd.actor import ReplayEnv, SlacActor
    from s2p_amd.iql import TanhGaussianPolicy
    data = SB.real_dataset(2, 12, 100, 100)
    sd = IR.init_params(Z, A8, 64, Z, seed=5, last_scale=30.0)
    acts, calls = {}, {}
    try:
        for on in (False, True):
            _fused(algo, on)
            policy = TanhGaussianPolicy(hidden_sizes=[64, 64], obs_dim=Z, action_dim=A8, device=hip_device)
            policy.load_state_dict(sd[1], strict=True)
            envs = [ReplayEnv(data, k) for k in range(2)]
            actor = SlacActor(policy, algo, len(envs), "latent_z")

            def run():
                actor.reset(np.stack([e.reset() for e in envs]))
                out = []
                for t in range(3):
                    a = actor.act(torch.randn(len(envs), S, Z, generator=torch.Generator().manual_seed(70 + t)))
                    out.append(a.copy())
                    actor.observe(np.stack([e.step(a[k])[0] for k, e in enumerate(envs)]), a)
                acts[on] = np.stack(out)
            calls[on] = count_calls(run)
    finally:
        _fused(algo, False)
    assert calls[True].get(NAME) == 3 and NAME not in calls[False]
    assert acts[True].shape == (3, 2, A8) and np.isfinite(acts[True]).all() and np.abs(acts[True]).max() > 0
    assert np.array_equal(acts[True].view(np.int32), acts[False].view(np.int32))
