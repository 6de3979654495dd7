"""N3j -- closed-loop imagination in the SLAC latent model: `LatentModel.imagine` on its per-layer path (13 library calls per step)
and as one launch (csrc/gauss_chain.hip: s2p_imagine_chain_fwd, `LatentModel.fused_chain`), `CriticSLAC.q_min`,
`slac_imagine.imagined_returns` / `behaviour`, imagine_policy.py.

The acceptance between the two paths is BITWISE (torch.equal): both run the same MFMA sequence per output element, the same
epilogues and the same tanh, at the smallest shapes that reach every code path (a partial 16-row tile, exactly one tile, one row
more, three workgroups; one step, one loop turn, five; action widths 6 and 1 for both paddings of the action chunk; policy widths
128 and 256 -- one and two passes over the column tiles -- and 1024, the full LDS map).  The toleranced checks against the recorded
run of the reference's modules (tests/golden/slac_imagine_golden_v1.npz) use the project's rule per step:
err(h) <= K_TOL x max(ref32_err(h), 1e-6), K_TOL = 4, ref32_err the deviation of the reference's own fp32 run from its fp64 run."""
import os

import numpy as np
import pytest
import torch

import slac_buffer_ref as SB
import slac_imagine_ref as IR
import slac_latent_ref as R
from guard_region import Region
from slac_chain_util import build_model, count_calls, model_cache

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
K_TOL, FLOOR = 4.0, 1e-6
Z1, Z2, Z = 32, 256, 288
BS, HS, AS, WS = (1, 15, 16, 17, 33), (1, 2, 5), (6, 1), (128, 256)
NAME = "s2p_imagine_chain_fwd"
OUT = ("actions", "mean", "std", "z")


def _make_policy(W, A, sd=None):
    from s2p_amd.offline_rl import TanhGaussianPolicy
    hid = list(W) if isinstance(W, (tuple, list)) else [W, W]
    return TanhGaussianPolicy(hidden_sizes=hid, obs_dim=Z, action_dim=A).load_state_dict(sd if sd is not None else IR.make_policy_params(W, A))


@pytest.fixture(scope="module")
def models(hip_device):
    """action width -> a LatentModel with the seeded weights of tests/slac_latent_ref.py; built once, left with fused_chain False."""
    return model_cache()


@pytest.fixture(scope="module")
def policies(hip_device):
    """(width, action width) -> a TanhGaussianPolicy with the seeded weights of tests/slac_imagine_ref.py."""
    cache = {}

    def get(W, A):
        if (W, A) not in cache:
            cache[W, A] = _make_policy(W, A)
        return cache[W, A]
    return get


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "slac_imagine_golden_v1.npz"))


def _inputs(B, H):
    return [t.cuda() for t in IR.make_inputs(B, H)]                    # row b, step k are the same whatever B and H are


def _imagine(m, po, fused, z0, noise=None, sample=True, H=None):
    m.fused_chain = fused
    try:
        with torch.enable_grad():                                      # imagine itself must switch grad off
            out = m.imagine(po, z0, noise.shape[1] if H is None else H, noise, sample)
        torch.cuda.synchronize()
        assert all(t.grad_fn is None and not t.requires_grad for t in out)
        return [t.clone() for t in out]
    finally:
        m.fused_chain = False


def _predict(m, fused, z0, actions, noise):
    m.fused_chain = fused
    try:
        out = m.predict(z0, actions, noise)
        torch.cuda.synchronize()
        return [t.clone() for t in out]
    finally:
        m.fused_chain = False


def _widths(A):
    return dict(zip(OUT, (A, Z1, Z1, Z)))


# ---- 1. bitwise against the per-layer path -------------------------------------------------------------------------------------------
def _bitwise(m, po, B, H, A, tag):
    z0, noise = _inputs(B, H)
    want, got = _imagine(m, po, False, z0, noise), _imagine(m, po, True, z0, noise)
    for name, a, b in zip(OUT, got, want):
        assert a.shape == b.shape == (B, H, _widths(A)[name])
        assert bool(torch.isfinite(b).all()) and float(b.abs().max()) > 0
        diff = int((a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).sum())
        print("%s B %2d H %d %-7s elements that differ: %d of %d" % (tag, B, H, name, diff, a.numel()))
        assert torch.equal(a, b), (tag, B, H, name, diff)
    assert float(want[0].abs().max()) <= 1.0


@pytest.mark.parametrize("W", WS)
@pytest.mark.parametrize("A", AS)
def test_fused_equals_per_layer_bitwise(models, policies, A, W):
    m, po = models(A), policies(W, A)
    for H in HS:
        for B in BS:
            _bitwise(m, po, B, H, A, "A %d W %d" % (A, W))


def test_fused_equals_per_layer_bitwise_at_the_full_lds_map(models, policies):
    _bitwise(models(6), policies(1024, 6), 17, 2, 6, "A 6 W 1024")


def test_policy_shapes_noise_and_errors(models, policies, golden):
    from s2p_amd.offline_rl import TanhGaussianPolicy
    m, po = models(6), policies(256, 6)
    z0, noise = _inputs(17, 5)
    for fused in (False, True):
        zero = _imagine(m, po, fused, z0, torch.zeros_like(noise))
        mean = _imagine(m, po, fused, z0, noise, sample=False)               # the noise argument is not used
        none = _imagine(m, po, fused, z0, None, sample=False, H=5)
        assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(mean, zero, none))
        assert torch.equal(mean[3][:, 0, :Z1], mean[1][:, 0])                # z1 = its mean when eps = 0
        torch.manual_seed(5)
        d1 = _imagine(m, po, fused, z0, None, H=5)
        torch.manual_seed(5)
        d2 = _imagine(m, po, fused, z0, None, H=5)
        assert all(torch.equal(a, b) for a, b in zip(d1, d2)) and not torch.equal(d1[3], mean[3])
        empty = _imagine(m, po, fused, z0, None, H=0)
        assert [tuple(t.shape) for t in empty] == [(17, 0, 6), (17, 0, Z1), (17, 0, Z1), (17, 0, Z)]
    # a policy outside the built shapes: a ValueError naming them on the fused path, any two-hidden-layer width per layer
    odd = _make_policy((160, 96), 6, {**IR.make_policy_params(160, 6), **_odd_tail(160, 96, 6)})
    act, mean, std, z = _imagine(m, odd, False, z0, noise)
    ref = max(float(max(golden["%s.actions.ref32_err" % r][0] for r in IR.ROLLOUTS)), FLOOR)
    assert R.rel_max(act[:, 0], odd.act(z0)) <= K_TOL * ref and float(act.abs().max()) > 0.5
    assert all(torch.equal(a, b) for a, b in zip(_predict(m, True, z0, act, noise), (mean, std, z)))
    for bad in (odd, _make_policy(192, 6)):
        with pytest.raises(ValueError, match="128"):
            _imagine(m, bad, True, z0, noise)
    with pytest.raises(ValueError):
        m.imagine(TanhGaussianPolicy(hidden_sizes=[128, 128], obs_dim=256, action_dim=6), z0, 2)          # not a latent_z policy
    with pytest.raises(ValueError):
        m.imagine(policies(128, 1), z0, 2)                                                                # another action width
    with pytest.raises(ValueError):
        m.imagine(TanhGaussianPolicy(hidden_sizes=[128, 128, 128], obs_dim=Z, action_dim=6), z0, 2)
    with pytest.raises(ValueError):
        m.imagine(po, z0[:, :Z2], 2)
    with pytest.raises(ValueError):
        m.imagine(po, z0, 5, noise[:, :4])
    with pytest.raises(ValueError):
        m.imagine(po, z0, -1)


def _odd_tail(w0, w1, a):
    g = torch.Generator().manual_seed(17)
    return {"fc1.weight": (torch.rand(w1, w0, generator=g) * 2 - 1) / w0 ** 0.5, "fc1.bias": torch.randn(w1, generator=g) * 0.05,
            "last_fc.weight": (torch.rand(a, w1, generator=g) * 2 - 1) * 7.0 / w1 ** 0.5,
            "last_fc_log_std.weight": (torch.rand(a, w1, generator=g) * 2 - 1) * 1e-3}


# ---- 2. closed loop == open loop under the same actions ---------------------------------------------------------------------------
@pytest.mark.parametrize("A", AS)
def test_predict_under_the_imagined_actions_is_bitwise_the_rollout(models, policies, A):
    m, po = models(A), policies(256, A)
    z0, noise = _inputs(17, 5)
    for fused in (False, True):
        act, mean, std, z = _imagine(m, po, fused, z0, noise)
        for pf in (False, True):
            got = _predict(m, pf, z0, act, noise)
            for name, a, b in zip(OUT[1:], got, (mean, std, z)):
                assert torch.equal(a, b), (A, fused, pf, name)


# ---- 3. the first action is the policy's ---------------------------------------------------------------------------------------------
def test_first_action_is_the_policys(models, policies, golden):
    """policy.act runs the grouped MLP kernels of csrc/mlp.hip, not s2p_linear_fwd: within the rule, not bitwise."""
    m, po = models(6), policies(256, 6)
    z0, noise = _inputs(33, 1)
    want = po.act(z0)
    ref = max(float(max(golden["%s.actions.ref32_err" % r][0] for r in IR.ROLLOUTS)), FLOOR)
    for fused in (False, True):
        a0 = _imagine(m, po, fused, z0, noise)[0][:, 0]
        err = R.rel_max(a0, want)
        print("fused %d: a(0) deviates from policy.act(z0) by %.3e (%.3f of max(ref32_err, 1e-6))" % (fused, err, err / ref))
        assert err <= K_TOL * ref, err
    assert float(want.abs().max()) > 0.5


# ---- 4. Markov restart ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
def test_markov_restart(models, policies, fused):
    m, po = models(6), policies(256, 6)
    z0, noise = _inputs(17, 5)
    full = _imagine(m, po, fused, z0, noise)
    tail = _imagine(m, po, fused, full[3][:, 2], noise[:, 3:])
    for name, a, b in zip(OUT, tail, full):
        assert a.shape[1] == 2 and torch.equal(a, b[:, 3:]), name
    other = z0.clone()
    other[:, :Z1] += 1.0                                                     # z1(0) IS an input here: the policy reads it
    assert not torch.equal(_imagine(m, po, fused, other, noise)[0][:, 0], full[0][:, 0])


# ---- 5. rows do not meet ---------------------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_their_tile(models, policies):
    m, po = models(6), policies(256, 6)
    z0, noise = _inputs(33, 5)
    full = _imagine(m, po, True, z0, noise)
    for row in (0, 32):                                      # the first row of the first tile, the only row of the last one
        alone = _imagine(m, po, True, z0[row:row + 1], noise[row:row + 1])
        for name, a, b in zip(OUT, alone, full):
            assert torch.equal(a[0], b[row]), (row, name)
    bad = 16                                                 # the first row of the second tile; rows 17..31 share its tile
    z0_nan = z0.clone()
    z0_nan[bad] = float("nan")
    got, per_layer = _imagine(m, po, True, z0_nan, noise), _imagine(m, po, False, z0_nan, noise)
    others = [r for r in range(33) if r != bad]
    for name, a, b, c in zip(OUT, got, full, per_layer):
        # relu(NaN) = 0 (`v > 0 ? v : 0`, as s2p_linear_fwd has it), so the poisoned row's ACTIONS are the policy's answer to a zero
        # hidden layer, finite and the same at every step; its latents are NaN
        assert bool(torch.isfinite(a[bad]).all() and (a[bad] == a[bad][0]).all()) if name == "actions" else bool(torch.isnan(a[bad]).all()), name
        assert torch.equal(a[others], b[others]), name
        assert torch.equal(a.contiguous().view(torch.int32), c.contiguous().view(torch.int32)), name          # NaN bits included


# ---- 6. nothing else is written ----------------------------------------------------------------------------------------------------------
def _direct(m, po, z0, B, H, A, eps, act, mean, std, z):
    """The entry point itself on [B*H, C] views with any pitch."""
    from s2p_amd import ops
    v3 = lambda t: t.as_strided((B, H, t.shape[1]), (H * t.stride(0), t.stride(0), 1))
    p1, p2 = m.z1_prior.packed(), m.z2_prior.packed()
    ops.imagine_chain_fwd(z0, v3(eps), [ops.chain_mlp(p1, k1=Z2), ops.chain_mlp(p2)], m.z1_prior.packed_cols(Z2, Z2 + A), p2["g1"][1][0],
                          A, ops.policy_mlp(po), v3(act), v3(mean), v3(std), v3(z))
    torch.cuda.synchronize()


@pytest.mark.parametrize("A", AS)
def test_only_the_four_outputs_are_written(models, policies, A):
    B, H = 17, 5
    m, po = models(A), policies(256, A)
    z0, noise = _inputs(B, H)
    want = _imagine(m, po, False, z0, noise)
    z0r = Region(B, Z, pitch=300, off=4, fill=z0)            # z0 inside a wider buffer: 16-byte aligned, the pitch a multiple of 4
    eps = Region(B * H, Z, pitch=301, off=7, fill=noise.reshape(B * H, Z))
    act = Region(B * H, A, pitch=11, off=3)                  # exactly A columns are written, not pad4(A)
    mean, std = Region(B * H, Z1, pitch=41, off=5), Region(B * H, Z1, pitch=33, off=0)
    z = Region(B * H, Z, pitch=321, off=17)
    params = m.z1_prior.layer_params() + m.z2_prior.layer_params()
    packs = lambda: [t for g in (m.z1_prior, m.z2_prior) for t in (g.packed()["g1"][0][0], g.packed()["w2"], g.packed()["w3"])] + \
        [m.z1_prior.packed_cols(Z2, Z2 + A), m.z2_prior.packed()["g1"][1][0]]
    z00, eps0, flat0 = z0r.buf.clone(), eps.buf.clone(), po.flat.clone()
    weights0, packs0 = [p.detach().clone() for p in params], [t.clone() for t in packs()]
    _direct(m, po, z0r.v, B, H, A, eps.v, act.v, mean.v, std.v, z.v)
    assert torch.equal(z0r.buf, z00) and torch.equal(eps.buf, eps0) and torch.equal(po.flat, flat0)
    assert all(torch.equal(p.detach(), w) for p, w in zip(params, weights0))
    assert all(torch.equal(a, b) for a, b in zip(packs(), packs0))
    got = [act.bits("actions"), mean.bits("mean"), std.bits("std"), z.bits("z")]
    for name, a, b in zip(OUT, got, want):
        assert torch.equal(a.view(B, H, _widths(A)[name]), b.cpu()), name


# ---- 7. a saturated policy -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [30.0, -30.0])
def test_saturated_actions_are_exactly_one(models, bias):
    A, B, H = 6, 17, 2
    sd = IR.make_policy_params(256, A)
    sd["last_fc.bias"] = torch.full((A,), bias)
    m, po = models(A), _make_policy(256, A, sd)
    z0, noise = _inputs(B, H)
    outs = [_imagine(m, po, fused, z0, noise) for fused in (False, True)]
    for got in outs:
        assert bool((got[0] == (1.0 if bias > 0 else -1.0)).all())
        assert all(bool(torch.isfinite(t).all()) for t in got) and float(got[2].min()) > 0
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ---- 8. pinned parity ------------------------------------------------------------------------------------------------------------------------
def _critic(hip_device):
    from s2p_amd.offline_rl import CriticSLAC, Qfunction, Vfunction
    hid = [IR.W, IR.W]
    q = [Qfunction(hidden_sizes=hid, output_size=1, input_size=Z + IR.A) for _ in range(4)]
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=hid, output_size=1, input_size=Z))
    sd = critic.state_dict()
    for i, names in enumerate((("qf1", "target_qf1"), ("qf2", "target_qf2"))):
        for n in names:
            sd.update({n + "." + k: v for k, v in IR.make_q_params(i).items()})
    return critic.load_state_dict(sd)


def test_pinned_parity(models, policies, golden, hip_device, capsys):
    """Both rollouts with the reward head, the discounted return (fp64 on the device), the critic's bootstrap and the value against the
    recorded fp64 run of the reference's modules, per step with that step's ref32_err.
    Measured on an MI355X (worst deviation over the steps / max(ref32_err, 1e-6) over all 18 quantities; the bound is K_TOL = 4):
    1.722642 on both paths (mean rollout's reward mean; sampled: actions 1.015, z1_mean 0.861, z 0.467, reward mean 1.417, returns
    0.592, bootstrap 0.551, value 0.587; mean: actions 1.530, z 0.738, returns 0.465, bootstrap 0.657, value 0.465), identical between
    the per-layer and the fused path in every quantity.  a(0) against policy.act(z0) measured 0.708, q_min 0.606."""
    from s2p_amd.slac_imagine import discounted
    m, po, critic = models(IR.A), policies(IR.W, IR.A), _critic(hip_device)
    z0, noise = _inputs(IR.B, IR.H)
    assert np.array_equal(golden["z0"], z0.cpu().numpy()) and np.array_equal(golden["noise"], noise.cpu().numpy())
    worst = {}
    for fused in (False, True):
        ratios = {}
        for rollout, sample in zip(IR.ROLLOUTS, (True, False)):
            act, mean, std, z = _imagine(m, po, fused, z0, noise, sample)
            rm, rs = m.predict_reward(z0, z, act)
            ret = discounted(rm, IR.DISCOUNT)
            zH = z[:, -1].contiguous()
            boot = critic.q_min(zH, po.act(zH))
            val = ret + IR.DISCOUNT ** IR.H * boot.double()
            assert ret.dtype == val.dtype == torch.float64 and ret.is_cuda and boot.shape == (IR.B,)
            got = dict(zip(IR.QUANTITIES, (act, mean, std, z, rm, rs, ret, boot, val)))
            for k in IR.QUANTITIES:
                key = "%s.%s" % (rollout, k)
                want, e32 = golden[key], np.maximum(golden[key + ".ref32_err"], FLOOR)
                err = IR.step_err(got[k], want).numpy() if k in IR.STEPWISE else np.float64(R.rel_max(got[k], want))
                ratios[key] = float(np.max(err / e32))
        worst[fused] = ratios
    with capsys.disabled():
        for key in worst[True]:
            print("\n%-22s deviation / max(ref32_err, 1e-6): per-layer %.6f, fused %.6f" % (key, worst[False][key], worst[True][key]), end="")
        print("\nworst: per-layer %.6f, fused %.6f" % (max(worst[False].values()), max(worst[True].values())))
    for fused in (False, True):
        for key, r in worst[fused].items():
            assert r <= K_TOL, (fused, key, r)
    assert worst[True] == worst[False]


def test_q_min(hip_device, golden):
    critic = _critic(hip_device)
    g = torch.Generator().manual_seed(9)
    z, a = torch.randn(33, Z, generator=g), torch.rand(33, IR.A, generator=g) * 2 - 1
    qs = [{k: v.double() for k, v in IR.make_q_params(i).items()} for i in range(2)]
    want = IR.q_min(qs, z.double(), a.double())
    counts = count_calls(lambda: critic.q_min(z.cuda(), a.cuda()))
    got = critic.q_min(z.cuda(), a.cuda()).clone()
    ref = max(float(max(golden["%s.bootstrap.ref32_err" % r] for r in IR.ROLLOUTS)), FLOOR)
    err = R.rel_max(got, want)
    print("q_min deviates from the fp64 restatement by %.3e (%.3f of max(ref32_err, 1e-6))" % (err, err / ref))
    assert got.shape == (33,) and got.grad_fn is None and err <= K_TOL * ref
    assert counts == {"s2p_mlp_linear_fwd": 3}                                # both networks: one grouped launch per layer
    assert critic.q_min(z[:5].cuda(), a[:5].cuda()).shape == (5,)             # another batch size rebuilds the tables
    assert torch.equal(critic.q_min(z.cuda(), a.cuda()), got)
    with pytest.raises(ValueError):
        critic.q_min(z.cuda(), a[:, :3].cuda())


# ---- 9. call counts --------------------------------------------------------------------------------------------------------------------------
def test_call_counts(models, policies):
    m, po = models(6), policies(256, 6)
    z0, noise = _inputs(17, 5)
    _imagine(m, po, False, z0, noise)                                         # (packs are built on first use)
    per_layer, fused = count_calls(lambda: _imagine(m, po, False, z0, noise)), count_calls(lambda: _imagine(m, po, True, z0, noise))
    print("library calls, per-layer:", per_layer, " fused:", fused)
    assert fused == {NAME: 1}
    assert per_layer == {"s2p_linear_fwd": 9 * 5, "s2p_linear_add_fwd": 2 * 5, "s2p_gauss_head_fwd": 2 * 5}
    assert sum(per_layer.values()) == 13 * 5


# ---- 10. imagined_returns, behaviour and the command line -----------------------------------------------------------------------------------
CONTEXT, HORIZON = 8, 3
KEYS = {"z0", "actions", "z", "z1_mean", "z1_std", "reward_mean", "reward_std", "returns", "bootstrap", "value"}


@pytest.fixture(scope="module")
def real_windows():
    from s2p_amd.slac_predict import gather, windows
    data = SB.real_dataset(2, 12, 100, 100)
    starts = windows(data, CONTEXT + HORIZON, stride=1, limit=3)
    assert starts.tolist() == [0, 12, 13]
    frames, actions, rewards = gather(data, starts, CONTEXT + HORIZON)
    return data, starts, frames, actions, rewards


def _noises(B):
    g = torch.Generator().manual_seed(77)
    return torch.randn(B, CONTEXT + 1, Z, generator=g).cuda(), torch.randn(B, HORIZON, Z, generator=g).cuda()


def _returns(m, po, critic, rw, fused, **kw):
    from s2p_amd.slac_imagine import imagined_returns
    _, _, frames, actions, _ = rw
    pn, n = _noises(frames.shape[0])
    m.fused_chain = fused
    try:
        out = imagined_returns(m, po, frames[:, :CONTEXT + 1], actions[:, :CONTEXT], HORIZON, IR.DISCOUNT, critic, CONTEXT, noise=n,
                               posterior_noise=pn, **kw)
        torch.cuda.synchronize()
        return out
    finally:
        m.fused_chain = False


def test_imagined_returns_and_behaviour(models, policies, real_windows, hip_device):
    from s2p_amd.slac_imagine import behaviour
    from s2p_amd.slac_predict import open_loop
    m, po, critic = models(SB.A), policies(256, SB.A), _critic(hip_device)
    data, starts, frames, actions, rewards = real_windows
    B = frames.shape[0]
    outs = {fused: _returns(m, po, critic, real_windows, fused) for fused in (False, True)}
    o = outs[True]
    assert set(o) == KEYS and all(v.is_cuda and v.grad_fn is None for v in o.values())
    assert o["actions"].shape == (B, HORIZON, SB.A) and o["z"].shape == (B, HORIZON, Z) and o["returns"].shape == (B,)
    assert o["reward_mean"].shape == o["reward_std"].shape == (B, HORIZON) and o["bootstrap"].shape == o["value"].shape == (B,)
    assert all(bool(torch.isfinite(v).all()) for v in o.values()) and float(o["actions"].abs().max()) <= 1.0
    for k in KEYS:
        assert torch.equal(outs[True][k], outs[False][k]), k
    g = IR.DISCOUNT ** torch.arange(HORIZON, dtype=torch.float64).cuda()
    assert o["returns"].dtype == torch.float64 and torch.equal(o["returns"], (o["reward_mean"].double() * g).sum(1))
    assert torch.equal(o["value"], o["returns"] + IR.DISCOUNT ** HORIZON * o["bootstrap"].double())
    zH = o["z"][:, -1].contiguous()
    assert torch.equal(o["bootstrap"], critic.q_min(zH, po.act(zH)))
    assert set(_returns(m, po, None, real_windows, True)) == KEYS - {"bootstrap", "value"}
    # the same start states under the dataset's recorded actions: open_loop's rollout, and the dataset's own reward sum
    pn, n = _noises(B)
    be = behaviour(m, data, starts, CONTEXT, HORIZON, IR.DISCOUNT, noise=n, posterior_noise=pn)
    ol = open_loop(m, frames, actions, rewards, context=CONTEXT, noise=n, posterior_noise=pn)
    assert torch.equal(be["z0"], o["z0"]) and torch.equal(be["z0"], ol["z0"]) and torch.equal(be["z"], ol["z"])
    assert torch.equal(be["reward_mean"], ol["reward_mean"]) and torch.equal(be["actions"].cpu(), torch.as_tensor(actions[:, CONTEXT:]))
    want = (rewards[:, CONTEXT:].astype(np.float64) * IR.DISCOUNT ** np.arange(HORIZON)).sum(1)
    assert np.allclose(be["data_returns"].cpu().numpy(), want, rtol=1e-14, atol=0)
    assert not torch.equal(be["z"], o["z"])                                  # the policy's actions are not the dataset's


def test_imagined_returns_bf16_stacks(models, policies, real_windows):
    """bf16 conv stacks, fp32 heads: z of the rollout within the bound tests/test_latent_predict_gpu.py uses for anything downstream
    of the bf16 encoder (1e-1, R.rel_max) of the fp32 model's."""
    po = policies(256, SB.A)
    ref = _returns(models(SB.A), po, None, real_windows, True)
    got = _returns(build_model(SB.A, torch.bfloat16), po, None, real_windows, True)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    err = R.rel_max(got["z"], ref["z"])
    print("bf16 stacks: z deviates from the fp32 model's by %.3e" % err)
    assert err <= 1e-1


def test_command_line(models, policies, real_windows, hip_device, tmp_path, capsys):
    import imagine_policy
    data = real_windows[0]
    path, ldir, pdir = str(tmp_path / "real.npz"), str(tmp_path / "latent"), str(tmp_path / "policy")
    np.savez(path, **data)
    models(SB.A).save_model(ldir)
    os.makedirs(pdir)
    torch.save(policies(256, SB.A).state_dict(), os.path.join(pdir, "policy.pth"))
    torch.save(_critic(hip_device).state_dict(), os.path.join(pdir, "critic.pth"))
    res = {}
    for fused in (False, True):
        out = str(tmp_path / ("imag%d.npz" % fused))
        argv = ["--data", path, "--latent_dir", ldir, "--policy_dir", pdir, "--out", out, "--context", str(CONTEXT), "--horizon",
                str(HORIZON), "--windows", "3", "--stride", "1", "--batch", "2", "--seed", "4", "--bootstrap"] + (["--fused_chain"] if fused else [])
        imagine_policy.main(argv)
        with np.load(out) as f:
            res[fused] = {k: f[k] for k in f.files}
    text = capsys.readouterr().out
    assert "imagined return" in text and "true reward sum" in text and "mean |a|" in text and "+-" in text and text.count("wrote") == 2
    r = res[True]
    assert set(r) == {"policy_return", "behaviour_return", "data_return", "bootstrap", "policy_value", "actions", "z", "starts"}
    assert r["starts"].tolist() == [0, 12, 13] and r["actions"].shape == (3, HORIZON, SB.A) and r["z"].shape == (3, HORIZON, Z)
    assert all(r[k].shape == (3,) for k in ("policy_return", "behaviour_return", "data_return", "bootstrap", "policy_value"))
    assert all(np.isfinite(r[k]).all() for k in r)
    rows = r["starts"][:, None] + CONTEXT + np.arange(HORIZON)[None]
    want = (data["rewards"][rows].astype(np.float64) * 0.99 ** np.arange(HORIZON)).sum(1)
    assert np.allclose(r["data_return"], want, rtol=1e-14, atol=0)
    for k in r:
        assert np.array_equal(res[True][k], res[False][k]), k
    with pytest.raises(SystemExit, match="no trajectory"):
        imagine_policy.main(["--data", path, "--latent_dir", ldir, "--policy_dir", pdir, "--out", str(tmp_path / "x.npz"), "--horizon", "5"])
