"""The HIP actor (s2p_amd/actor.py, SPEC.md N3f) against the fixture the real reference `rollout()` wrote
(tests/golden/make_golden_actor.py): every step's policy input and action of the fixture's episodes within
K_TOL x max(ref32_err, 1e-6), K_TOL = 4 (the project's rule: ref32_err is the deviation of the reference's own fp32 run from its fp64
run); a batch of three staggered environments against each environment alone, bitwise; the cached feature window against a full
re-encode of its frames; the bf16 encoder; and the command line in a child process."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import actor_ref as AR
import slac_latent_ref as R
import slac_oracle as SO

pytestmark = pytest.mark.gpu
K_TOL, FLOOR = 4.0, 1e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "actor_golden_v1.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def latent_p():
    return R.make_params(AR.A)


@pytest.fixture(scope="module")
def algos(hip_device, latent_p):
    """dtype -> the stand-in for `SlacAlgorithm` the actor needs (latent, state_shape, action_shape, num_sequences); built once."""
    from s2p_amd.slac import LatentModel
    cache = {}

    def get(dtype=torch.float32):
        if dtype not in cache:
            m = LatentModel(AR.STATE_SHAPE, (AR.A,), image_size=100, dtype=dtype)
            m.load_state_dict(R.full_state_dict(latent_p), strict=True)
            cache[dtype] = types.SimpleNamespace(latent=m, state_shape=AR.STATE_SHAPE, action_shape=(AR.A,), num_sequences=AR.S)
        return cache[dtype]
    return get


def _policy(input_type):
    from s2p_amd.offline_rl import TanhGaussianPolicy
    obs_dim = AR.obs_dim_of(input_type)
    return TanhGaussianPolicy([AR.H, AR.H], obs_dim, AR.A).load_state_dict(AR.make_policy_params(obs_dim), strict=True)


def _actor(algos, input_type, same_obs=False, num_envs=1, dtype=torch.float32):
    from s2p_amd.actor import SlacActor
    return SlacActor(_policy(input_type), algos(dtype), num_envs, input_type, same_obs)


class _Recording:
    """A `SlacActor` that keeps every step's policy input, as `actor_ref.RefActor` does."""

    def __init__(self, actor):
        self.actor, self.inputs, self.input_type = actor, [], actor.input_type

    def reset(self, frames, mask=None):
        self.actor.reset(frames, mask)

    def observe(self, frames, actions, reset_mask=None):
        self.actor.observe(frames, actions, reset_mask)

    def act(self, noise=None):
        a = self.actor.act(noise)
        x = self.actor.ob.feature_action if self.input_type == "feature_action" else self.actor._z[:, :AR.Z]
        self.inputs.append(x.detach().cpu().clone())
        return a


@pytest.mark.parametrize("same_obs", [False, True])
@pytest.mark.parametrize("input_type", AR.INPUT_TYPES)
def test_fixture_episodes_fp32(golden, algos, input_type, same_obs):
    name = AR.config_name(input_type, same_obs)
    actor = _Recording(_actor(algos, input_type, same_obs))
    env = AR.ScriptedEnv()
    tol_in = K_TOL * max(float(golden[name + ".input.ref32_err"]), FLOOR)
    tol_act = K_TOL * max(float(golden[name + ".action.ref32_err"]), FLOOR)
    worst_in = worst_act = 0.0
    for ep in range(AR.EPISODES):
        actor.inputs = []
        inputs, actions, ret, length, terminal = AR.run_ref_episode(actor, env, ep)
        assert (ret, length, terminal) == (float(golden["%s.ep%d.return" % (name, ep)]), int(golden["%s.ep%d.length" % (name, ep)]),
                                           bool(golden["%s.ep%d.terminal" % (name, ep)]))
        want = golden["%s.ep%d.actions" % (name, ep)]
        for t, (x, a) in enumerate(zip(inputs, actions)):
            pre = "%s.ep%d.input%d." % (name, ep, t)
            e_in = AR.input_err(x, {k[len(pre):]: v for k, v in golden.items() if k.startswith(pre)})
            e_act = R.rel_max(a, want[t])
            worst_in, worst_act = max(worst_in, e_in), max(worst_act, e_act)
            print("%s ep %d step %2d  input err %.3e (tol %.3e)  action err %.3e (tol %.3e)" % (name, ep, t, e_in, tol_in, e_act, tol_act))
            assert a.dtype == np.float32 and a.shape == (AR.A,)
    print("%s worst: input %.3e / %.3e, action %.3e / %.3e" % (name, worst_in, tol_in, worst_act, tol_act))
    assert worst_in <= tol_in and worst_act <= tol_act, (name, worst_in, tol_in, worst_act, tol_act)


STAGGER = ((9, None), (6, None), (4, None))


class _SeededNoise:
    """`latent_z` draws its eps on the device; here a slot's eps is a function of (environment, step) alone, whatever the batch."""

    def __init__(self, actor, env_ids):
        self.actor, self.env_ids, self.k = actor, env_ids, 0

    def reset(self, *a):
        self.actor.reset(*a)

    def observe(self, *a):
        self.actor.observe(*a)

    def act(self):
        noise = None
        if self.actor.input_type == "latent_z":
            noise = torch.cat([torch.randn(1, AR.S, AR.Z, generator=torch.Generator().manual_seed(1000 * e + self.k)) for e in self.env_ids])
        self.k += 1
        return self.actor.act(noise)


@pytest.mark.parametrize("input_type", AR.INPUT_TYPES)
def test_three_staggered_environments_equal_each_alone_bitwise(algos, input_type):
    """Three scripted environments whose first episodes end at steps 9 / 6 / 4 (the later ones at the cap of 10), five episodes in
    all: the resets fall on different steps.  Each slot's actions are BITWISE those of a num_envs = 1 run on that environment alone
    (lock-step keeps a slot's step count equal to the batch's, so both runs hand a slot the same eps)."""
    from s2p_amd.actor import run_episodes

    def run(env_ids, episodes):
        envs = [AR.ScriptedEnv(STAGGER[e], seed=500 + e) for e in env_ids]
        run_episodes(envs, _SeededNoise(_actor(algos, input_type, False, len(env_ids)), env_ids), episodes, 10)
        return envs

    together = run((0, 1, 2), 5)
    assert [e.episode + 1 for e in together] == [1, 2, 2]
    for e, env in enumerate(together):
        alone = run((e,), env.episode + 1)[0]
        n = len(env.actions)
        assert n > 0 and len(alone.actions) == n
        got, want = np.stack(env.actions), np.stack(alone.actions)
        print("environment %d: %d steps, largest difference %.3e" % (e, n, float(np.abs(got - want).max())))
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32)), e


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-4), (torch.bfloat16, 4e-2)])
def test_cached_window_equals_a_full_reencode(algos, dtype, tol):
    """11 steps into an episode (the window has wrapped) the cached features equal `Encoder.forward` on the window's 8 frames, and
    the fp64 oracle's features, within the bounds tests/test_slac.py holds features to; the bf16 actions are finite and in (-1, 1)."""
    actor = _actor(algos, "feature_action", False, 1, dtype)
    env = AR.ScriptedEnv((None,))
    actor.reset(env.reset()[None])
    for t in range(11):
        a = actor.act()
        assert a.shape == (1, AR.A) and np.isfinite(a).all() and (np.abs(a) < 1).all()
        o, _, _, _ = env.step(a[0])
        actor.observe(o[None], a)
    window = env.frames[11 - AR.S + 1:12]                                          # [8,3,100,100]
    cached = actor.ob.features.detach().cpu()
    enc = algos(dtype).latent.encoder
    full = enc(torch.from_numpy(window).permute(0, 2, 3, 1).contiguous()[None]).detach().cpu()
    oracle = SO.encoder_forward({k[len("encoder."):]: v.double() for k, v in R.make_params(AR.A).items() if k.startswith("encoder.")},
                                torch.from_numpy(window)[None].double() / 255.0)
    print("cached vs Encoder.forward %.3e, vs the fp64 oracle %.3e (bound %.0e)" % (R.rel_max(cached, full), R.rel_max(cached, oracle), tol))
    assert cached.shape == (1, AR.S, AR.FEAT) and R.rel_max(cached, full) < tol and R.rel_max(cached, oracle) < tol
    acts = actor.ob.actions.detach().cpu()
    assert acts.shape == (1, AR.S - 1, AR.A) and torch.equal(acts[0], torch.from_numpy(np.stack(env.actions[-(AR.S - 1):])))


def test_masked_reset_keeps_the_other_slots(algos):
    """`reset(frames, mask)` on a partial mask leaves the unmasked rows bit for bit as they were."""
    actor = _actor(algos, "feature_action", False, 3)
    frames = np.stack([AR.make_frames(7, e)[0] for e in range(3)])
    actor.reset(frames)
    actor.observe(np.stack([AR.make_frames(7, e)[1] for e in range(3)]), np.full((3, AR.A), 0.25, dtype=np.float32))
    before = actor.ob.feature_action.detach().cpu().clone()
    actor.reset(frames[::-1].copy(), np.array([False, True, False]))
    after = actor.ob.feature_action.detach().cpu()
    assert torch.equal(after[0], before[0]) and torch.equal(after[2], before[2]) and not torch.equal(after[1], before[1])
    assert bool((after[1, AR.S * AR.FEAT:] == 0).all()) and torch.equal(after[1, :AR.FEAT], actor.ob.fill.cpu())


def test_evaluate_policy_command_line(hip_device, latent_p, tmp_path):
    """`evaluate_policy.py --env replay:...` on a 2-trajectory, 12-frame synthetic dataset in a fresh child process: the returns it
    writes are the dataset's reward sums, in completion order."""
    rng = np.random.RandomState(3)
    frames = rng.randint(0, 256, size=(12, 100, 100, 3)).astype(np.uint8)          # NHWC, as the dataset files hold them
    rewards = rng.rand(12).astype(np.float32)
    terminals, timeouts = np.zeros(12, dtype=bool), np.zeros(12, dtype=bool)
    terminals[6], timeouts[11] = True, True                                       # trajectories of 7 and 5 rows
    data = os.path.join(tmp_path, "replay.npz")
    np.savez(data, image_observations=frames, rewards=rewards, terminals=terminals, timeouts=timeouts)
    torch.save(R.full_state_dict(latent_p), os.path.join(tmp_path, "latent.pth"))
    torch.save(AR.make_policy_params(AR.P), os.path.join(tmp_path, "policy.pth"))
    out = os.path.join(tmp_path, "returns.npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate_policy.py"), "--latent_dir", str(tmp_path), "--policy_dir", str(tmp_path),
                        "--env", "replay:" + data, "--episodes", "2", "--num_envs", "2", "--max_path_length", "20", "--out", out],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Average Returns" in p.stdout
    got = np.load(out)
    want = [float(rewards[7:].astype(np.float64).sum()), float(rewards[:7].astype(np.float64).sum())]
    assert got["returns"].tolist() == want and got["lengths"].tolist() == [5, 7] and got["terminals"].tolist() == [False, True]
    assert float(got["average_return"]) == pytest.approx(np.mean(want))
