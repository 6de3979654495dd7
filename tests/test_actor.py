"""Policy evaluation on SLAC latents, CPU side (SPEC.md N3f): the plain-torch restatement of the acting step against the fixture the
real reference `rollout()` wrote (tests/golden/make_golden_actor.py), then the lock-step episode loop and `ReplayEnv` on it."""
import os

import numpy as np
import pytest
import torch

import actor_ref as AR
import slac_latent_ref as R
from s2p_amd.actor import ReplayEnv, run_episodes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "actor_golden_v1.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def latent_p():
    return R.make_params(AR.A)


def test_fixture_weights_are_the_seeded_ones(golden, latent_p):
    assert golden["sizes"].tolist() == [AR.A, AR.H, AR.S, AR.DONE_STEP, AR.MAX_PATH, AR.EPISODES]
    ps = [AR.make_policy_params(AR.obs_dim_of(t)) for t in AR.INPUT_TYPES]
    assert abs(AR.checksum(latent_p, ps) - float(golden["checksum"])) <= 1e-9 * float(golden["checksum"])


@pytest.mark.parametrize("same_obs", [False, True])
@pytest.mark.parametrize("input_type", AR.INPUT_TYPES)
def test_restatement_reproduces_the_reference_rollout(golden, latent_p, input_type, same_obs):
    """fp64, 1e-9: every step's policy input (for `latent_z` this pins WHICH z the policy reads) and action, and per episode the
    return, the length and the terminal flag (episode 0 ends by `done`, episode 1 by the length cap)."""
    torch.set_num_threads(8)
    name = AR.config_name(input_type, same_obs)
    actor = AR.RefActor(latent_p, AR.make_policy_params(AR.obs_dim_of(input_type)), 1, input_type, same_obs)
    env = AR.ScriptedEnv()
    for ep in range(AR.EPISODES):
        inputs, actions, ret, length, terminal = AR.run_ref_episode(actor, env, ep)
        assert (ret, length, terminal) == (float(golden["%s.ep%d.return" % (name, ep)]), int(golden["%s.ep%d.length" % (name, ep)]),
                                           bool(golden["%s.ep%d.terminal" % (name, ep)]))
        assert R.rel_max(np.stack(actions), golden["%s.ep%d.actions" % (name, ep)]) < 1e-9
        for t, x in enumerate(inputs):
            pre = "%s.ep%d.input%d." % (name, ep, t)
            rec = {k[len(pre):]: v for k, v in golden.items() if k.startswith(pre)}
            assert rec and AR.input_err(x, rec) < 1e-9, (ep, t)
    assert [int(golden["%s.ep%d.length" % (name, e)]) for e in range(2)] == [AR.DONE_STEP, AR.MAX_PATH]
    assert [bool(golden["%s.ep%d.terminal" % (name, e)]) for e in range(2)] == [True, False]


def test_latent_z_reads_the_previous_frames_latent(latent_p):
    """The quirk kept from the reference: the policy's `latent_z` input is z_[:, -2], not the newest latent."""
    actor = AR.RefActor(latent_p, AR.make_policy_params(AR.Z), 1, "latent_z", False)
    env = AR.ScriptedEnv()
    actor.reset(env.reset()[None])
    noise = AR.make_noise(0, 0)
    x = actor.policy_input(noise)
    state = torch.as_tensor(np.stack(list(actor.state[0])))[None].double() / 255.0
    action = torch.as_tensor(np.stack(list(actor.action[0])))[None].double()
    _, _, z1, z2 = R.sample_posterior(actor.p, AR.SO.encoder_forward(actor.enc, state), action, noise.double())
    z = torch.cat([z1, z2], dim=-1)
    assert torch.equal(x, z[:, -2]) and not torch.allclose(x, z[:, -1])


# ---- ReplayEnv and the episode loop ------------------------------------------------------------------------------------------------
def _dataset(lengths, terminal_ends, shape=(3, 4, 4), tp1=False):
    """Trajectories of the given lengths; trajectory i ends by a terminal if terminal_ends[i], else by a timeout.  Frame values count
    up, so a frame names its row."""
    T = sum(lengths)
    frames = (np.arange(T, dtype=np.uint8)[:, None, None, None] + np.zeros(shape, dtype=np.uint8))
    rewards = np.arange(1, T + 1, dtype=np.float32) * 0.25
    terminals, timeouts = np.zeros(T, dtype=bool), np.zeros(T, dtype=bool)
    end = -1
    for n, term in zip(lengths, terminal_ends):
        end += n
        (terminals if term else timeouts)[end] = True
    d = dict(image_observations=frames, rewards=rewards, terminals=terminals, timeouts=timeouts)
    if tp1:
        d["image_observations_tp1"] = frames + 100
    return d


def test_replay_env_on_a_synthetic_dataset():
    d = _dataset([3, 2], [True, False])
    env = ReplayEnv(d, 1)
    assert env.num_trajectories == 2 and len(env) == 2
    assert int(env.reset()[0, 0, 0]) == 3
    o, r, done, info = env.step(np.zeros(2))
    assert (int(o[0, 0, 0]), r, done, info) == (4, 1.0, False, {})
    o, r, done, info = env.step(None)
    assert (int(o[0, 0, 0]), r, done, info) == (4, 1.25, True, {"TimeLimit.truncated": True})       # no next frame recorded: the last again
    with pytest.raises(RuntimeError):
        env.step(None)
    assert int(env.reset()[0, 0, 0]) == 3                                  # reset() starts the same trajectory again
    env = ReplayEnv(d, 0)
    steps = [env.step(None) for _ in range(3)]
    assert [s[2] for s in steps] == [False, False, True] and steps[-1][3] == {} and [int(s[0][0, 0, 0]) for s in steps] == [1, 2, 2]
    with pytest.raises(IndexError):
        ReplayEnv(d, 2)
    env = ReplayEnv(_dataset([3], [True], tp1=True), 0)                     # recorded next frames are handed out as they are
    env.reset()
    assert [int(env.step(None)[0][0, 0, 0]) for _ in range(3)] == [100, 101, 102]
    nhwc = dict(d, image_observations=np.zeros((5, 4, 4, 3), dtype=np.uint8))
    assert ReplayEnv(nhwc, 0).reset().shape == (3, 4, 4)                    # NHWC datasets are handed out CHW
    only_timeouts = {k: v for k, v in d.items() if k != "terminals"}
    assert ReplayEnv(only_timeouts, 0).num_trajectories == 1 and len(ReplayEnv(only_timeouts, 0)) == 5


class _CountingActor:
    """Records every call's mask; its action for slot n names the call."""

    def __init__(self, N):
        self.N, self.calls, self.k = N, [], 0

    def reset(self, frames, mask=None):
        self.calls.append(("reset", np.array(mask, copy=True), frames[:, 0, 0, 0].copy()))

    def observe(self, frames, actions, reset_mask=None):
        self.calls.append(("observe", np.array(reset_mask, copy=True), frames[:, 0, 0, 0].copy()))

    def act(self):
        self.k += 1
        return np.full((self.N, 2), float(self.k), dtype=np.float32)


def test_run_episodes_returns_lengths_and_terminal_flags():
    """One slot, three episodes on a 3-trajectory dataset: by `done` (a terminal), by `TimeLimit.truncated` (a timeout) and by the
    length cap.  Returns are the dataset's reward sums."""
    d = _dataset([3, 2, 6], [True, False, True])

    class Cycle:                                                           # trajectory 0, 1, 2 on successive resets
        def __init__(self):
            self.k, self.env = -1, None

        def reset(self):
            self.k += 1
            self.env = ReplayEnv(d, self.k)
            return self.env.reset()

        def step(self, a):
            return self.env.step(a)

    out = run_episodes([Cycle()], _CountingActor(1), episodes=3, max_path_length=4)
    r = d["rewards"].astype(np.float64)
    assert out["returns"].tolist() == [r[0:3].sum(), r[3:5].sum(), r[5:9].sum()]
    assert out["lengths"].tolist() == [3, 2, 4] and out["terminals"].tolist() == [True, False, False]
    assert out["average_return"] == pytest.approx(np.mean([r[0:3].sum(), r[3:5].sum(), r[5:9].sum()]))
    empty = run_episodes([Cycle()], _CountingActor(1), episodes=0, max_path_length=4)
    assert len(empty["returns"]) == 0 and np.isnan(empty["average_return"])


def test_run_episodes_masks_with_three_slots_and_five_episodes():
    """Slots replay trajectories of 2, 4 and 3 steps and 5 episodes are started in all: slots 0, 1, 2 at the start, slot 0 again after
    step 2, slot 2 again after step 3; the slots that end later idle.  Every call carries the mask of the slots that restart."""
    d = _dataset([2, 4, 3], [True, True, True])
    envs = [ReplayEnv(d, k) for k in range(3)]
    actor = _CountingActor(3)
    out = run_episodes(envs, actor, episodes=5, max_path_length=10)
    assert [c[0] for c in actor.calls] == ["reset"] + ["observe"] * 5
    assert [c[1].tolist() for c in actor.calls] == [[True, True, True],
                                                    [False, False, False],      # after step 1
                                                    [True, False, False],       # after step 2: slot 0 ended and starts episode 4
                                                    [False, False, True],       # after step 3: slot 2 ended and starts episode 5
                                                    [False, False, False],      # after step 4: slots 0 and 1 ended and idle
                                                    [False, False, False]]      # after step 5; slot 2 ends at step 6: no call follows
    # the frame a restarting slot hands over is its trajectory's first (row 0 of trajectory 0, row 6 of trajectory 2)
    assert int(actor.calls[2][2][0]) == 0 and int(actor.calls[3][2][2]) == 6
    r = d["rewards"].astype(np.float64)
    t0, t1, t2 = r[0:2].sum(), r[2:6].sum(), r[6:9].sum()
    assert out["returns"].tolist() == [t0, t2, t0, t1, t2] and out["lengths"].tolist() == [2, 3, 2, 4, 3]
    assert out["terminals"].all() and actor.k == 6


def test_run_episodes_with_the_reference_actor_on_replayed_frames(latent_p):
    """The fp64 restatement as the actor of `run_episodes`, two slots against one: a slot's actions do not depend on its neighbours
    (to 1e-12: the restatement is fp64)."""
    torch.set_num_threads(8)
    pol = AR.make_policy_params(AR.P)
    envs = [AR.ScriptedEnv((3, None)), AR.ScriptedEnv((2, None), seed=77)]
    out = run_episodes(envs, AR.RefActor(latent_p, pol, 2, "feature_action", False), episodes=2, max_path_length=3)
    assert out["lengths"].tolist() == [2, 3] and out["returns"].tolist() == [1.5, 3.0] and out["terminals"].tolist() == [True, True]
    solo = AR.ScriptedEnv((3, None))
    run_episodes([solo], AR.RefActor(latent_p, pol, 1, "feature_action", False), episodes=1, max_path_length=3)
    assert np.allclose(np.stack(solo.actions), np.stack(envs[0].actions), rtol=0, atol=1e-12)
