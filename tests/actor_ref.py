"""Plain-torch restatement of the SLAC acting step (SPEC.md N3f) with a deque per environment, the scripted environment and the seeded
weights / frames / noise of its fixture -- TEST INFRASTRUCTURE ONLY.  Shared by tests/golden/make_golden_actor.py (which runs the real
reference `rollout()` on these) and by tests/test_actor.py / tests/test_actor_gpu.py (which check this restatement, then the HIP
actor, against the recorded fp64 results)."""
from collections import deque

import numpy as np
import torch
import torch.nn.functional as F

import slac_latent_ref as R
import slac_oracle as SO

A, H, S, FEAT, Z = 3, 64, 8, 256, 288
P = S * FEAT + (S - 1) * A
STATE_SHAPE = (3, 100, 100)
DONE_STEP, MAX_PATH, EPISODES = 11, 13, 2
SEEDS = dict(frames=931, policy=932, noise=933)
INPUT_TYPES = ("feature_action", "latent_z")
NSAMP = 256


def config_name(input_type, same_obs):
    return "%s.%s" % (input_type, "same" if same_obs else "zero")


def make_frames(seed, episode):
    """The MAX_PATH + 1 frames of one scripted episode, uint8 [14,3,100,100]."""
    return np.random.RandomState(seed * 100 + episode).randint(0, 256, size=(MAX_PATH + 1,) + STATE_SHAPE).astype(np.uint8)


class _Space:
    def __init__(self, shape):
        self.shape = shape


class ScriptedEnv:
    """Episode e (the e-th `reset()`) shows the frames of `make_frames(seed, e)`; step t (1-based) pays 0.5 t and is `done` at
    `done_steps[e]` (None: never -- the length cap ends the episode).  The action is ignored."""

    def __init__(self, done_steps=(DONE_STEP, None), seed=None):
        self.done_steps, self.seed = tuple(done_steps), SEEDS["frames"] if seed is None else seed
        self.observation_space, self.action_space = _Space(STATE_SHAPE), _Space((A,))
        self.episode, self.t, self.actions = -1, 0, []

    def reset(self):
        self.episode += 1
        self.frames, self.t = make_frames(self.seed, self.episode), 0
        return self.frames[0].copy()

    def step(self, action):
        self.t += 1
        self.actions.append(np.array(action, copy=True))
        return self.frames[self.t].copy(), 0.5 * self.t, self.t == self.done_steps[self.episode % len(self.done_steps)], {}


def make_policy_params(obs_dim, seed=None):
    """Seeded weights of TanhGaussianPolicy(hidden [H, H], obs_dim, A) under the reference's keys.  The reference's +-1e-3 last
    layer would leave every action near 0: `last_fc` is drawn wide enough that tanh(mean) spreads over (-1, 1)."""
    g = torch.Generator().manual_seed((SEEDS["policy"] if seed is None else seed) + obs_dim)
    p, n_in = {}, obs_dim
    for i in range(2):
        p["fc%d.weight" % i] = (torch.rand(H, n_in, generator=g) * 2 - 1) / H ** 0.5
        p["fc%d.bias" % i] = torch.randn(H, generator=g) * 0.05
        n_in = H
    p["last_fc.weight"] = (torch.rand(A, H, generator=g) * 2 - 1) * (1.5 if obs_dim == P else 0.3)     # (the feature rows are the smaller input)
    p["last_fc.bias"] = torch.randn(A, generator=g) * 0.05
    p["last_fc_log_std.weight"] = (torch.rand(A, H, generator=g) * 2 - 1) * 1e-3
    p["last_fc_log_std.bias"] = (torch.rand(A, generator=g) * 2 - 1) * 1e-3
    return p


def obs_dim_of(input_type):
    return P if input_type == "feature_action" else Z


def make_noise(episode, t):
    """eps of the posterior sample of step t of an episode, [1, S, 288]."""
    g = torch.Generator().manual_seed(SEEDS["noise"] * 10000 + episode * 100 + t)
    return torch.randn(1, S, Z, generator=g)


def checksum(latent_p, policy_ps):
    return float(R.checksum(latent_p) + sum(R.checksum(p) for p in policy_ps))


def sample(v):
    f = torch.as_tensor(v).detach().double().flatten().cpu()
    return f[::max(1, f.numel() // NSAMP)][:NSAMP]


def input_record(x):
    """What the fixture keeps of one policy input: the whole row where it is short, else its norm, sum and a strided sample."""
    x = torch.as_tensor(x).detach().double().flatten().cpu()
    if x.numel() <= 512:
        return dict(full=x.numpy())
    return dict(norm=np.float64(x.norm()), sum=np.float64(x.sum()), samp=sample(x).numpy())


def input_err(x, rec):
    """The deviation of a policy input from its record, relative to the record's size: the largest of the measures it holds."""
    x = torch.as_tensor(x).detach().double().flatten().cpu()
    if "full" in rec:
        return R.rel_max(x, rec["full"])
    n = float(rec["norm"])
    return max(abs(float(x.norm()) - n) / n, abs(float(x.sum()) - float(rec["sum"])) / (n * x.numel() ** 0.5),
               R.rel_max(sample(x), rec["samp"]))


class RefActor:
    """The acting step restated: a deque of frames and one of actions per slot, the whole window re-encoded on every `act` (what the
    reference does), `preprocess` / `prepare_batch`, the policy MLP and tanh(mean).  Duck-types `SlacActor`."""

    def __init__(self, latent_p, policy_p, num_envs=1, input_type="feature_action", reset_w_same_obs=False, dtype=torch.float64):
        self.p = {k: v.to(dtype) for k, v in latent_p.items()}
        self.enc = {k[len("encoder."):]: v for k, v in self.p.items() if k.startswith("encoder.")}
        self.pol = {k: v.to(dtype) for k, v in policy_p.items()}
        self.N, self.input_type, self.same, self.dtype = num_envs, input_type, reset_w_same_obs, dtype
        self.state, self.action, self.inputs, self.calls = [None] * num_envs, [None] * num_envs, [], []

    def _reset_slot(self, n, frame):
        self.state[n], self.action[n] = deque(maxlen=S), deque(maxlen=S - 1)
        for _ in range(S - 1):
            self.state[n].append(frame.copy() if self.same else np.zeros(STATE_SHAPE, dtype=np.uint8))
            self.action[n].append(np.zeros(A, dtype=np.float64))
        self.state[n].append(frame.copy())

    def reset(self, frames, mask=None):
        mask = np.ones(self.N, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
        self.calls.append(("reset", mask.copy()))
        for n in np.flatnonzero(mask):
            self._reset_slot(n, np.asarray(frames[n]))

    def observe(self, frames, actions, reset_mask=None):
        mask = np.zeros(self.N, dtype=bool) if reset_mask is None else np.asarray(reset_mask, dtype=bool)
        self.calls.append(("observe", mask.copy()))
        for n in range(self.N):
            if mask[n]:
                self._reset_slot(n, np.asarray(frames[n]))
            else:
                self.state[n].append(np.asarray(frames[n]).copy())
                self.action[n].append(np.asarray(actions[n], dtype=np.float64).copy())

    def policy_input(self, noise=None):
        state = torch.as_tensor(np.stack([np.stack(list(s)) for s in self.state])).to(self.dtype) / 255.0     # [N,S,3,100,100]
        action = torch.as_tensor(np.stack([np.stack(list(a)) for a in self.action])).to(self.dtype)          # [N,S-1,A]
        feat = SO.encoder_forward(self.enc, state)
        if self.input_type == "feature_action":
            return torch.cat([feat.reshape(self.N, -1), action.reshape(self.N, -1)], dim=1)
        if noise is None:
            noise = torch.randn(self.N, S, Z)
        _, _, z1, z2 = R.sample_posterior(self.p, feat, action, noise.to(self.dtype))
        return torch.cat([z1, z2], dim=-1)[:, -2]              # the latent of the PREVIOUS frame (rollout_functions.py:151 with algo.py:135)

    def act(self, noise=None):
        with torch.no_grad():
            x = self.policy_input(noise)
            self.inputs.append(x.clone())
            h = F.relu(F.linear(x, self.pol["fc0.weight"], self.pol["fc0.bias"]))
            h = F.relu(F.linear(h, self.pol["fc1.weight"], self.pol["fc1.bias"]))
            return torch.tanh(F.linear(h, self.pol["last_fc.weight"], self.pol["last_fc.bias"])).numpy()


def run_ref_episode(actor, env, episode, max_path_length=MAX_PATH):
    """One episode of slot 0 of `actor` the way the reference's `rollout()` steps it, with the fixture's recorded noise:
    -> (inputs [T], actions [T], return, length, terminal)."""
    actor.reset(env.reset()[None])
    inputs, actions, ret, t, terminal = [], [], 0.0, 0, False
    while t < max_path_length:
        a = actor.act(make_noise(episode, t) if actor.input_type == "latent_z" else None)[0]
        inputs.append(actor.inputs[-1][0] if actor.inputs else None)
        actions.append(a)
        o, r, done, info = env.step(a.copy())
        ret, t = ret + r, t + 1
        if done:
            terminal = not info.get("TimeLimit.truncated", False)
            break
        actor.observe(o[None], a[None])
    return inputs, actions, ret, t, terminal
