"""Policy evaluation on SLAC latents (SPEC.md N3f; reference `rlkit/torch/slac/trainer.py:12-47` SlacObservation,
`rlkit/torch/slac/algo.py:75-81` preprocess, `rlkit/samplers/rollout_functions.py:127-205` the SLAC branch of `rollout()`).

The reference rebuilds an [1,8,3,100,100] window from a deque on every environment step, uploads it, encodes all 8 frames and
copies the policy input to the host and back.  Here the observation state of `num_envs` environments stays on the device AS the
policy-input rows: a step uploads one frame per environment, encodes those frames alone, shifts the new feature and action into
the rows (s2p_feature_action_push, two ping-pong buffers) and runs the three policy layers on one wave per output column
(s2p_mlp_linear_fwd_skinny).  `run_episodes` steps a list of environments in lock-step over one device batch; `ReplayEnv` replays a
dataset trajectory where no simulator is installed.  No CPU fallback: `SlacObservationBatch` and `SlacActor` need a HIP device
(`run_episodes` and `ReplayEnv` are plain Python)."""
import numpy as np
import torch

from ._lib import check, chunk_elems, dtype_id, lib, ptr, stream
from .mlp import Net, fwd_plan, fwd_tables, run
from .ops import pad_to
from .slac import FEAT, Z1, Z2

APPEND, RESET_FILL, RESET_SAME = 0, 1, 2          # the reset codes of s2p_feature_action_push


class SlacObservationBatch:
    """`SlacObservation` for `num_envs` environments at once, device-resident.  Row n of `feature_action` is
    [f_0 .. f_{S-1} | a_0 .. a_{S-2}] of environment n -- what `preprocess` concatenates -- so the policy reads the state in place.
    `fill` is the encoder's feature of an all-zero frame (the S-1 frames `reset_episode` pads a new episode with): `refresh()`
    recomputes it, call it after the encoder's weights change."""

    def __init__(self, num_envs, state_shape, action_shape, num_sequences, encoder, reset_w_same_obs=False):
        self.N, self.S, self.A, self.F = int(num_envs), int(num_sequences), int(action_shape[0]), FEAT
        self.state_shape, self.encoder, self.device = tuple(int(s) for s in state_shape), encoder, encoder.device
        if self.N < 1 or self.S < 1 or len(self.state_shape) != 3:
            raise ValueError("num_envs >= 1, num_sequences >= 1 and a [C,H,W] state_shape are needed")
        self.reset_code = RESET_SAME if reset_w_same_obs else RESET_FILL
        self.P = self.S * self.F + (self.S - 1) * self.A
        self.pitch = pad_to(self.P, 4)
        dev, f = self.device, torch.float32
        self._buf = [torch.zeros(self.N, self.pitch, dtype=f, device=dev) for _ in range(2)]
        self._cur = 0
        # ONE pinned staging buffer and ONE device buffer per step's upload: the frames, then the actions (fp32), then the reset codes
        # (int32), each part on a 16-byte boundary
        C, H, W = self.state_shape
        Ap = max(self.A, 1)
        o_act = pad_to(self.N * C * H * W, 16)
        o_code = o_act + pad_to(self.N * Ap * 4, 16)
        self._stage = torch.zeros(o_code + self.N * 4, dtype=torch.uint8).pin_memory()
        self._dev = torch.zeros(o_code + self.N * 4, dtype=torch.uint8, device=dev)

        def parts(b):
            return (b[:self.N * C * H * W].view((self.N,) + self.state_shape), b[o_act:o_act + self.N * Ap * 4].view(f).view(self.N, Ap),
                    b[o_code:].view(torch.int32))
        self._stage_frames, self._stage_act, self._stage_code = (t.numpy() for t in parts(self._stage))
        self._frames, self._act, self._code = parts(self._dev)
        self._nhwc = torch.empty(self.N, H, W, chunk_elems(encoder.dtype), dtype=encoder.dtype, device=dev)
        self._uploaded = None
        self.fill = torch.zeros(self.F, dtype=f, device=dev)
        self.refresh()

    # ---- the pieces of a step -------------------------------------------------------------------------------------------------------
    def _encode(self, frames_dev, nhwc):
        """uint8 [n,C,H,W] on the device -> fp32 features [n,256]: one conversion launch, one encoder pass over n frames."""
        n, (C, H, W) = frames_dev.shape[0], self.state_shape
        check(lib().s2p_u8_chw_to_nhwc01(dtype_id(nhwc.dtype), ptr(frames_dev), n, C, H, W, ptr(nhwc), nhwc.shape[3], stream()),
              "s2p_u8_chw_to_nhwc01")
        with torch.no_grad():
            return self.encoder.run(nhwc).reshape(n, -1).float()

    def refresh(self):
        zero = torch.zeros((1,) + self.state_shape, dtype=torch.uint8, device=self.device)
        self.fill.copy_(self._encode(zero, torch.empty_like(self._nhwc[:1]))[0])

    def _upload(self, frames, actions, codes):
        """Host arrays -> the device through the pinned staging buffer, one asynchronous copy (the staging buffer is not rewritten
        before the previous step's copy has left it)."""
        if self._uploaded is not None:
            self._uploaded.synchronize()
        frames = np.asarray(frames)
        if frames.shape != self._stage_frames.shape or frames.dtype != np.uint8:
            raise ValueError("frames: uint8 %s are needed, got %s %s" % (self._stage_frames.shape, frames.dtype, frames.shape))
        self._stage_frames[...] = frames
        if actions is not None and self.A:
            self._stage_act[...] = np.asarray(actions, dtype=np.float32).reshape(self.N, self.A)
        self._stage_code[...] = codes
        self._dev.copy_(self._stage, non_blocking=True)
        self._uploaded = torch.cuda.Event()
        self._uploaded.record()

    def _push(self, feat):
        src, dst = self._buf[self._cur], self._buf[1 - self._cur]
        check(lib().s2p_feature_action_push(ptr(src), ptr(dst), self.pitch, self.N, self.S, self.F, self.A, ptr(feat), feat.shape[1],
                                            ptr(self._act), self._act.shape[1], ptr(self._code), ptr(self.fill), stream()),
              "s2p_feature_action_push")
        self._cur = 1 - self._cur

    def _mask(self, mask, default):
        if mask is None:
            return np.full(self.N, default, dtype=bool)
        mask = np.asarray(mask, dtype=bool).reshape(-1)
        if mask.shape != (self.N,):
            raise ValueError("a mask of %d slots is needed" % self.N)
        return mask

    # ---- SlacObservation's surface --------------------------------------------------------------------------------------------------
    def reset(self, frames, mask=None):
        """`reset_episode(frames[n])` for the masked slots (all of them without a mask); the other slots keep their state."""
        mask = self._mask(mask, True)
        self._upload(frames, None, np.where(mask, self.reset_code, APPEND).astype(np.int32))
        prev = self._buf[self._cur]
        self._push(self._encode(self._frames, self._nhwc))
        if not mask.all():                          # (the push appended to the unmasked rows: hand them their previous state back)
            keep = (self._code == APPEND)[:, None]
            torch.where(keep, prev, self._buf[self._cur], out=self._buf[self._cur])

    def append(self, frames, actions, reset_mask=None):
        """`append(frames[n], actions[n])` for every slot; a slot in `reset_mask` starts a new episode at its frame instead."""
        mask = self._mask(reset_mask, False)
        self._upload(frames, actions, np.where(mask, self.reset_code, APPEND).astype(np.int32))
        self._push(self._encode(self._frames, self._nhwc))

    @property
    def feature_action(self):
        return self._buf[self._cur][:, :self.P]

    @property
    def features(self):
        return self._buf[self._cur][:, :self.S * self.F].unflatten(1, (self.S, self.F))

    @property
    def actions(self):
        return self._buf[self._cur][:, self.S * self.F:self.P].unflatten(1, (self.S - 1, self.A))

    def input_buffers(self):
        """The two [N, pitch] buffers `feature_action` alternates between (the policy's first layer reads them in place)."""
        return list(self._buf)

    def current(self):
        return self._cur


class SlacActor:
    """The deterministic evaluation policy on a batch of environments: `MakeDeterministic(policy)` over the SLAC observation
    (rollout_functions.py:140-156).  `feature_action`: the policy reads the observation rows.  `latent_z`: the policy reads the
    posterior latent of the window -- `z_[:, -2]` of `prepare_batch`, the latent of the PREVIOUS frame, as the reference feeds it
    (rollout_functions.py:151-152 with algo.py:135; SPEC.md N3f)."""

    def __init__(self, policy, slac_algo, num_envs=1, slac_policy_input_type="feature_action", reset_w_same_obs=False):
        if slac_policy_input_type not in ("feature_action", "latent_z"):
            raise ValueError("slac_policy_input_type %r" % (slac_policy_input_type,))
        if policy.device is None:
            raise RuntimeError("the actor (HIP) needs a policy on a HIP device: there is no CPU fallback")
        self.policy, self.latent, self.input_type, self.N = policy, slac_algo.latent, slac_policy_input_type, int(num_envs)
        if self.N > 16:
            raise ValueError("num_envs <= 16 (s2p_mlp_linear_fwd_skinny)")
        self.ob = SlacObservationBatch(self.N, slac_algo.state_shape, slac_algo.action_shape, slac_algo.num_sequences,
                                       self.latent.encoder, reset_w_same_obs)
        self.A = policy.action_dim
        want = self.ob.P if self.input_type == "feature_action" else Z1 + Z2
        if policy.obs_dim != want:
            raise ValueError("the policy's obs_dim is %d, the %s input has %d columns" % (policy.obs_dim, self.input_type, want))
        dev, f = policy.device, torch.float32
        hs = [torch.empty(self.N, max(policy.hidden_sizes), dtype=f, device=dev) for _ in range(2)]
        self._raw = torch.empty(self.N, 2 * self.A, dtype=f, device=dev)
        self._raw_host = torch.zeros(self.N, 2 * self.A, dtype=f).pin_memory()
        if self.input_type == "feature_action":
            inputs = self.ob.input_buffers()
        else:
            self._z = torch.zeros(self.N, policy.packed.off[0][2], dtype=f, device=dev)
            inputs = [self._z]
        # one table per input buffer; a table holds bare addresses, so the bound nets (and with them every buffer) are kept beside it
        self._nets = [Net("policy", policy.packed, self.N).bind(policy.flat, None, x, self._raw,
                                                               act=[hs[li % 2] for li in range(len(policy.hidden_sizes))]) for x in inputs]
        self._tables = [fwd_tables(fwd_plan([n])) for n in self._nets]

    def reset(self, frames, mask=None):
        self.ob.reset(frames, mask)

    def observe(self, frames, actions, reset_mask=None):
        self.ob.append(frames, actions, reset_mask)

    @torch.no_grad()
    def policy_input(self, noise=None):
        """The rows the policy reads, [N, obs_dim] (a view of the device state)."""
        if self.input_type == "feature_action":
            return self.ob.feature_action
        _, _, z1, z2 = self.latent.sample_posterior(self.ob.features, self.ob.actions, noise)
        self._z[:, :Z1].copy_(z1[:, -2])
        self._z[:, Z1:Z1 + Z2].copy_(z2[:, -2])
        return self._z[:, :Z1 + Z2]

    @torch.no_grad()
    def act(self, noise=None):
        """tanh(mean) for every slot, np.float32 [N, A].  `noise` ([N, S, 288], the eps of the posterior sample) makes a `latent_z`
        step reproducible; without it the eps are drawn on the device."""
        self.policy_input(noise)
        run(self._tables[self.ob.current() if self.input_type == "feature_action" else 0], "s2p_mlp_linear_fwd_skinny")
        self._raw_host.copy_(self._raw, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return np.tanh(self._raw_host.numpy()[:, :self.A])


class ReplayEnv:
    """One trajectory of a dataset (`image_observations`, `rewards`, `terminals` and / or `timeouts`; `image_observations_tp1` if
    the file has it) replayed as an environment: `reset()` hands out its first frame, `step(a)` ignores the action and hands out
    the next frame, the recorded reward and `done` at the trajectory's last transition, with `info["TimeLimit.truncated"]` where
    the dataset marks a timeout that is no terminal.  Trajectories end where `terminals` or `timeouts` is set, and at the last row."""

    def __init__(self, arrays, trajectory=0):
        frames = np.asarray(arrays["image_observations"])
        if frames.ndim == 4 and frames.shape[-1] == 3 and frames.shape[1] != 3:
            frames = frames.transpose(0, 3, 1, 2)                              # NHWC datasets: environments hand out CHW
        T = len(frames)
        zeros = np.zeros(T, dtype=bool)
        term = np.asarray(arrays["terminals"]).reshape(-1).astype(bool) if "terminals" in arrays else zeros
        tout = np.asarray(arrays["timeouts"]).reshape(-1).astype(bool) if "timeouts" in arrays else zeros
        rew = np.asarray(arrays["rewards"], dtype=np.float64).reshape(-1) if "rewards" in arrays else np.zeros(T)
        ends = np.flatnonzero(term | tout).tolist()
        if not ends or ends[-1] != T - 1:
            ends.append(T - 1)
        starts = [0] + [e + 1 for e in ends[:-1]]
        if not 0 <= trajectory < len(ends):
            raise IndexError("trajectory %d of %d" % (trajectory, len(ends)))
        a, b = starts[trajectory], ends[trajectory] + 1
        nxt = np.asarray(arrays["image_observations_tp1"]) if "image_observations_tp1" in arrays else None
        if nxt is not None and nxt.shape[-1] == 3 and nxt.shape[1] != 3:
            nxt = nxt.transpose(0, 3, 1, 2)
        self.frames = np.ascontiguousarray(frames[a:b]).astype(np.uint8)
        # without recorded next frames, the frame after the last transition is the last frame again
        self.next_frames = np.ascontiguousarray(nxt[a:b]).astype(np.uint8) if nxt is not None else \
            np.concatenate([self.frames[1:], self.frames[-1:]])
        self.rewards, self.terminal, self.timeout = rew[a:b], term[a:b], tout[a:b]
        self.num_trajectories, self.t = len(ends), 0

    def __len__(self):
        return len(self.frames)

    def reset(self):
        self.t = 0
        return self.frames[0].copy()

    def step(self, action):
        t = self.t
        if t >= len(self.frames):
            raise RuntimeError("step() past the end of the trajectory: call reset()")
        self.t += 1
        done = t == len(self.frames) - 1
        info = {"TimeLimit.truncated": True} if done and self.timeout[t] and not self.terminal[t] else {}
        return self.next_frames[t].copy(), float(self.rewards[t]), bool(done), info


def run_episodes(envs, actor, episodes, max_path_length):
    """`episodes` evaluation episodes over the environments of `envs`, stepped in lock-step with ONE actor batch per step
    (`actor.reset(frames, mask)`, `actor.observe(frames, actions, reset_mask)`, `actor.act() -> [N, A]`; duck-typed).  A slot whose
    episode ends -- `done`, or `max_path_length` steps -- starts the next episode until `episodes` have been started; then it
    idles (still computed, its action dropped).  -> dict(returns, lengths, terminals [episodes] in completion order, slot order
    within a step; average_return).  `terminals` is `done` without `info["TimeLimit.truncated"]` (rollout_functions.py:184-187)."""
    N = len(envs)
    if N < 1 or episodes < 0 or max_path_length < 1:
        raise ValueError("at least one environment, episodes >= 0 and max_path_length >= 1 are needed")
    returns, lengths, terminals = [], [], []
    active, ret, length, started, frames = [False] * N, [0.0] * N, [0] * N, 0, None
    for i, env in enumerate(envs):
        if started < episodes:
            o = np.asarray(env.reset())
            if frames is None:
                frames = np.zeros((N,) + o.shape, dtype=np.uint8)
            frames[i], active[i], started = o, True, started + 1
    if frames is not None:
        actor.reset(frames.copy(), np.ones(N, dtype=bool))
    while any(active):
        actions = np.asarray(actor.act())
        reset_mask = np.zeros(N, dtype=bool)
        for i, env in enumerate(envs):
            if not active[i]:
                continue
            o, r, done, info = env.step(np.array(actions[i], copy=True))
            ret[i] += float(r)
            length[i] += 1
            if done or length[i] >= max_path_length:
                returns.append(ret[i]); lengths.append(length[i])
                terminals.append(bool(done) and not (info or {}).get("TimeLimit.truncated", False))
                ret[i], length[i] = 0.0, 0
                if started < episodes:
                    o, started, reset_mask[i] = env.reset(), started + 1, True
                else:
                    active[i] = False
            frames[i] = np.asarray(o)
        if any(active):
            actor.observe(frames.copy(), actions, reset_mask)
    returns = np.asarray(returns, dtype=np.float64)
    return dict(returns=returns, lengths=np.asarray(lengths, dtype=np.int64), terminals=np.asarray(terminals, dtype=bool),
                average_return=float(returns.mean()) if len(returns) else float("nan"))
