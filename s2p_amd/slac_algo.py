"""The glue between the datasets and the SLAC latent model (SPEC.md N3c; reference `rlkit/torch/slac/algo.py:12-150` and its offline
loader `:154-416`): a device-resident `ReplayBuffer`, the `LatentModel`, its Adam, `update_latent`, `prepare_batch`, and
`load_data_in_buffer`, which turns a dataset file into window slot tables in vectorised numpy and hands each file to the buffer
in one `load_windows` call (the reference pushes every row through `reset_episode` / `append` in Python)."""
import numpy as np
import torch
from torch.optim import Adam

from .data import load_arrays
from .slac import LatentModel, create_feature_actions
from .slac_buffer import FeatureBatch, ReplayBuffer

INTEGER_INF = int(1e9)                             # `slac_observation_indices` of rows without a full window (rollout.py:111)
SEQUENTIAL_MIX_TYPES = ("random_state_5step_random_action", "random_state_1step_random_action", "random_state_5step_offRL_action")
UNCERTAINTY_TYPES = (None, "aleatoric", "disagreement", "max_of_both", "min_of_both", "average_both")


def uncertainty_penalty(data, uncertainty_type, lam):
    """lambda * u per row, fp32 (algo.py:321-335); u picked by `uncertainty_type`."""
    if uncertainty_type not in UNCERTAINTY_TYPES:
        raise NotImplementedError("uncertainty_type %r" % (uncertainty_type,))
    if uncertainty_type is None:
        return None
    if lam is None:
        raise ValueError("uncertainty_penalty_lambda is needed with an uncertainty_type")

    def arr(k):
        return np.asarray(data[k], dtype=np.float32).reshape(-1)
    if uncertainty_type == "aleatoric":
        return np.float32(lam) * arr("aleatoric_uncertainty")
    if uncertainty_type == "disagreement":
        return np.float32(lam) * arr("disagreement_uncertainty")
    a, d = arr("aleatoric_uncertainty"), arr("disagreement_uncertainty")
    if uncertainty_type == "max_of_both":
        return np.float32(lam) * np.maximum(a, d)
    if uncertainty_type == "min_of_both":
        return np.float32(lam) * np.minimum(a, d)
    return np.float32(lam * 0.5) * (a + d)


def sequential_windows(data, S):
    """Windows of the sequential branch (algo.py:368-407): (slots [W,S+1] into [image_observations | image_observations_tp1],
    rows [W,S] of the transitions of each window)."""
    timeouts = np.asarray(data["timeouts"]).reshape(-1) == 1
    N = len(timeouts)
    n_eff = N - 1 if N and timeouts[N - 1] else N               # a last row that is a timeout is dropped
    i = np.arange(n_eff, dtype=np.int64)
    is_start = np.zeros(n_eff, dtype=bool)
    if n_eff:
        is_start[0] = True
        is_start[1:] = timeouts[:n_eff - 1]
    start = np.maximum.accumulate(np.where(is_start, i, 0))     # first row of the episode of row i
    ends = i[i - start + 1 >= S]                                # the window ending at transition i holds i-S+1 .. i
    rows = ends[:, None] - (S - 1) + np.arange(S, dtype=np.int64)[None, :]
    slots = np.empty((len(ends), S + 1), dtype=np.int64)
    first = rows[:, 0]
    # its first frame: the episode's reset frame when it begins the episode, else the next-frame of the transition before it
    slots[:, 0] = np.where(first == start[ends], first, N + first - 1)
    slots[:, 1:] = N + rows
    return slots, rows


def all_state_windows(data, S):
    """Windows of the `all_state_1step_random_action` branch (algo.py:268-352): (slots [W,S+1], rows i [W], previous rows [W,S])."""
    obs_idx = np.asarray(data["slac_observation_indices"], dtype=np.int64)
    act_idx = np.asarray(data["slac_action_indices"], dtype=np.int64)
    timeouts = np.asarray(data["timeouts"]).reshape(-1) == 1
    N = len(timeouts)
    if obs_idx.shape != (N, S + 1) or act_idx.shape != (N, S) or not (act_idx == obs_idx[:, :-1]).all():
        raise ValueError("slac_observation_indices [N,S+1] / slac_action_indices [N,S] do not match (algo.py:287)")
    bad = obs_idx >= INTEGER_INF
    if (bad.any(axis=1) != bad.all(axis=1)).any():
        raise ValueError("a row's slac_observation_indices are partly invalid (algo.py:289-290)")
    valid = ~bad.any(axis=1)
    if N and timeouts[N - 1]:
        valid[N - 1] = False                                     # a last row that is a timeout is dropped
    i = np.nonzero(valid)[0]
    if len(i) and (i[0] == 0 or obs_idx[i].min() < 0 or obs_idx[i].max() >= N):
        raise IndexError("slac_observation_indices out of range")
    prev = act_idx[i]
    if timeouts[prev].any():
        raise NotImplementedError("a timeout inside a window of the all_state_1step_random_action data (algo.py:314-316)")
    slots = np.empty((len(i), S + 1), dtype=np.int64)
    slots[:, :S] = obs_idx[i, :S]
    slots[:, S] = N + i - 1                                      # the generated frame of row i-1
    return slots, i, prev


class SlacAlgorithm:
    def __init__(self, state_shape, action_shape, action_repeat, device, seed, gamma=0.99, batch_size_sac=256, batch_size_latent=32,
                 buffer_size=10 ** 5, num_sequences=8, lr_sac=3e-4, lr_latent=1e-4, feature_dim=256, z1_dim=32, z2_dim=256,
                 hidden_units=(256, 256), tau=5e-3, image_size=100, use_seperate_buffer=False, dtype=torch.float32,
                 frame_capacity=None, fused_chain=False, fused_chain_grad=False, chain_compute="fp32", chain_grad_compute="fp32"):
        np.random.seed(seed)
        torch.manual_seed(seed)
        torch.cuda.manual_seed(seed)
        self.buffer = ReplayBuffer(buffer_size, num_sequences, state_shape, action_shape, device, dtype=dtype,
                                   frame_capacity=frame_capacity)
        self.use_seperate_buffer = use_seperate_buffer
        if use_seperate_buffer:
            self.buffer_gen = ReplayBuffer(buffer_size, num_sequences, state_shape, action_shape, device, dtype=dtype,
                                           frame_capacity=frame_capacity)
        self.latent = LatentModel(state_shape, action_shape, feature_dim, z1_dim, z2_dim, hidden_units, image_size=image_size,
                                  dtype=dtype, device=device)
        self.latent.fused_chain = bool(fused_chain)         # no-grad posterior chains (prepare_batch, the actor) as one launch each
        self.latent.fused_chain_grad = bool(fused_chain_grad)         # update_latent's chain: one launch forward, one backward
        self.latent.chain_compute = chain_compute            # "bf16": the fused no-grad chains multiply in bf16 (SPEC.md N3m)
        self.latent.chain_grad_compute = chain_grad_compute  # "bf16": update_latent's fused chain multiplies in bf16 (SPEC.md N3p)
        self.target_entropy = -float(action_shape[0])
        self.optim_latent = Adam(self.latent.parameters(), lr=lr_latent)
        self.learning_steps_sac = 0
        self.learning_steps_latent = 0
        self.state_shape = state_shape
        self.action_shape = action_shape
        self.action_repeat = action_repeat
        self.device = device
        self.gamma = gamma
        self.batch_size_sac = batch_size_sac
        self.batch_size_latent = batch_size_latent
        self.num_sequences = num_sequences
        self.tau = tau
        self.create_feature_actions = create_feature_actions

    def update_latent(self, writer=None):
        self.learning_steps_latent += 1
        state_, action_, reward_, done_ = self.buffer.sample_latent(self.batch_size_latent)
        loss_kld, loss_image, loss_reward = self.latent.calculate_loss(state_, action_, reward_, done_)
        self.optim_latent.zero_grad()
        (loss_kld + loss_image + loss_reward).backward()
        self.optim_latent.step()
        return loss_kld, loss_image, loss_reward

    def cache_features(self, chunk=1024):
        """Build the buffers' feature tables from the encoder as it is now (for `freeze_slac` runs; SPEC.md N3g): afterwards
        `buffer.random_batch(..., frames="features")` yields a `FeatureBatch`, on which `prepare_batch` skips the encoder."""
        self.buffer.attach_features(self.latent.encoder, chunk)
        if self.use_seperate_buffer:
            self.buffer_gen.attach_features(self.latent.encoder, chunk)

    def prepare_batch(self, state_, action_, noise=None):
        """`state_`: frames (a FrameBatch or a frame tensor) or a `FeatureBatch`, whose cached features, policy-input rows and last
        action the sampling launch already wrote: only the posterior chain runs.  `noise` is `sample_posterior`'s."""
        cached = isinstance(state_, FeatureBatch)
        with torch.no_grad():
            feature_ = state_.feature_ if cached else self.latent.encoder(state_)                # f(1:t+1)
            z_ = torch.cat(self.latent.sample_posterior(feature_, action_, noise)[2:4], dim=-1)  # z(1:t+1)
        z, next_z = z_[:, -2], z_[:, -1]
        if cached:
            return z, next_z, state_.action, state_.feature_action, state_.next_feature_action
        action = action_[:, -1]
        feature_action, next_feature_action = self.create_feature_actions(feature_, action_)
        return z, next_z, action, feature_action, next_feature_action

    def save_model(self, save_dir):
        self.latent.save_model(save_dir)

    def load_data_in_buffer(self, path_or_arrays, data_num=None, uncertainty_type=None, uncertainty_penalty_lambda=None,
                            generated_for_slac=False, data_mix_type=None):
        """Load one dataset (.npz, .hdf5 with h5py, or a dict of arrays) into the buffer as the reference loader does, both branches
        (SPEC.md N3c).  The frame block handed to the buffer is `image_observations` followed by `image_observations_tp1`."""
        if data_mix_type is not None and data_mix_type != "all_state_1step_random_action" and data_mix_type not in SEQUENTIAL_MIX_TYPES:
            raise NotImplementedError("data_mix_type %r" % (data_mix_type,))
        if uncertainty_type not in UNCERTAINTY_TYPES:
            raise NotImplementedError("uncertainty_type %r" % (uncertainty_type,))
        if data_num == 0:
            return
        data = load_arrays(path_or_arrays) if isinstance(path_or_arrays, str) else dict(path_or_arrays)
        if data_num is not None:
            data = {k: v[:data_num] for k, v in data.items()}
        S = self.num_sequences
        frames = (np.asarray(data["image_observations"]), np.asarray(data["image_observations_tp1"]))
        actions = np.asarray(data["actions"], dtype=np.float32)
        rewards = np.asarray(data["rewards"], dtype=np.float32).reshape(-1)
        if generated_for_slac and data_mix_type == "all_state_1step_random_action":
            buffer = self.buffer_gen if self.use_seperate_buffer else self.buffer
            slots, i, prev = all_state_windows(data, S)
            pen = uncertainty_penalty(data, uncertainty_type, uncertainty_penalty_lambda)
            gen_reward = rewards if pen is None else rewards - pen
            o_act = np.asarray(data["original_actions"], dtype=np.float32)
            o_rew = np.asarray(data["original_rewards"], dtype=np.float32).reshape(-1)
            act = np.concatenate([o_act[prev[:, :S - 1]], actions[i - 1][:, None]], axis=1)
            rew = np.concatenate([o_rew[prev[:, :S - 1]], gen_reward[i - 1][:, None]], axis=1)
        else:
            buffer = self.buffer
            slots, rows = sequential_windows(data, S)
            act, rew = actions[rows], rewards[rows]
        buffer.load_windows(frames, slots, act, rew, np.zeros(rew.shape, dtype=np.float32))      # mask is always False: done_ = 0
        if not generated_for_slac:
            self.buffer._real_n = self.buffer._n
