"""TEST INFRASTRUCTURE ONLY: a restatement of the reference's `state_transition_rollout.py:105-229` (rollout type
`all_state_1step_random_action`, normalize 'all', trajectory-wise data for SLAC) with the model handed in as a callable, and the
seeded dataset of tests/golden/transition_rollout_golden_v1.npz.  It keeps what the product vectorises or moves to the device: the
per-trajectory loop, the draws from the GLOBAL numpy stream in the reference's order, the numpy normalisation of the whole dataset
and the torch / numpy post-processing per trajectory.  tests/golden/make_golden_transition_rollout.py runs it with the REAL
`gaussian_ensemble.EnsembleTransition`; tests/tools/bench_transition_rollout.py times it on a device."""
import numpy as np
import torch

S, SEED, N_MEMBERS = 8, 7, 7
LENGTHS = (9, 12, 10)                       # one trajectory of exactly S + 1 rows (a single valid window), unequal lengths
OBS_DIM, ACT_DIM = 17, 6
ACT_LOW = np.array([-1.0, -1.0, -1.0, -0.5, -2.0, -1.0])
ACT_HIGH = np.array([1.0, 1.0, 1.0, 0.5, 2.0, 3.0])
INTEGER_INF = int(1e9)


def make_dataset(frame=2):
    """The real dataset the fixture is generated from: N = 31 rows, fp32 observations with a non-zero mean and a non-unit scale
    per column, a uint8 [N, frame, frame, 3] pass-through key."""
    r = np.random.RandomState(2026)
    n = sum(LENGTHS)
    scale, shift = r.uniform(0.2, 5.0, OBS_DIM), r.uniform(-3.0, 3.0, OBS_DIM)
    obs = (r.randn(n, OBS_DIM) * scale + shift).astype(np.float32)
    timeouts = np.zeros(n, dtype=bool)
    timeouts[np.cumsum(LENGTHS) - 1] = True
    return dict(observations=obs, actions=r.uniform(-1, 1, (n, ACT_DIM)).astype(np.float32),
                rewards=(r.randn(n) * 1.5 + 3.0).astype(np.float32),
                next_observations=(obs + 0.1 * scale * r.randn(n, OBS_DIM)).astype(np.float32),
                terminals=np.zeros(n, dtype=bool), timeouts=timeouts,
                image_observations=r.randint(0, 256, size=(n, frame, frame, 3)).astype(np.uint8))


def window_rows(traj_length, traj_start, num_seq):
    """:105-132 for one trajectory."""
    assert traj_length > num_seq, "traj length : {} slac num seq : {}".format(traj_length, num_seq)
    obs_rows, act_rows = [], []
    for i in range(traj_length):
        if i < num_seq:
            obs_rows.append(np.array([INTEGER_INF] * (num_seq + 1)))
            act_rows.append(np.array([INTEGER_INF] * num_seq))
        else:
            obs_rows.append(np.arange(i - num_seq, i + 1) + traj_start)
            act_rows.append(np.arange(i - num_seq, i) + traj_start)
    obs_idx, act_idx = np.stack(obs_rows, axis=0), np.stack(act_rows, axis=0)
    assert obs_idx.shape == (traj_length, num_seq + 1) and act_idx.shape == (traj_length, num_seq)
    return obs_idx.astype(int), act_idx.astype(int)


def rollout(data, cfg, model, act_low, act_high, seed, num_seq=S, n_members=N_MEMBERS, device="cpu", members_out=None):
    """model(x [B, obs_dim + A] on `device`) -> (mean [E, B, obs_dim + 1], std [E, B, obs_dim + 1]), the `.mean` / `.stddev` of the
    reference's Normal.  Returns the dataset dict of :222-229 (the input arrays are not modified).  Seeds and draws from the global
    numpy stream as the reference does; the stream's previous state is put back afterwards.  members_out: a list that receives the
    member indices drawn per trajectory (the reference does not keep them)."""
    dataset = {k: v for k, v in data.items() if k != "actions"}
    dataset["original_actions"], dataset["original_rewards"] = data["actions"], data["rewards"]
    timeout_rows = np.sort(np.where(data["timeouts"] == 1)[0])
    if len(timeout_rows) == 0:
        raise NotImplementedError
    assert (data["terminals"] == 0).all()
    n_rows, obs_dim, act_dim = data["observations"].shape[0], data["observations"].shape[1], data["actions"].shape[1]
    obs_mean, obs_std = cfg["obs_mean"], cfg["obs_std"]
    next_obs_mean, next_obs_std = cfg["next_obs_mean"], cfg["next_obs_std"]
    reward_mean, reward_std = cfg["reward_mean"], cfg["reward_std"]
    keep = np.random.get_state()
    np.random.seed(seed)
    lists = {k: [] for k in ("actions", "rewards", "next_observations", "disagreement_uncertainty", "aleatoric_uncertainty",
                             "slac_action_indices", "slac_observation_indices")}
    normalized_obs = (data["observations"] - obs_mean) / obs_std
    with torch.no_grad():
        for t, end in enumerate(timeout_rows):
            start = 0 if t == 0 else timeout_rows[t - 1] + 1
            if end >= n_rows:
                raise NotImplementedError
            batch = end - start + 1
            obs_idx, act_idx = window_rows(batch, start, num_seq)
            batch_obs = torch.from_numpy(normalized_obs[start:end + 1]).to(device)
            actions = np.random.uniform(low=act_low, high=act_high, size=(batch, act_dim)).astype(np.float32)
            batch_act = torch.from_numpy(actions).to(device)
            mean, std = model(torch.cat([batch_obs, batch_act], axis=-1))
            predicted_obs, predicted_rew = mean[:, :, :obs_dim], mean[:, :, -1]
            assert mean.shape == (n_members, batch, obs_dim + 1)
            member = np.random.randint(0, n_members, size=batch)
            rows = np.arange(batch)
            if members_out is not None:
                members_out.append(member)
            next_obs = predicted_obs[member, rows].detach().cpu().numpy() * next_obs_std + next_obs_mean
            reward = predicted_rew[member, rows].detach().cpu().numpy() * reward_std + reward_mean
            modes = mean[:, :, :-1]
            diff = modes - torch.mean(modes, dim=0)
            disagreement = torch.max(torch.norm(diff, dim=-1, keepdim=True), dim=0)[0].cpu().numpy()
            aleatoric = torch.max(torch.norm(std, dim=-1, keepdim=True), dim=0)[0].cpu().numpy()
            assert next_obs.shape == (batch, obs_dim) and reward.shape == (batch,)
            for k, v in zip(lists, (actions, reward, next_obs, disagreement, aleatoric, act_idx, obs_idx)):
                lists[k].append(v)
    np.random.set_state(keep)
    for k, v in lists.items():
        dataset[k] = np.concatenate(v, axis=0)
    return dataset
