"""State-transition rollout (SPEC.md N2c): the producer of the `all_state_1step_random_action` generated dataset, i.e. the stage
between train_dynamics.py and augment.py.  Restates the reference's `state_transition_rollout.py:59-243` for its only rollout type:
for every row of a real dataset draw one random action and one random ensemble member, run the ensemble, and write the
de-normalised next state and reward of the picked member, the two uncertainties and the SLAC window index tables in the
reference's on-disk schema.

Everything here is numpy on the host except the prediction itself, which is `EnsembleTransition.rollout_sweep` (one device sweep
over the whole dataset) unless a `predict` callable is given.

Out of scope: multi-step rollout types (the loader names `random_state_5step_*`, the reference ships no producer for them),
sharding over ranks, and running the generator in the same process (augment.py is the next stage).
"""
import os

import numpy as np
import torch

INTEGER_INF = int(1e9)
REQUIRED = ("observations", "actions", "rewards", "next_observations", "timeouts")
CFG_KEYS = ("obs_mean", "obs_std", "next_obs_mean", "next_obs_std", "reward_mean", "reward_std")


def trajectories(timeouts):
    """-> (starts, ends) int64, `ends` inclusive (state_transition_rollout.py:74, 151-158): a trajectory ends on a timeout row."""
    t = np.asarray(timeouts).reshape(-1)
    ends = np.sort(np.where(t == 1)[0]).astype(np.int64)
    if len(ends) == 0:
        raise ValueError("the dataset has no timeout: trajectory boundaries are needed (state_transition_rollout.py:75-76)")
    if ends[-1] != len(t) - 1:
        raise ValueError("%d rows follow the last timeout: every row must belong to a trajectory" % (len(t) - 1 - ends[-1]))
    starts = np.concatenate([np.zeros(1, np.int64), ends[:-1] + 1])
    return starts, ends


def window_indices(starts, ends, S=8):
    """-> (obs_idx int64 [N, S+1], act_idx int64 [N, S]) (state_transition_rollout.py:105-132, all trajectories at once): row i of
    a trajectory, i >= S, lists the dataset rows i-S .. i (observations) and i-S .. i-1 (actions); its first S rows hold int(1e9)."""
    starts, ends = np.asarray(starts, np.int64), np.asarray(ends, np.int64)
    lengths = ends - starts + 1
    if (lengths <= S).any():
        k = int(np.argmax(lengths <= S))
        raise ValueError("trajectory %d has %d rows: more than %d are needed (state_transition_rollout.py:106)" % (k, lengths[k], S))
    N = int(lengths.sum())
    row = np.arange(N, dtype=np.int64)
    first = (row - np.repeat(starts, lengths) < S)[:, None]
    obs_idx = np.where(first, INTEGER_INF, row[:, None] + np.arange(-S, 1, dtype=np.int64))
    act_idx = np.where(first, INTEGER_INF, row[:, None] + np.arange(-S, 0, dtype=np.int64))
    return obs_idx, act_idx


def draw(starts, ends, act_low, act_high, n_members, seed, action_dim=None):
    """-> (actions fp32 [N, A], ensemble_idx int64 [N]) from a local RandomState(seed), in the reference's order: per trajectory
    first uniform(low, high, size=(n, A)).astype(float32) (state_transition_rollout.py:175), then randint(0, n_members, size=n)
    (:192) -- the numpy stream `np.random.seed(seed)` gives the reference.  act_low / act_high: a scalar or a length-A array each;
    `action_dim` is needed only when both are scalars."""
    low, high = np.asarray(act_low), np.asarray(act_high)
    A = action_dim
    if A is None:
        if low.ndim == 0 and high.ndim == 0:
            raise ValueError("scalar bounds need action_dim")
        A = max(low.size, high.size)
    low, high = np.broadcast_to(low, (A,)), np.broadcast_to(high, (A,))   # (a scalar and an array of its value draw alike)
    rng = np.random.RandomState(seed)
    actions, members = [], []
    for s, e in zip(np.asarray(starts).tolist(), np.asarray(ends).tolist()):
        n = e - s + 1
        actions.append(rng.uniform(low=low, high=high, size=(n, A)).astype(np.float32))
        members.append(rng.randint(0, n_members, size=n))
    return np.concatenate(actions, 0), np.concatenate(members, 0).astype(np.int64)


def _host(v, shape):
    v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    return np.ascontiguousarray(v, dtype=np.float32).reshape(shape)


def generate(data, cfg, model=None, act_low=-1.0, act_high=1.0, seed=0, S=8, chunk=16384, predict=None, n_members=None):
    """data: the reference's input arrays (state_transition_rollout.py:61-73): `observations`, `actions`, `rewards`,
    `next_observations`, `timeouts`, optionally `terminals` (all zero) and any other key, which passes through untouched on the
    host.  cfg: the normalize_configs_dict.pkl dict.  Returns the reference's dataset dict (:222-229): the input with `actions`
    (drawn), `rewards` [N], `next_observations` [N, obs_dim], `disagreement_uncertainty` / `aleatoric_uncertainty` [N, 1] (fp32)
    and `slac_action_indices` / `slac_observation_indices` (int64) written, the input's actions and rewards kept as
    `original_actions` / `original_rewards`.  predict(observations, actions, ensemble_idx, cfg) -> (next_obs, reward, disagreement,
    aleatoric) replaces the device sweep `model.rollout_sweep`.  The member is drawn among n_members: the model's ensemble size
    by default, the reference's 7 (:192) where there is no model."""
    for k in REQUIRED:
        if k not in data:
            raise KeyError("rollout: the dataset has no '%s' (expected the keys of state_transition_rollout.py:61-73)" % k)
    if "terminals" in data and not (np.asarray(data["terminals"]) == 0).all():
        raise ValueError("the dataset has terminal states: none are assumed (state_transition_rollout.py:78)")
    obs = np.ascontiguousarray(data["observations"], dtype=np.float32)
    if obs.ndim != 2 or np.asarray(data["actions"]).ndim != 2 or len(data["actions"]) != len(obs):
        raise ValueError("observations [N, obs_dim] and actions [N, A] are needed")
    N, A = obs.shape[0], np.asarray(data["actions"]).shape[1]
    starts, ends = trajectories(data["timeouts"])
    if ends[-1] + 1 != N:
        raise ValueError("timeouts has %d rows, observations %d" % (ends[-1] + 1, N))
    obs_idx, act_idx = window_indices(starts, ends, S)
    cfg = {k: np.asarray(cfg[k], dtype=np.float32) for k in CFG_KEYS}
    if predict is None:
        if model is None:
            raise ValueError("generate needs a model or a predict callable")

        def predict(o, a, e, c):
            return model.rollout_sweep(o, a, e, c["obs_mean"], c["obs_std"], c["next_obs_mean"], c["next_obs_std"],
                                       c["reward_mean"], c["reward_std"], chunk=chunk)
    if n_members is None:
        n_members = model.E if model is not None else 7
    actions, members = draw(starts, ends, act_low, act_high, n_members, seed, action_dim=A)
    next_obs, reward, disagreement, aleatoric = predict(obs, actions, members, cfg)
    out = {k: v for k, v in data.items() if k != "actions"}
    out["original_actions"], out["original_rewards"] = data["actions"], data["rewards"]
    out["actions"] = actions
    out["rewards"] = _host(reward, (N,))
    out["next_observations"] = _host(next_obs, (N, obs.shape[1]))
    out["disagreement_uncertainty"] = _host(disagreement, (N, 1))
    out["aleatoric_uncertainty"] = _host(aleatoric, (N, 1))
    out["slac_action_indices"], out["slac_observation_indices"] = act_idx, obs_idx
    return out


def model_sizes(sd, obs_dim):
    """The constructor arguments of the ensemble from a reference state dict's shapes -> dict(obs_dim, action_dim,
    hidden_features, hidden_layers, ensemble_size)."""
    n_hidden = len([k for k in sd if k.startswith("backbones.") and k.endswith(".weight") and "saved" not in k])
    if n_hidden == 0 or "output_layer.weight" not in sd:
        raise ValueError("not an EnsembleTransition state dict: no backbones.*.weight / output_layer.weight")
    E, n_in, hidden = (int(v) for v in sd["backbones.0.weight"].shape)
    if n_in <= obs_dim:
        raise ValueError("the first layer has %d inputs, the observations %d columns: no room for an action" % (n_in, obs_dim))
    if int(sd["output_layer.weight"].shape[2]) != 2 * (obs_dim + 1):
        raise ValueError("the output layer has %d columns, 2 * (obs_dim + 1) = %d are needed" % (
            int(sd["output_layer.weight"].shape[2]), 2 * (obs_dim + 1)))
    return dict(obs_dim=obs_dim, action_dim=n_in - obs_dim, hidden_features=hidden, hidden_layers=n_hidden, ensemble_size=E)


def build_model(sd, obs_dim, device="cuda:0"):
    from .dynamics import EnsembleTransition
    return EnsembleTransition(device=device, **model_sizes(sd, obs_dim)).load_state_dict(sd)


def run(data_path, model_dir, iteration, out_path, act_low=-1.0, act_high=1.0, seed=0, S=8, chunk=16384, device="cuda:0",
        predict=None):
    """Dataset file + the two files train_dynamics.py wrote -> the generated dataset file augment.py reads.  Returns the dict."""
    from .augment import save_arrays
    from .data import load_arrays
    data = load_arrays(data_path)
    cfg = torch.load(os.path.join(model_dir, "normalize_configs_dict.pkl"), map_location="cpu", weights_only=False)
    sd = torch.load(os.path.join(model_dir, "model_dist_state_dict_%d.pkl" % iteration), map_location="cpu", weights_only=False)
    sizes = model_sizes(sd, np.asarray(data["observations"]).shape[1])
    if np.asarray(data["actions"]).shape[1] != sizes["action_dim"]:
        raise ValueError("the dataset's actions have %d columns, the model takes %d" % (np.asarray(data["actions"]).shape[1], sizes["action_dim"]))
    model = build_model(sd, sizes["obs_dim"], device) if predict is None else None
    out = generate(data, cfg, model, act_low, act_high, seed, S, chunk, predict, n_members=sizes["ensemble_size"])
    save_arrays(out_path, out)
    return out
