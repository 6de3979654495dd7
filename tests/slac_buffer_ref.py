"""Seeded datasets and drivers shared by tests/test_slac_buffer.py and tests/golden/make_golden_slac_buffer.py: a small real dataset
and the generated (`all_state_1step_random_action`) dataset made from it, in the on-disk schema of the reference
(`state_transition_rollout.py:105-132,222-243`), and an episode driver for the step-wise `reset_episode` / `append` surface."""
import numpy as np

S, A = 8, 6
H, W, C = 6, 5, 3
TRAJ, ROWS = 3, 14
N = TRAJ * ROWS
INTEGER_INF = int(1e9)
LAMBDA = 0.5
UNCERTAINTY = "max_of_both"
# (name, buffer_size, what is loaded)
SCENARIOS = (("real64", 64, ("real",)), ("gen64", 64, ("gen",)), ("real10", 10, ("real",)), ("gen10", 10, ("gen",)),
             ("mixed64", 64, ("real", "gen")))
FRAME_CAPACITY = 128                      # the episodes here are far shorter than the default capacity assumes
APPEND_EPISODES, APPEND_BUFFER = (11, 9), 3
BATCH_SEED, BATCH = 3, 4


def real_dataset(traj=TRAJ, rows=ROWS, h=H, w=W):
    TRAJ, ROWS, H, W, N = traj, rows, h, w, traj * rows
    r = np.random.RandomState(11)
    frames = r.randint(0, 256, size=(TRAJ, ROWS + 1, H, W, C)).astype(np.uint8)
    frames[0, 0].reshape(-1)[:6] = (0, 1, 127, 128, 254, 255)
    timeouts = np.zeros(N, dtype=bool)
    timeouts[ROWS - 1::ROWS] = True                                   # the last row of each trajectory
    return dict(observations=r.randn(N, 4).astype(np.float32), next_observations=r.randn(N, 4).astype(np.float32),
                actions=r.uniform(-1, 1, (N, A)).astype(np.float32), rewards=r.randn(N).astype(np.float32), timeouts=timeouts,
                image_observations=np.ascontiguousarray(frames[:, :-1].reshape(N, H, W, C)),
                image_observations_tp1=np.ascontiguousarray(frames[:, 1:].reshape(N, H, W, C)))


def slac_indices(traj=TRAJ, rows=ROWS):
    """state_transition_rollout.py:105-132, per trajectory."""
    TRAJ, ROWS, N = traj, rows, traj * rows
    obs = np.full((N, S + 1), INTEGER_INF, dtype=np.int64)
    act = np.full((N, S), INTEGER_INF, dtype=np.int64)
    for t in range(TRAJ):
        for i in range(S, ROWS):
            obs[t * ROWS + i] = np.arange(i - S, i + 1) + t * ROWS
            act[t * ROWS + i] = np.arange(i - S, i) + t * ROWS
    return obs, act


def generated_dataset(traj=TRAJ, rows=ROWS, h=H, w=W):
    H, W, N = h, w, traj * rows
    real = real_dataset(traj, rows, h, w)
    r = np.random.RandomState(12)
    obs, act = slac_indices(traj, rows)
    return dict(observations=real["observations"], next_observations=r.randn(N, 4).astype(np.float32),
                actions=r.uniform(-1, 1, (N, A)).astype(np.float32), rewards=r.randn(N).astype(np.float32), timeouts=real["timeouts"],
                image_observations=real["image_observations"],
                image_observations_tp1=r.randint(0, 256, size=(N, H, W, C)).astype(np.uint8),
                original_actions=real["actions"], original_rewards=real["rewards"],
                slac_observation_indices=obs, slac_action_indices=act,
                aleatoric_uncertainty=r.uniform(0, 2, (N, 1)).astype(np.float32),
                disagreement_uncertainty=r.uniform(0, 2, (N, 1)).astype(np.float32))


DATASETS = dict(real=real_dataset, gen=generated_dataset)
# keyword arguments of load_data_in_buffer per dataset (data_num = N: the reference loader reads the generated keys only then)
LOAD_ARGS = dict(real=dict(data_num=N),
                 gen=dict(data_num=N, uncertainty_type=UNCERTAINTY, uncertainty_penalty_lambda=LAMBDA, generated_for_slac=True,
                          data_mix_type="all_state_1step_random_action"))


def drive_append(buf):
    """Two episodes (11 and 9 steps) of seeded CHW uint8 frames through reset_episode / append."""
    r = np.random.RandomState(13)
    for steps in APPEND_EPISODES:
        buf.reset_episode(r.randint(0, 256, size=(C, H, W)).astype(np.uint8))
        for t in range(steps):
            last = t == steps - 1
            buf.append(r.uniform(-1, 1, A).astype(np.float32), float(r.randn()), False,
                       r.randint(0, 256, size=(C, H, W)).astype(np.uint8), last)
