"""N2c -- the state-transition rollout (s2p_amd/transition_rollout.py, rollout_dynamics.py), host side.  PINNED:
tests/golden/transition_rollout_golden_v1.npz holds what tests/transition_rollout_ref.py (the restatement of
state_transition_rollout.py:105-229) produced with the REAL reference ensemble (tests/golden/make_golden_transition_rollout.py).
The prediction runs on oracle/ensemble_oracle.py in fp32 torch here; the device sweep is tests/test_transition_rollout_gpu.py."""
import os

import numpy as np
import pytest
import torch

import ensemble_oracle as EO
import slac_buffer_ref as SB
import transition_rollout_ref as R
from s2p_amd import transition_rollout as TR

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "transition_rollout_golden_v1.npz"))
E = np.load(os.path.join(HERE, "golden", "ensemble_golden_v1.npz"))
SD = {k[3:]: torch.from_numpy(E[k]) for k in E.files if k.startswith("sd.")}
DATA = {k[3:]: G[k] for k in G.files if k.startswith("in.")}
OUT = {k[4:]: G[k] for k in G.files if k.startswith("out.")}
CFG = {k[4:]: (G[k] if G[k].ndim else float(G[k])) for k in G.files if k.startswith("cfg.")}
LOW, HIGH, SEED = G["act_low"], G["act_high"], int(G["seed"])
PREDICTED = ("next_observations", "rewards", "disagreement_uncertainty", "aleatoric_uncertainty")
N = 31


def close(a, b, tol):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12)) < tol


def oracle_predict(obs, actions, idx, cfg, sd=SD):
    """The whole dataset in one batch (rows do not interact) on the oracle, fp32."""
    x = np.concatenate([(obs - cfg["obs_mean"]) / cfg["obs_std"], actions], axis=1)
    assert x.dtype == np.float32
    mean, std = EO.ensemble_forward(sd, torch.from_numpy(x), obs.shape[1])
    return EO.rollout_postprocess(mean, std, torch.from_numpy(idx).long(), torch.from_numpy(cfg["next_obs_mean"]),
                                  torch.from_numpy(cfg["next_obs_std"]), float(cfg["reward_mean"]), float(cfg["reward_std"]))


def same_schema(out, ref):
    assert set(out) == set(ref), set(out) ^ set(ref)
    for k in ref:
        assert out[k].dtype == ref[k].dtype and out[k].shape == ref[k].shape, (k, out[k].dtype, out[k].shape)


def exact_keys_match(out, ref):
    for k in ref:
        if k not in PREDICTED:
            assert np.array_equal(out[k], ref[k]), k


def test_fixture_is_the_dataset_the_issue_describes():
    starts, ends = TR.trajectories(DATA["timeouts"])
    assert (ends - starts + 1).tolist() == [9, 12, 10] and DATA["observations"].dtype == np.float32
    assert DATA["image_observations"].shape == (N, 2, 2, 3) and DATA["image_observations"].dtype == np.uint8
    assert np.abs(DATA["observations"].mean(0)).min() > 0.01 and np.abs(DATA["observations"].std(0) - 1).min() > 0.01
    assert len(set((HIGH - LOW).tolist())) > 1 and SEED == 7
    regenerated = R.make_dataset()
    assert all(np.array_equal(regenerated[k], DATA[k]) for k in DATA)


def test_trajectories_windows_and_draws_equal_the_fixture():
    starts, ends = TR.trajectories(DATA["timeouts"])
    assert starts.tolist() == [0, 9, 21] and ends.tolist() == [8, 20, 30]
    obs_idx, act_idx = TR.window_indices(starts, ends, 8)
    assert obs_idx.dtype == np.int64 and act_idx.dtype == np.int64
    assert np.array_equal(obs_idx, OUT["slac_observation_indices"]) and np.array_equal(act_idx, OUT["slac_action_indices"])
    assert (obs_idx[:8] == int(1e9)).all() and obs_idx[8].tolist() == list(range(9)) and (obs_idx[9:17] == int(1e9)).all()
    actions, members = TR.draw(starts, ends, LOW, HIGH, 7, SEED)
    assert actions.dtype == np.float32 and members.dtype == np.int64 and members.shape == (N,)
    assert np.array_equal(actions.view(np.uint32), OUT["actions"].view(np.uint32))          # bit for bit
    assert np.array_equal(members, G["ensemble_idx"]) and len(set(members.tolist())) > 3


def test_window_indices_equal_the_buffer_tests_layout():
    starts = np.arange(SB.TRAJ) * SB.ROWS
    obs_idx, act_idx = TR.window_indices(starts, starts + SB.ROWS - 1, SB.S)
    ref_obs, ref_act = SB.slac_indices()
    assert np.array_equal(obs_idx, ref_obs) and np.array_equal(act_idx, ref_act)


def test_generate_on_the_oracle_matches_the_reference_run():
    before = {k: v.copy() for k, v in DATA.items()}
    out = TR.generate(DATA, CFG, act_low=LOW, act_high=HIGH, seed=SEED, predict=oracle_predict)
    same_schema(out, OUT)
    exact_keys_match(out, OUT)
    for k in PREDICTED:
        err = float(np.abs(out[k].astype(np.float64) - OUT[k]).max() / np.abs(OUT[k]).max())
        print(k, "relative-to-max error %.3g" % err)
        assert close(out[k], OUT[k], 1e-6), (k, err)
    assert np.array_equal(out["original_actions"], DATA["actions"]) and np.array_equal(out["original_rewards"], DATA["rewards"])
    assert all(np.array_equal(before[k], DATA[k]) for k in DATA)                             # the input is not modified
    # a wrong member pick would be far outside the tolerance: the members' predictions differ by much more than 1e-6
    other = TR.generate(DATA, CFG, act_low=LOW, act_high=HIGH, seed=SEED,
                        predict=lambda o, a, e, c: oracle_predict(o, a, (e + 1) % 7, c))
    assert not close(other["next_observations"], OUT["next_observations"], 1e-3)


def test_output_is_what_the_downstream_stages_accept():
    from s2p_amd.augment import check_inputs
    from s2p_amd.slac_algo import all_state_windows
    data = dict(DATA, image_observations=np.random.RandomState(0).randint(0, 256, size=(N, 4, 4, 3)).astype(np.uint8))
    out = TR.generate(data, CFG, act_low=LOW, act_high=HIGH, seed=SEED, predict=oracle_predict)
    check_inputs(out, 17)
    out["image_observations_tp1"] = np.zeros_like(out["image_observations"])
    slots, rows, prev = all_state_windows(out, 8)
    assert len(rows) == (9 - 8) + (12 - 8) + (10 - 8) - 1 == 6                               # the last row is a timeout: dropped
    assert rows.tolist() == [8, 17, 18, 19, 20, 29] and slots.shape == (6, 9) and prev.shape == (6, 8)


def test_bad_datasets_are_refused():
    t = np.zeros(20, dtype=bool)
    with pytest.raises(ValueError, match="no timeout"):
        TR.trajectories(t)
    t[9] = True
    with pytest.raises(ValueError, match="follow the last timeout"):
        TR.trajectories(t)
    with pytest.raises(ValueError, match="trajectory 1 has 8 rows"):
        TR.window_indices(np.array([0, 9]), np.array([8, 16]), 8)
    TR.window_indices(np.array([0, 9]), np.array([8, 17]), 8)
    with pytest.raises(ValueError, match="terminal"):
        bad = dict(DATA, terminals=DATA["terminals"].copy())
        bad["terminals"][3] = True
        TR.generate(bad, CFG, predict=oracle_predict)
    with pytest.raises(KeyError, match="timeouts"):
        TR.generate({k: v for k, v in DATA.items() if k != "timeouts"}, CFG, predict=oracle_predict)
    with pytest.raises(ValueError, match="model or a predict"):
        TR.generate(DATA, CFG)


def test_scalar_and_vector_bounds_draw_alike_and_the_global_stream_is_left_alone():
    starts, ends = TR.trajectories(DATA["timeouts"])
    keep = np.random.get_state()                                                             # (put back below: other tests draw from it)
    np.random.seed(123)
    state = np.random.get_state()
    a0, m0 = TR.draw(starts, ends, -1.0, 1.0, 7, 5, action_dim=6)
    a1, m1 = TR.draw(starts, ends, np.full(6, -1.0), np.full(6, 1.0), 7, 5)
    a2, m2 = TR.draw(starts, ends, -1.0, np.full(6, 1.0), 7, 5)
    assert np.array_equal(a0, a1) and np.array_equal(m0, m1) and np.array_equal(a0, a2) and np.array_equal(m0, m2)
    after = np.random.get_state()
    assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    with pytest.raises(ValueError, match="action_dim"):
        TR.draw(starts, ends, -1.0, 1.0, 7, 5)
    # the stream is the reference's: np.random.seed(seed), then per trajectory uniform before randint
    np.random.seed(5)
    ref = [(np.random.uniform(low=-1.0, high=1.0, size=(n, 6)).astype(np.float32), np.random.randint(0, 7, size=n)) for n in (9, 12, 10)]
    np.random.set_state(keep)
    assert np.array_equal(a0, np.concatenate([r[0] for r in ref])) and np.array_equal(m0, np.concatenate([r[1] for r in ref]))


def test_model_sizes_from_a_state_dict():
    assert TR.model_sizes(SD, 17) == dict(obs_dim=17, action_dim=6, hidden_features=64, hidden_layers=3, ensemble_size=7)
    with_saved = dict(SD, **{"backbones.0.saved_weight": SD["backbones.0.weight"]})
    assert TR.model_sizes(with_saved, 17)["hidden_layers"] == 3
    with pytest.raises(ValueError, match="2 \\* \\(obs_dim \\+ 1\\)"):
        TR.model_sizes(SD, 16)
    with pytest.raises(ValueError, match="no room for an action"):
        TR.model_sizes(SD, 23)


def test_command_line_runs_end_to_end_on_an_injected_model(tmp_path, monkeypatch):
    import rollout_dynamics
    a = rollout_dynamics.parse_args("--data d.npz --model_dir m --iter 50 --out o.npz".split())
    assert (a.data, a.model_dir, a.iter, a.out, a.seed, a.action_low, a.action_high, a.num_sequences, a.chunk, a.device) == (
        "d.npz", "m", 50, "o.npz", 0, -1.0, 1.0, 8, 16384, "cuda:0")
    a = rollout_dynamics.parse_args("--data d.npz --model_dir m --iter 5 --out o.npz --action_low -1 -2 --action_high 1 2 --seed 3 "
                                    "--num_sequences 4 --chunk 100 --device cuda:1".split())
    assert (a.action_low, a.action_high, a.seed, a.num_sequences, a.chunk, a.device) == ([-1.0, -2.0], [1.0, 2.0], 3, 4, 100, "cuda:1")

    model_dir = tmp_path / "world_model"
    model_dir.mkdir()
    torch.save(CFG, str(model_dir / "normalize_configs_dict.pkl"))
    torch.save({k: v.clone() for k, v in SD.items()}, str(model_dir / "model_dist_state_dict_3.pkl"))
    np.savez(str(tmp_path / "real.npz"), **DATA)
    built = []

    class Model:
        E = 7

        def rollout_sweep(self, o, a, e, om, os_, nom, nos, rm, rs, chunk):
            built.append(chunk)
            return oracle_predict(o, a, e, dict(obs_mean=om, obs_std=os_, next_obs_mean=nom, next_obs_std=nos, reward_mean=rm, reward_std=rs))

    def build_model(sd, obs_dim, device):
        assert TR.model_sizes(sd, obs_dim)["hidden_features"] == 64 and device == "cuda:0"
        return Model()
    monkeypatch.setattr(TR, "build_model", build_model)
    out_path = str(tmp_path / "gen.npz")
    rollout_dynamics.main(["--data", str(tmp_path / "real.npz"), "--model_dir", str(model_dir), "--iter", "3", "--out", out_path,
                           "--seed", str(SEED), "--action_low"] + [str(v) for v in LOW] + ["--action_high"] + [str(v) for v in HIGH] +
                          ["--chunk", "11"])
    assert built == [11]
    with np.load(out_path) as z:
        written = {k: z[k] for k in z.files}
    same_schema(written, OUT)
    exact_keys_match(written, OUT)
    assert all(close(written[k], OUT[k], 1e-6) for k in PREDICTED)
    # `predict` handed to run(): no model is built at all
    monkeypatch.setattr(TR, "build_model", lambda *a: pytest.fail("a model was built"))
    out = TR.run(str(tmp_path / "real.npz"), str(model_dir), 3, str(tmp_path / "gen2.npz"), LOW, HIGH, SEED, predict=oracle_predict)
    assert np.array_equal(out["next_observations"], written["next_observations"])
