"""End-to-end runs of the three training scripts of the latent pipeline -- train_latent.py, train_iql.py, train_cql.py -- on a
tiny dataset: what `main` writes against the same steps driven through the API with the same seed, and the empty-buffer exit.

The data: 2 episodes x 12 frames of 100 x 100 x 3 (the smallest frame the latent model builds at) from tests/slac_buffer_ref.py,
and the generated file made from it with window tables for 3-step sequences.  Two runs of one script with one seed write the same
files bit for bit at these shapes (no kernel on these paths accumulates with atomics in an order that varies), and so do the
script and the in-test statement below, which shares nothing with the scripts but the library: hence `torch.equal` throughout."""
import os

import numpy as np
import pytest
import torch

import slac_buffer_ref as SB

pytestmark = pytest.mark.gpu

TRAJ, ROWS, NS, SEED = 2, 12, 3, 0
COMMON = ["--num_sequences", str(NS), "--batch_size", "4", "--batch_size_latent", "2", "--hidden", "64", "--steps", "2", "--log_every", "1"]
LATENT = ["--num_sequences", str(NS), "--batch_size", "4", "--steps", "2", "--log_every", "1"]     # train_latent.py's share of COMMON
CQL_MORE = ["--num_random", "2", "--policy_eval_start", "1"]                        # step 1 clones, step 2 takes the SAC policy loss
FORMS = {"default_gen": [],
         "frozen_cached_fused_bf16_latent_z": ["--freeze_slac", "--cache_features", "--fused_chain", "--bf16_chain", "--bf16_mlp",
                                               "--slac_policy_input_type", "latent_z"]}
FILES = ("critic.pth", "policy.pth", "latent.pth", "encoder.pth")


def _generated(traj, rows, S):
    """SB.generated_dataset with the window tables of S-step sequences (state_transition_rollout.py:105-132, per trajectory)."""
    gen = SB.generated_dataset(traj, rows, 100, 100)
    obs = np.full((traj * rows, S + 1), SB.INTEGER_INF, dtype=np.int64)
    for t in range(traj):
        for i in range(S, rows):
            obs[t * rows + i] = np.arange(i - S, i + 1) + t * rows
    gen["slac_observation_indices"], gen["slac_action_indices"] = obs, np.ascontiguousarray(obs[:, :-1])
    return gen


@pytest.fixture(scope="module")
def files(hip_device, tmp_path_factory):
    d = tmp_path_factory.mktemp("latent_scripts")
    real, gen = SB.real_dataset(TRAJ, ROWS, 100, 100), _generated(TRAJ, ROWS, NS)
    assert real["image_observations"].shape == (TRAJ * ROWS, 100, 100, 3) and real["actions"].shape == (TRAJ * ROWS, SB.A)
    np.savez(str(d / "real.npz"), **real)
    np.savez(str(d / "gen.npz"), **gen)
    return dict(dir=d, real=str(d / "real.npz"), gen=str(d / "gen.npz"))


def _load(path):
    return torch.load(path, map_location="cpu")


def _same_state(got, want, what):
    assert list(got) == list(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k].cpu(), want[k].cpu()), (what, k)


@pytest.fixture(scope="module")
def latent_dirs(files):
    """train_latent.main, per-layer and with --fused_chain_grad -> the two output directories."""
    import train_latent
    out = {}
    for name, more in (("layers", []), ("fused", ["--fused_chain_grad"])):
        out[name] = str(files["dir"] / ("latent_" + name))
        train_latent.main(["--real", files["real"], "--gen", files["gen"], "--out", out[name], "--seed", str(SEED)] + LATENT + more)
    return out


def test_train_latent_writes_a_strict_model_bitwise_in_both_chain_forms(latent_dirs, hip_device):
    from s2p_amd.slac import LatentModel
    sds = {}
    for name, d in latent_dirs.items():
        assert sorted(os.listdir(d)) == ["encoder.pth", "latent.pth"]
        sds[name] = sd = _load(os.path.join(d, "latent.pth"))
        m = LatentModel((3, 100, 100), (SB.A,), device=hip_device)
        m.load_state_dict(sd, strict=True)
        m.encoder.load_state_dict(_load(os.path.join(d, "encoder.pth")), strict=True)
        assert all(bool(torch.isfinite(v).all()) for v in sd.values())
        _same_state(m.state_dict(), sd, name + " reload")
    for f in ("latent.pth", "encoder.pth"):                                                     # train_latent.py: "bit for bit"
        _same_state(_load(os.path.join(latent_dirs["fused"], f)), _load(os.path.join(latent_dirs["layers"], f)), f)


def _by_the_api(kind, flags, files, latent_dir):
    """The steps of train_iql.py / train_cql.py through the API, from the same seed -> (critic, policy, latent, encoder) state."""
    from s2p_amd.cql import CQLTrainer
    from s2p_amd.iql import IQLTrainer
    from s2p_amd.offline_rl import CriticSLAC, Qfunction, TanhGaussianPolicy, Vfunction
    from s2p_amd.slac_algo import SlacAlgorithm
    import train_cql
    import train_iql
    with np.load(files["real"]) as z:
        real = {k: z[k] for k in z.files}
    gen = None
    if "--gen" in flags:
        with np.load(files["gen"]) as z:
            gen = {k: z[k] for k in z.files}
    rows = TRAJ * ROWS * (2 if gen else 1)
    fused, latent_z = "--fused_chain" in flags, "latent_z" in flags
    algo = SlacAlgorithm((3, 100, 100), (SB.A,), 1, "cuda:0", SEED, batch_size_sac=4, batch_size_latent=2, buffer_size=rows,
                         num_sequences=NS, dtype=torch.float32, frame_capacity=2 * rows + NS + 1, fused_chain=fused,
                         fused_chain_grad=False, chain_compute="bf16" if "--bf16_chain" in flags else "fp32")
    algo.latent.load_state_dict(_load(os.path.join(latent_dir, "latent.pth")), strict=True)
    algo.load_data_in_buffer(real)
    if gen is not None:
        algo.load_data_in_buffer(gen, data_num=TRAJ * ROWS, uncertainty_type=None, uncertainty_penalty_lambda=0.0,
                                 generated_for_slac=True, data_mix_type="all_state_1step_random_action")
    assert len(algo.buffer) > 0
    q = [Qfunction(hidden_sizes=[64, 64], output_size=1, input_size=288 + SB.A) for _ in range(4)]
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=[64, 64], output_size=1, input_size=288))
    policy = TanhGaussianPolicy(hidden_sizes=[64, 64], obs_dim=288 if latent_z else NS * 256 + (NS - 1) * SB.A, action_dim=SB.A)
    kw = dict(critic=critic, slac_algo=algo, freeze_slac="--freeze_slac" in flags,
              slac_policy_input_type="latent_z" if latent_z else "feature_action", mlp_compute="bf16" if "--bf16_mlp" in flags else "fp32")
    if kind == "iql":
        trainer = IQLTrainer(None, policy, **kw, **train_iql.IQL_KWARGS)
    else:
        noise = torch.Generator(device="cuda:0").manual_seed(SEED)
        trainer = CQLTrainer(None, policy, num_random=2, min_q_weight=5.0, temp=1.0, policy_eval_start=1, deterministic_backup=False,
                             generator=noise, **kw, **train_cql.CQL_KWARGS)
    frames = None
    if "--cache_features" in flags:
        algo.cache_features()
        frames = "features"
    for _ in range(2):
        trainer.train_from_torch(algo.buffer.random_batch(4, frames=frames))
    torch.cuda.synchronize()
    return {"critic.pth": critic.state_dict(), "policy.pth": policy.state_dict(), "latent.pth": algo.latent.state_dict(),
            "encoder.pth": algo.latent.encoder.state_dict()}


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("kind", ["iql", "cql"])
def test_offline_rl_script_against_the_api(kind, form, files, latent_dirs, capsys):
    mod = __import__("train_" + kind)
    flags = FORMS[form] + (["--gen", files["gen"]] if form == "default_gen" else [])
    out = str(files["dir"] / ("%s_%s" % (kind, form)))
    mod.main(["--real", files["real"], "--latent_dir", latent_dirs["layers"], "--out", out, "--seed", str(SEED)] + COMMON + flags +
             (CQL_MORE if kind == "cql" else []))
    text = capsys.readouterr().out
    assert "step 1 " in text and "step 2 " in text and ("feature table:" in text) == ("--cache_features" in flags)
    assert sorted(os.listdir(out)) == sorted(FILES)
    want = _by_the_api(kind, flags, files, latent_dirs["layers"])
    for f in FILES:
        got = _load(os.path.join(out, f))
        assert all(bool(torch.isfinite(v).all()) for v in got.values()), f
        _same_state(got, want[f], "%s %s %s" % (kind, form, f))
    before = _load(os.path.join(latent_dirs["layers"], "latent.pth"))
    after = _load(os.path.join(out, "latent.pth"))
    if "--freeze_slac" in flags:                                       # a frozen latent model is written as it was read
        _same_state(after, before, "frozen latent.pth")
    else:
        assert any(not torch.equal(after[k], before[k]) for k in before)


@pytest.mark.parametrize("script", ["train_latent", "train_iql", "train_cql"])
def test_no_window_in_the_data_exits(script, files, latent_dirs):
    mod = __import__(script)
    argv = ["--real", files["real"], "--out", str(files["dir"] / "never"), "--steps", "1", "--num_sequences", str(ROWS + 1)]
    if script != "train_latent":
        argv += ["--latent_dir", latent_dirs["layers"], "--hidden", "64"]
    with pytest.raises(SystemExit, match="no window of %d steps in the data" % (ROWS + 1)):
        mod.main(argv)
    assert not os.path.exists(str(files["dir"] / "never"))
