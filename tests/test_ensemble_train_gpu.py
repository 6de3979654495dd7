"""N2b -- ensemble dynamics training on HIP (s2p_amd/dynamics.py, csrc/ensemble_train.hip).  PINNED parity:
tests/golden/ensemble_train_golden_v1.npz holds fp64 autograd results of the REAL reference module (gaussian_ensemble.py) and
`ref32_err`, the deviation of the reference's own fp32 run from them; shapes the fixture does not hold are checked against
tests/ensemble_train_ref.py run in fp64 and fp32 on the CPU inside the test (its fp32-fp64 deviation is the ref32_err there).

fp32 tolerance of every loss / gradient quantity: K_TOL x max(ref32_err of that quantity, 1e-6), K_TOL = 4 -- the rule, floor and
constant of tests/test_slac_latent.py: the HIP path is the same fp32 arithmetic in another summation order (MFMA k-chunks, rows
summed in row order by one wave, fixed-order LDS reductions in the head).  Forward means / stds: close(..., 1e-5) as in
tests/test_ensemble.py.  Worst observed ratios (deviation / max(ref32_err, 1e-6)) on an MI355X, per group: see DESIGN.md
section 6b.2 (printed by test_zz_report_worst_ratios).

The weight-gradient kernel has no row split at any B (one wave sums all rows of its tile in row order), so B = 300 exercises the
row tail of the 128-row forward / input-gradient tiles and the 16-row unroll tail of the weight gradient, not a second pass."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ensemble_train_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = np.load(os.path.join(HERE, "golden", "ensemble_train_golden_v1.npz"))
SD = {k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("sd.")}
SELECT = [int(i) for i in G["select"]]
K_TOL = 4.0
FLOOR = 1e-6
WORST = {}


def close(a, b, tol):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12)) < tol


def _check(group, err, ref_err, what=""):
    ref = max(float(ref_err), FLOOR)
    WORST[group] = max(WORST.get(group, 0.0), err / ref)
    print("%-22s %-28s err %.3e  ref32_err %.3e  ratio %.3f" % (group, what, err, float(ref_err), err / ref))
    assert err <= K_TOL * ref, (group, what, err, K_TOL * ref)


def _group(name):
    return "head/bounds gradients" if name.endswith("logstd") else ("weight gradients" if name.endswith("weight") else "bias gradients")


def _check_case(out, want, n_hidden, unselected=()):
    """out: loss_and_grad's result; want: name -> (fp64 value, ref32_err) for loss, nll, mse and grad.<name>."""
    loss, nll, mse, grads = out
    ref, err = want["loss"]
    _check("losses", abs(float(loss) - float(ref)) / abs(float(ref)), err, "loss")
    _check("losses", R.rel_max(nll.cpu(), want["nll"][0]), want["nll"][1], "nll per member")
    _check("losses", R.rel_max(mse.cpu(), want["mse"][0]), want["mse"][1], "mse per member")
    names = R.live_names(n_hidden)
    assert sorted(grads) == sorted(names)
    for k in names:
        g = grads[k]
        assert g is not None and float(g.abs().max()) > 0, k                  # no gradient is missing or all-zero
        ref, err = want["grad." + k]
        assert tuple(g.shape) == tuple(np.shape(ref)), k
        _check(_group(k), R.rel_max(g.cpu(), ref), err, k)
        if unselected and g.dim() == 3:
            assert float(g[list(unselected)].abs().max()) == 0.0, k          # exactly zero for unselected members


def _fixture_want(tag):
    keys = ["loss", "nll", "mse"] + ["grad." + k for k in R.live_names(3)]
    return {k: (G[f"{tag}.{k}"], G[f"{tag}.{k}.ref32_err"]) for k in keys}


def _restatement_want(p, x, y, select=None):
    r64, r32 = R.loss_and_grad(p, x, y, select, torch.float64), R.loss_and_grad(p, x, y, select, torch.float32)
    want = {}
    for i, k in enumerate(("loss", "nll", "mse")):
        want[k] = (r64[i].numpy(), R.rel_max(r32[i], r64[i]))
    for k in r64[3]:
        want["grad." + k] = (r64[3][k].numpy(), R.rel_max(r32[3][k], r64[3][k]))
    return want


def _model(sd, obs=17, act=6, hidden=32, E=7):
    from s2p_amd.dynamics import EnsembleTransition
    return EnsembleTransition(obs, act, hidden, 3, ensemble_size=E).load_state_dict(sd)


def test_fixture_parity_3d_input(hip_device):
    m = _model(SD)
    x, y = torch.from_numpy(G["x3"]), torch.from_numpy(G["y3"])
    mean, std = m(x)
    assert mean.shape == (7, 37, 18) and close(mean.cpu(), G["c3.mean"], 1e-5) and close(std.cpu(), G["c3.std"], 1e-5)
    _check_case(m.loss_and_grad(x, y), _fixture_want("c3"), 3)


def test_fixture_parity_2d_shared_input_and_selection(hip_device):
    m = _model(SD)
    x, y = torch.from_numpy(G["x3"]), torch.from_numpy(G["y3"])
    mean, std = m(x[1])                                     # the existing [B, in] forward
    assert mean.shape == (7, 37, 18) and close(mean.cpu(), G["c2.mean"], 1e-5) and close(std.cpu(), G["c2.std"], 1e-5)
    _check_case(m.loss_and_grad(x[1], y[1]), _fixture_want("c2"), 3)
    m.set_select(SELECT)
    mean, std = m(x[SELECT])
    assert mean.shape == (5, 37, 18) and close(mean.cpu(), G["sel.mean"], 1e-5) and close(std.cpu(), G["sel.std"], 1e-5)
    out = m.loss_and_grad(x[SELECT], y[SELECT])
    assert out[1].shape == (5,) and out[2].shape == (5,)
    _check_case(out, _fixture_want("sel"), 3, unselected=[e for e in range(7) if e not in SELECT])
    mean2, _ = m(x[1])                                      # a shared input over the selected members
    assert mean2.shape == (5, 37, 18) and close(mean2.cpu(), G["c2.mean"][SELECT], 1e-5)


@pytest.mark.parametrize("B,hidden,E", [(1, 32, 7), (300, 64, 7), (33, 32, 1), (40, 32, 8)])
def test_edges_against_the_restatement(hip_device, B, hidden, E):
    p = R.make_params(100 + B, E, 23, hidden, 3, 18)
    g = torch.Generator().manual_seed(B)
    x = torch.randn(E, B, 23, generator=g)
    x[:, 0] *= 10.0
    y = x[..., :18] * 0.9 + 0.3 * torch.randn(E, B, 18, generator=g)
    m = _model(p, hidden=hidden, E=E)
    _check_case(m.loss_and_grad(x, y), _restatement_want(p, x, y), 3)
    mu, ls = R.forward({k: v.double() for k, v in p.items()}, x.double())
    mean, std = m(x)
    assert close(mean.cpu(), mu, 1e-5) and close(std.cpu(), ls.exp(), 1e-5)


def _full_size_params():
    g = torch.Generator().manual_seed(3)                    # as test_hip_ensemble_full_size_matches_oracle
    E, H = 7, 256
    sd = {}
    for i, (a, b) in enumerate([(23, H), (H, H), (H, H)]):
        sd[f"backbones.{i}.weight"] = torch.randn(E, a, b, generator=g) / (2 * a ** 0.5)
        sd[f"backbones.{i}.bias"] = torch.randn(E, 1, b, generator=g) * 0.1
    sd["output_layer.weight"] = torch.randn(E, H, 36, generator=g) / (2 * H ** 0.5)
    sd["output_layer.bias"] = torch.randn(E, 1, 36, generator=g) * 0.1
    sd["max_logstd"] = torch.ones(18); sd["min_logstd"] = -5 * torch.ones(18)
    return sd, g


def test_reference_configuration(hip_device):
    sd, g = _full_size_params()
    x = torch.randn(7, 256, 23, generator=g)
    y = x[..., :18] + 0.3 * torch.randn(7, 256, 18, generator=g)
    _check_case(_model(sd, hidden=256).loss_and_grad(x, y), _restatement_want(sd, x, y), 3)


def test_two_calls_are_bitwise_identical(hip_device):
    m = _model(SD)
    x, y = torch.from_numpy(G["x3"]), torch.from_numpy(G["y3"])
    a, b = m.loss_and_grad(x, y), m.loss_and_grad(x, y)
    for u, v in zip(a[:3], b[:3]):
        assert torch.equal(u, v)
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


def test_one_optimizer_step_is_wired_to_the_gradients(hip_device):
    from s2p_amd.dynamics import EnsembleTrainer
    m = _model(SD)
    x, y = torch.from_numpy(G["x3"]), torch.from_numpy(G["y3"])
    names = R.live_names(3)
    before = m.state_dict()
    pt = {k: before[k].clone().requires_grad_(True) for k in names}
    opt = torch.optim.Adam([pt[k] for k in names], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    tr = EnsembleTrainer(m)
    for step in (1, 2):
        grads = m.loss_and_grad(x, y)[3]
        for k in names:
            pt[k].grad = grads[k].cpu().clone()
        opt.step()
        tr.train_step(x, y)
        after = m.state_dict()
        assert int(tr.step.item()) == step
        for k in names:
            assert R.rel_max(after[k], pt[k].detach()) < 1e-5, (step, k)          # the tolerance of test_posenc_losses_adam
            moved = (after[k] - before[k]).abs().max()
            assert 0.5e-3 * step < float(moved) < 1.5e-3 * step, (step, k, float(moved))   # |Adam update| ~ lr per step on a constant batch
        for k in after:
            if "saved" in k:
                assert torch.equal(after[k], before[k]), k


def test_training_follows_the_fp64_trajectory(hip_device):
    from s2p_amd.dynamics import EnsembleTrainer, EnsembleTransition
    c = R.SYS
    p, xs, ys, xh, yh = R.training_problem()
    m = EnsembleTransition(c["obs"], c["act"], c["hidden"], c["n_hidden"], ensemble_size=c["E"]).load_state_dict(p)
    tr = EnsembleTrainer(m)
    first = tr.evaluate(xh, yh).cpu()
    assert R.rel_max(first, G["traj.holdout_mse_initial"]) < 1e-5
    for x, y in zip(xs, ys):
        loss = tr.train_step(x, y)[0]
    last = tr.evaluate(xh, yh).cpu()
    assert bool((last < first).all()), (first, last)                              # every member improved on the holdout rows
    want = float(G["traj.losses"][-1])
    err = abs(float(loss) - want) / abs(want)
    tol = K_TOL * max(float(G["traj.final_loss.ref32_err"]), 1e-5)
    print("final loss", float(loss), "fp64 restatement", want, "rel err %.3e tol %.3e" % (err, tol))
    assert err <= tol, (err, tol)


def test_fit_bookkeeping(hip_device):
    from s2p_amd.dynamics import EnsembleTrainer, EnsembleTransition
    X, Y = R.synthetic_system(400, 5, 5, 2)
    m = EnsembleTransition(5, 2, 32, 3, ensemble_size=7).init_parameters(seed=1)
    sd0 = m.state_dict()
    assert list(sd0) == [str(k) for k in G["state_dict_names"]]
    for k in sd0:
        if "saved" in k:
            assert torch.equal(sd0[k], sd0[k.replace("saved_", "")])
    w0 = sd0["backbones.0.weight"]
    assert float(w0.abs().max()) <= 2.0 + 1e-6 and abs(float(w0.std()) - 1 / (2 * 7 ** 0.5)) < 0.02 and float(sd0["output_layer.bias"].abs().max()) == 0
    tr = EnsembleTrainer(m, lr=1e-3)
    saves = []
    orig = m.update_save
    m.update_save = lambda idx: (saves.append(list(idx)), orig(idx))[1]
    info = tr.fit(X, Y, epochs=2, batch_size=64, holdout=60, n_elite=5, seed=3)
    # update_save fired for all members at the start, then exactly for the members whose holdout MSE improved on their best
    best, want_calls = info["initial_mse"].clone(), [list(range(7))]
    assert len(info["epoch_mse"]) == 2
    for mse, saved in zip(info["epoch_mse"], info["saved"]):
        want = [e for e in range(7) if float(mse[e]) < float(best[e])]
        assert saved == want
        if want:
            want_calls.append(want)
            best[want] = mse[want]
    assert saves == want_calls and len(saves) > 1            # (training on this system does improve somebody)
    assert torch.equal(best, info["holdout_mse"]) and info["elites"] == sorted(torch.argsort(best)[:5].tolist())
    assert len(m.select) == 5 and m.select == info["elites"] and len(set(m.select)) == 5
    sd = m.state_dict()
    for k in sd:                                            # the selected members were restored from their saved copies
        if "saved" in k:
            assert torch.equal(sd[k][m.select], sd[k.replace("saved_", "")][m.select]), k
    m2 = EnsembleTransition(5, 2, 32, 3, ensemble_size=7).load_state_dict(sd)
    sd2 = m2.state_dict()
    assert list(sd2) == list(sd)
    for k in sd:
        assert sd2[k].dtype == torch.float32 and torch.equal(sd2[k], sd[k]), k


def test_cli_writes_the_two_files_stage_a_loads(hip_device, tmp_path):
    from s2p_amd.dynamics import EnsembleTransition
    X, Y = R.synthetic_system(300, 7, 17, 6)
    rng = np.random.default_rng(0)
    np.savez(tmp_path / "data.npz", observations=X[:, :17].numpy() * 2 + 1, actions=X[:, 17:].numpy(),
             next_observations=Y[:, :17].numpy() * 2 + 1, rewards=Y[:, 17].numpy() * 3 + rng.normal(size=300).astype(np.float32))
    out = tmp_path / "wm"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_dynamics.py"), "--data", str(tmp_path / "data.npz"), "--out", str(out),
                        "--epochs", "1", "--hidden_features", "32", "--batch_size", "64", "--seed", "0"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    cfg = torch.load(out / "normalize_configs_dict.pkl", weights_only=False)      # (as state_transition_rollout.py:89 loads it)
    assert sorted(cfg) == sorted(["obs_mean", "obs_std", "next_obs_mean", "next_obs_std", "reward_mean", "reward_std"])
    sd = torch.load(out / "model_dist_state_dict_1.pkl", map_location="cpu")
    assert list(sd) == [str(k) for k in G["state_dict_names"]]
    for k, shape in zip(sd, G["state_dict_shapes"]):
        assert isinstance(sd[k], torch.Tensor) and sd[k].dtype == torch.float32 and not sd[k].is_cuda
        assert ",".join(map(str, sd[k].shape)) == str(shape), k
    m = EnsembleTransition(17, 6, 32, 3, ensemble_size=7).load_state_dict(sd)
    xin = (torch.from_numpy(np.concatenate([(X[:8, :17].numpy() * 2 + 1 - cfg["obs_mean"]) / cfg["obs_std"], X[:8, 17:].numpy()], 1))).float()
    nobs, rew, dis, ale = m.rollout_step(xin, np.zeros(8, np.int32), cfg["next_obs_mean"], cfg["next_obs_std"],
                                         float(cfg["reward_mean"]), float(cfg["reward_std"]))
    assert nobs.shape == (8, 17) and rew.shape == (8,) and bool(torch.isfinite(nobs).all()) and bool(torch.isfinite(dis).all())


def test_zz_report_worst_ratios(hip_device):
    print("\nworst deviation / max(ref32_err, 1e-6) per group:", {k: round(v, 3) for k, v in WORST.items()})
    assert WORST and max(WORST.values()) <= K_TOL
