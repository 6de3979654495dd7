"""`slac_imagine.compare_policies` and select_policy.py: several policies ranked by imagined return from ONE filtering pass on common
random numbers, in both compute modes of the rollout (fp32; bf16 = SPEC.md N3m for the filtering chain + N3n for the rollout)."""
import os

import numpy as np
import pytest
import torch

import slac_buffer_ref as SB
import slac_imagine_ref as IM
from slac_chain_util import count_calls, model_cache

pytestmark = pytest.mark.gpu
Z = 288
CONTEXT, HORIZON = 8, 3
MODES = {"fp32": dict(fused_chain=False, chain_compute="fp32"), "fused": dict(fused_chain=True, chain_compute="fp32"),
         "bf16": dict(fused_chain=True, chain_compute="bf16")}


def _make_policy(W, A, seed=None):
    from s2p_amd.offline_rl import TanhGaussianPolicy
    return TanhGaussianPolicy(hidden_sizes=[W, W], obs_dim=Z, action_dim=A).load_state_dict(IM.make_policy_params(W, A, seed))


def _critic():
    from s2p_amd.offline_rl import CriticSLAC, Qfunction, Vfunction
    hid = [IM.W, IM.W]
    q = [Qfunction(hidden_sizes=hid, output_size=1, input_size=Z + IM.A) for _ in range(4)]
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=hid, output_size=1, input_size=Z))
    sd = critic.state_dict()
    for i, names in enumerate((("qf1", "target_qf1"), ("qf2", "target_qf2"))):
        for n in names:
            sd.update({n + "." + k: v for k, v in IM.make_q_params(i).items()})
    return critic.load_state_dict(sd)


@pytest.fixture(scope="module")
def model(hip_device):
    return model_cache()(SB.A)


@pytest.fixture(scope="module")
def trio(hip_device):
    """Three policies, the first and the last with the same weights; the widths differ."""
    return [_make_policy(256, SB.A), _make_policy(128, SB.A), _make_policy(256, SB.A)]


@pytest.fixture(scope="module")
def real_windows():
    from s2p_amd.slac_predict import gather, windows
    data = SB.real_dataset(2, 12, 100, 100)
    starts = windows(data, CONTEXT + HORIZON, stride=1, limit=3)
    frames, actions, _ = gather(data, starts, CONTEXT)
    return data, starts, frames, actions


def _mode(m, mode, fn):
    for k, v in MODES[mode].items():
        setattr(m, k, v)
    try:
        out = fn("bf16" if mode == "bf16" else "fp32")
        torch.cuda.synchronize()
        return out
    finally:
        m.fused_chain, m.chain_compute = False, "fp32"


@pytest.mark.parametrize("mode", list(MODES))
def test_compare_policies(model, trio, real_windows, mode):
    from s2p_amd.slac_imagine import compare_policies, imagined_returns, paired
    m = model
    _, _, frames, actions = real_windows
    B, A = frames.shape[0], SB.A
    g = torch.Generator().manual_seed(77)
    pn, n = torch.randn(B, CONTEXT + 1, Z, generator=g).cuda(), torch.randn(B, HORIZON, Z, generator=g).cuda()
    critic = _critic()
    # one policy: imagined_returns, bitwise -- with the noise given, and drawn from the same generator state
    for kw in (dict(noise=n, posterior_noise=pn), dict()):
        pair = []
        for fn in (lambda c: imagined_returns(m, trio[0], frames, actions, HORIZON, 0.99, critic, CONTEXT, compute=c, **kw),
                   lambda c: compare_policies(m, trio[:1], frames, actions, HORIZON, 0.99, [critic], CONTEXT, compute=c, **kw)):
            torch.manual_seed(3)
            pair.append(_mode(m, mode, fn))
        one, cp = pair
        assert set(cp) == {"z0", "returns", "actions", "reward_mean", "bootstrap", "value"}
        assert torch.equal(cp["z0"], one["z0"])
        for k in ("returns", "actions", "reward_mean", "bootstrap", "value"):
            assert cp[k].shape == (1,) + one[k].shape and cp[k].dtype == one[k].dtype and torch.equal(cp[k][0], one[k]), (mode, k)
    # three policies: ONE filtering pass (the encoder runs once), a rollout each; equal policies give identical returns
    got = {}

    def three(c):
        got["cp"] = compare_policies(m, trio, frames, actions, HORIZON, 0.99, None, CONTEXT, noise=n, posterior_noise=pn, compute=c)

    def single_policy(c):
        imagined_returns(m, trio[0], frames, actions, HORIZON, 0.99, None, CONTEXT, noise=n, posterior_noise=pn, compute=c)
    calls = {"n": _mode(m, mode, lambda c: count_calls(lambda: three(c)))}
    single = _mode(m, mode, lambda c: count_calls(lambda: single_policy(c)))
    cp = got["cp"]
    rollout = {"fp32": None, "fused": "s2p_imagine_chain_fwd", "bf16": "s2p_imagine_chain_fwd_bf16"}[mode]
    if rollout:
        assert calls["n"][rollout] == 3 and single[rollout] == 1
    conv = [k for k in single if "conv" in k]
    assert conv and all(calls["n"][k] == single[k] for k in conv)                   # the conv stacks ran once, not three times
    assert set(cp) == {"z0", "returns", "actions", "reward_mean"}
    assert cp["returns"].shape == (3, B) and cp["returns"].dtype == torch.float64 and cp["actions"].shape == (3, B, HORIZON, A)
    assert cp["reward_mean"].shape == (3, B, HORIZON) and bool(torch.isfinite(cp["returns"]).all())
    assert torch.equal(cp["returns"][0], cp["returns"][2]) and torch.equal(cp["actions"][0], cp["actions"][2])
    assert not torch.equal(cp["returns"][0], cp["returns"][1])
    s = paired(cp["returns"].cpu().numpy())
    assert abs(int(np.where(s["order"] == 0)[0][0]) - int(np.where(s["order"] == 2)[0][0])) == 1
    assert s["diff_mean"][0] == s["diff_mean"][2] and s["diff_se"][0] == s["diff_se"][2]
    with pytest.raises(ValueError):
        compare_policies(m, [], frames, actions, HORIZON)
    with pytest.raises(ValueError):
        compare_policies(m, trio, frames, actions, HORIZON, critics=[critic])
    with pytest.raises(ValueError, match="fused"):
        compare_policies(m, trio, frames, actions, HORIZON, compute="bf16")          # the model is not in fused mode


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_command_line(model, trio, real_windows, mode, tmp_path, capsys):
    import select_policy
    from s2p_amd.slac_imagine import behaviour, compare_policies, paired
    from s2p_amd.slac_predict import gather
    data, starts, _, _ = real_windows
    path, ldir = str(tmp_path / "real.npz"), str(tmp_path / "latent")
    np.savez(path, **data)
    model.save_model(ldir)
    pdirs = []
    for i, po in enumerate(trio):
        pdirs.append(str(tmp_path / ("policy%d" % i)))
        os.makedirs(pdirs[-1])
        torch.save(po.state_dict(), os.path.join(pdirs[-1], "policy.pth"))
        torch.save(_critic().state_dict(), os.path.join(pdirs[-1], "critic.pth"))
    flags = ["--fused_chain", "--bf16_chain"] if mode == "bf16" else []
    base = ["--data", path, "--latent_dir", ldir, "--policy_dirs"] + pdirs + ["--context", str(CONTEXT), "--horizon", str(HORIZON),
                                                                              "--windows", "3", "--stride", "1", "--batch", "2"] + flags
    res = {}
    for name, more in (("sampled", ["--seed", "4"]), ("mean", ["--mean"])):
        out = str(tmp_path / (name + ".npz"))
        counts = count_calls(lambda: select_policy.main(base + ["--out", out] + more))
        with np.load(out) as f:
            res[name] = {k: f[k] for k in f.files}
        assert ("s2p_imagine_chain_fwd_bf16" in counts) == (mode == "bf16") and ("s2p_posterior_chain_fwd_bf16" in counts) == (mode == "bf16")
    text = capsys.readouterr().out
    assert "to the best" in text and "true reward sum" in text and "model return" in text and text.count("wrote") == 2
    assert all(text.count(d) == 2 for d in pdirs) and ("bf16 rollout" in text) == (mode == "bf16")
    for r in res.values():
        assert set(r) == {"returns", "order", "starts", "policy_dirs", "behaviour_return", "data_return"}
        assert r["returns"].shape == (3, 3) and r["returns"].dtype == np.float64 and np.isfinite(r["returns"]).all()
        assert r["starts"].tolist() == starts.tolist() and r["policy_dirs"].tolist() == pdirs
        assert r["behaviour_return"].shape == r["data_return"].shape == (3,)
        # the equal policies: identical returns, adjacent in the ranking, difference 0 +- 0
        s = paired(r["returns"])
        assert r["order"].tolist() == s["order"].tolist() and sorted(r["order"].tolist()) == [0, 1, 2]
        assert np.array_equal(r["returns"][0], r["returns"][2]) and not np.array_equal(r["returns"][0], r["returns"][1])
        where = {int(p): k for k, p in enumerate(r["order"])}
        assert where[2] == where[0] + 1
        two = paired(r["returns"][[0, 2]])
        assert two["diff_mean"].tolist() == [0.0, 0.0] and two["diff_se"].tolist() == [0.0, 0.0]
    assert not np.array_equal(res["sampled"]["returns"], res["mean"]["returns"])
    # the file holds what the API returns: the mean rollout is a function of its inputs alone
    for k, v in MODES["bf16" if mode == "bf16" else "fp32"].items():
        setattr(model, k, v)
    try:
        rows, be = [], []
        for lo in (0, 2):
            st = starts[lo:lo + 2]
            frames, actions, _ = gather(data, st, CONTEXT)
            rows.append(compare_policies(model, trio, frames, actions, HORIZON, 0.99, None, CONTEXT, sample=False,
                                         compute="bf16" if mode == "bf16" else "fp32")["returns"].cpu().numpy())
            be.append(behaviour(model, data, st, CONTEXT, HORIZON, 0.99, sample=False)["returns"].cpu().numpy())
    finally:
        model.fused_chain, model.chain_compute = False, "fp32"
    assert np.array_equal(np.concatenate(rows, axis=1), res["mean"]["returns"])
    assert np.array_equal(np.concatenate(be), res["mean"]["behaviour_return"])
    # --bootstrap: each directory's critic.pth ends its policy's rollout, and the ranking is by that value
    out = str(tmp_path / "boot.npz")
    select_policy.main(base + ["--out", out, "--mean", "--bootstrap"])
    with np.load(out) as f:
        boot = {k: f[k] for k in f.files}
    assert "return + bootstrap" in capsys.readouterr().out
    assert set(boot) == set(res["mean"]) | {"value"} and np.array_equal(boot["returns"], res["mean"]["returns"])
    assert boot["value"].shape == (3, 3) and np.array_equal(boot["value"][0], boot["value"][2])
    assert not np.array_equal(boot["value"], boot["returns"]) and boot["order"].tolist() == paired(boot["value"])["order"].tolist()
    with pytest.raises(SystemExit, match="actions"):
        bad = str(tmp_path / "other")
        os.makedirs(bad)
        torch.save(_make_policy(128, SB.A + 1).state_dict(), os.path.join(bad, "policy.pth"))
        select_policy.main(["--data", path, "--latent_dir", ldir, "--policy_dirs", pdirs[0], bad, "--out", str(tmp_path / "x.npz"),
                            "--context", str(CONTEXT), "--horizon", str(HORIZON)])
