"""N3o -- closed-loop imagination of a `feature_action` policy: `LatentModel.imagine_feature_action` (policy -> prior step -> decoder ->
s2p_decoded_to_frames -> encoder -> s2p_feature_action_push per step), `slac_imagine.imagined_returns` / `compare_policies` with such
a policy, imagine_policy.py and select_policy.py.

The structural checks are BITWISE (torch.equal): every row the policy read is returned, so each action is `policy.act` of its row,
each window is the one before shifted by one feature and one action, the new feature is the encoder's answer -- at the same batch
size -- to the replay buffer's gather of the returned uint8 frame, and the latents are `predict`'s under the returned actions.  B 3 and
17 (17 crosses the 16-row forms of `policy.act` and leaves one row to the push's second block row), H 3, S 8, A 6, policy [128, 128].
The toleranced checks against the recorded run of the reference's modules (tests/golden/slac_imagine_fa_golden_v1.npz) use the
project's rule per step: err(h) <= K_TOL x max(ref32_err(h), 1e-6), K_TOL = 4."""
import os
import types

import numpy as np
import pytest
import torch

import slac_buffer_ref as SB
import slac_imagine_fa_ref as FA
import slac_imagine_ref as IR
from slac_chain_util import build_model, model_cache

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
K_TOL, FLOOR = 4.0, 1e-6
Z1, Z, F, S, A, P, H = 32, 288, 256, FA.S, FA.A, FA.OBS, 3
NF = S * F                                                               # feature columns of a window


def _fa_policy(sd=None, hidden=(FA.W, FA.W), obs_dim=P, a=A):
    from s2p_amd.offline_rl import TanhGaussianPolicy
    po = TanhGaussianPolicy(hidden_sizes=list(hidden), obs_dim=obs_dim, action_dim=a)
    return po.load_state_dict(sd) if sd is not None else po


def _z_policy(W=128):
    from s2p_amd.offline_rl import TanhGaussianPolicy
    return TanhGaussianPolicy(hidden_sizes=[W, W], obs_dim=Z, action_dim=A).load_state_dict(IR.make_policy_params(W, A))


def _critic():
    from s2p_amd.offline_rl import CriticSLAC, Qfunction, Vfunction
    hid = [IR.W, IR.W]
    q = [Qfunction(hidden_sizes=hid, output_size=1, input_size=Z + A) for _ in range(4)]
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=hid, output_size=1, input_size=Z))
    sd = critic.state_dict()
    for i, names in enumerate((("qf1", "target_qf1"), ("qf2", "target_qf2"))):
        for n in names:
            sd.update({n + "." + k: v for k, v in IR.make_q_params(i).items()})
    return critic.load_state_dict(sd)


@pytest.fixture(scope="module")
def model(hip_device):
    return model_cache()(A)


@pytest.fixture(scope="module")
def policy(hip_device):
    return _fa_policy(FA.make_policy_params())


def _inputs(B):
    z0, noise = FA.make_inputs(B, H)
    return z0.cuda(), FA.make_window(B).cuda(), noise.cuda()


def _run(m, po, z0, window, noise=None, **kw):
    with torch.enable_grad():                                            # the method itself must switch grad off
        out = m.imagine_feature_action(po, z0, window, kw.pop("H", H), noise, **kw)
    torch.cuda.synchronize()
    assert all(t is None or (t.grad_fn is None and not t.requires_grad) for t in out)
    return [t.clone() if t is not None else None for t in out]


def _gathered_features(m, frames_u8):
    """The encoder's features, at the batch size of frames_u8 [B,100,100,3], of those frames as the replay buffer hands them over:
    s2p_window_gather_u8 over a pool that holds each frame once."""
    from s2p_amd import ops
    B = frames_u8.shape[0]
    table = torch.arange(B, dtype=torch.int32, device="cuda").reshape(B, 1)
    win = torch.arange(B, dtype=torch.int64, device="cuda")
    x, _ = ops.window_gather_u8(frames_u8.contiguous(), table, win, m.encoder.dtype, want_u8=False)
    with torch.no_grad():
        return m.encoder.run(x).reshape(B, -1).float()


def _check_structure(m, po, B, quantize=True):
    z0, window, noise = _inputs(B)
    act, mean, std, z, obs, frames = _run(m, po, z0, window, noise, quantize=quantize, keep_frames=True)
    assert act.shape == (B, H, A) and mean.shape == std.shape == (B, H, Z1) and z.shape == (B, H, Z) and obs.shape == (B, H, P)
    assert frames.dtype == torch.uint8 and frames.shape == (B, H - 1, 100, 100, 3)
    assert all(bool(torch.isfinite(t).all()) for t in (act, mean, std, z, obs)) and float(act.abs().max()) > 0.3
    assert torch.equal(obs[:, 0], window)
    for h in range(H):
        assert torch.equal(act[:, h], po.act(obs[:, h].contiguous())), h
    for h in range(H - 1):
        a, b = obs[:, h], obs[:, h + 1]
        assert torch.equal(b[:, :NF - F], a[:, F:NF]) and torch.equal(b[:, NF:P - A], a[:, NF + A:]), h
        assert torch.equal(b[:, P - A:], act[:, h]), h
        if quantize:                                                     # the encoder saw exactly the returned uint8 frame
            assert torch.equal(b[:, NF - F:NF], _gathered_features(m, frames[:, h])), h
        assert len(torch.unique(frames[:, h])) > 4                       # a picture, not a constant
    for got, want in zip(m.predict(z0, act, noise), (mean, std, z)):
        assert torch.equal(got, want)
    return z0, window, noise, (act, mean, std, z, obs, frames)


@pytest.mark.parametrize("B", [3, 17])
def test_every_step_is_what_its_pieces_compute(model, policy, B):
    z0, window, noise, first = _check_structure(model, policy, B)
    again = _run(model, policy, z0, window, noise, keep_frames=True)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    # final_obs adds window(H) and the frame behind it, and changes nothing else
    fin = _run(model, policy, z0, window, noise, final_obs=True, keep_frames=True)
    assert fin[4].shape == (B, H + 1, P) and fin[5].shape == (B, H, 100, 100, 3)
    assert all(torch.equal(a, b) for a, b in zip(first[:4], fin[:4])) and torch.equal(fin[4][:, :H], first[4])
    assert torch.equal(fin[5][:, :H - 1], first[5])
    assert torch.equal(fin[4][:, H, NF - F:NF], _gathered_features(model, fin[5][:, H - 1]))
    assert torch.equal(fin[4][:, H, P - A:], first[0][:, H - 1])
    # without keep_frames: no frames, the same numbers
    bare = _run(model, policy, z0, window, noise)
    assert bare[5] is None and all(torch.equal(a, b) for a, b in zip(first[:5], bare[:5]))
    # sample False: zero noise, whatever is passed
    mean = _run(model, policy, z0, window, noise, sample=False)
    zero = _run(model, policy, z0, window, torch.zeros_like(noise))
    none = _run(model, policy, z0, window, None, sample=False)
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(mean[:5], zero[:5], none[:5]))
    assert not torch.equal(mean[3], first[3])


def test_clamp_only_mode(model, policy):
    """quantize False: the same first step (window(0), a(0), z(1)), so the same first uint8 frame; the encoder then sees the float
    frame, so window(1)'s new feature is another one."""
    z0, window, noise, q = _check_structure(model, policy, 3)
    _, _, _, c = _check_structure(model, policy, 3, quantize=False)
    assert torch.equal(c[0][:, 0], q[0][:, 0]) and torch.equal(c[3][:, 0], q[3][:, 0]) and torch.equal(c[5][:, 0], q[5][:, 0])
    fq, fc = q[4][:, 1, NF - F:NF], c[4][:, 1, NF - F:NF]
    assert not torch.equal(fq, fc) and bool(torch.isfinite(fc).all())


def test_bf16_stacks(hip_device, policy):
    m = build_model(A, torch.bfloat16)
    _check_structure(m, policy, 3)


def test_refusals(model, policy):
    m, po = model, policy
    z0, window, noise = _inputs(3)
    bad_policies = [_fa_policy(obs_dim=P + 1), _fa_policy(obs_dim=F), _z_policy(), _fa_policy(obs_dim=S * F + (S - 1) * 1, a=1),
                    _fa_policy(hidden=(128, 128, 128)), types.SimpleNamespace(obs_dim=P, action_dim=A, hidden_sizes=[128, 128], device=None)]
    for bad in bad_policies:
        with pytest.raises(ValueError):
            m.imagine_feature_action(bad, z0, window, H, noise)
    for kw in (dict(window=window[:, :P - 1]), dict(window=window[:2]), dict(z0=z0[:, :Z - 1]), dict(noise=noise[:, :2]), dict(H=-1)):
        a = dict(z0=z0, window=window, noise=noise, H=H)
        a.update(kw)
        with pytest.raises(ValueError):
            m.imagine_feature_action(po, a["z0"], a["window"], a["H"], a["noise"])
    big = 65536                                                          # one row more than s2p_feature_action_push takes
    with pytest.raises(ValueError, match="65535"):
        m.imagine_feature_action(po, torch.zeros(big, Z, device="cuda"), torch.zeros(big, P, device="cuda"), 0)
    # `imagine` still refuses the policy, as tests/test_latent_imagine_gpu.py expects of a policy that is no latent_z one
    with pytest.raises(ValueError):
        m.imagine(po, z0, 2)
    empty = _run(m, po, z0, window, None, H=0, final_obs=True, keep_frames=True)
    assert [tuple(t.shape) for t in empty] == [(3, 0, A), (3, 0, Z1), (3, 0, Z1), (3, 0, Z), (3, 1, P), (3, 0, 100, 100, 3)]
    assert torch.equal(empty[4][:, 0], window)


# ---- imagined_returns and compare_policies ----------------------------------------------------------------------------------------------
CONTEXT = 8


@pytest.fixture(scope="module")
def real_windows():
    from s2p_amd.slac_predict import gather, windows
    data = SB.real_dataset(2, 12, 100, 100)
    starts = windows(data, CONTEXT + H, stride=1, limit=3)
    frames, actions, _ = gather(data, starts, CONTEXT)
    return data, starts, frames, actions


def _noises(B):
    g = torch.Generator().manual_seed(78)
    return torch.randn(B, CONTEXT + 1, Z, generator=g).cuda(), torch.randn(B, H, Z, generator=g).cuda()


def test_imagined_returns_and_compare_policies(model, policy, real_windows):
    from s2p_amd.slac_imagine import compare_policies, compare_rollouts, imagined_returns
    m, pfa, pz, critic = model, policy, _z_policy(), _critic()
    _, _, frames, actions = real_windows
    B = frames.shape[0]
    pn, n = _noises(B)
    kw = dict(noise=n, posterior_noise=pn)
    # a latent_z policy: what it gave before, i.e. `imagine` from the filtered start state
    oz = imagined_returns(m, pz, frames, actions, H, 0.99, critic, CONTEXT, **kw)
    want = m.imagine(pz, oz["z0"], H, n)
    assert "obs" not in oz and all(torch.equal(oz[k], w) for k, w in zip(("actions", "z1_mean", "z1_std", "z"), want))
    zH = oz["z"][:, -1].contiguous()
    assert torch.equal(oz["bootstrap"], critic.q_min(zH, pz.act(zH)))
    # a feature_action policy: window(0) is cut from the context, the rollout is imagine_feature_action's, the bootstrap reads window(H)
    of = imagined_returns(m, pfa, frames, actions, H, 0.99, critic, CONTEXT, keep_frames=True, **kw)
    assert torch.equal(of["z0"], oz["z0"]) and of["obs"].shape == (B, H + 1, P) and of["frames_u8"].shape == (B, H, 100, 100, 3)
    feat = m.encoder(torch.as_tensor(frames[:, :CONTEXT + 1]).cuda())
    acts = torch.as_tensor(actions).cuda()
    w0 = torch.cat([feat[:, CONTEXT + 1 - S:].reshape(B, -1), acts[:, CONTEXT - (S - 1):CONTEXT].reshape(B, -1)], dim=1)
    assert torch.equal(of["obs"][:, 0], w0)
    direct = m.imagine_feature_action(pfa, of["z0"], w0, H, n, final_obs=True)
    assert all(torch.equal(of[k], d) for k, d in zip(("actions", "z1_mean", "z1_std", "z", "obs"), direct))
    zH = of["z"][:, -1].contiguous()
    assert torch.equal(of["bootstrap"], critic.q_min(zH, pfa.act(of["obs"][:, H].contiguous())))
    assert not torch.equal(of["bootstrap"], critic.q_min(zH, pfa.act(of["obs"][:, H - 1].contiguous())))
    assert torch.equal(of["value"], of["returns"] + 0.99 ** H * of["bootstrap"].double())
    rm, _ = m.predict_reward(of["z0"], of["z"], of["actions"])
    assert torch.equal(of["reward_mean"], rm) and bool(torch.isfinite(of["returns"]).all())
    # without a critic the rollout stops at window(H-1)
    nf = imagined_returns(m, pfa, frames, actions, H, 0.99, None, CONTEXT, **kw)
    assert nf["obs"].shape == (B, H, P) and "frames_u8" not in nf and torch.equal(nf["returns"], of["returns"])
    # one feature_action policy: compare_policies is imagined_returns
    one = compare_policies(m, [pfa], frames, actions, H, 0.99, [critic], CONTEXT, **kw)
    for k in ("returns", "actions", "reward_mean", "bootstrap", "value"):
        assert torch.equal(one[k][0], of[k]), k
    # a mixed pair shares z0 and the noise: each row is that policy's own imagined_returns
    cp = compare_rollouts(m, [pz, pfa], frames, actions, H, 0.99, [critic, critic], CONTEXT, keep_frames=True, **kw)
    assert torch.equal(cp["z0"], oz["z0"]) and cp["returns"].shape == (2, B)
    for k in ("returns", "actions", "reward_mean", "bootstrap", "value"):
        assert torch.equal(cp[k][0], oz[k]) and torch.equal(cp[k][1], of[k]), k
    assert cp["frames_u8"][0] is None and torch.equal(cp["frames_u8"][1], of["frames_u8"])
    # quantize passes through
    fl = imagined_returns(m, pfa, frames, actions, H, 0.99, None, CONTEXT, quantize=False, **kw)
    assert torch.equal(fl["obs"][:, 0], nf["obs"][:, 0]) and not torch.equal(fl["obs"][:, 1], nf["obs"][:, 1])
    with pytest.raises(ValueError, match="context"):
        imagined_returns(m, pfa, frames[:, :7], actions[:, :6], H, context=6)
    with pytest.raises(ValueError, match="bf16"):
        imagined_returns(m, pfa, frames, actions, H, context=CONTEXT, compute="bf16")
    with pytest.raises(ValueError, match="bf16"):
        compare_policies(m, [pz, pfa], frames, actions, H, context=CONTEXT, compute="bf16")
    with pytest.raises(ValueError, match="feature_action"):
        imagined_returns(m, _fa_policy(obs_dim=P + 1), frames, actions, H, context=CONTEXT)


# ---- reference parity ---------------------------------------------------------------------------------------------------------------------
def test_pinned_parity(model, policy, capsys):
    """Clamp-only mode against the recorded fp64 run of the reference's modules, per step with that step's ref32_err; quantised mode:
    every pixel of our step-0 frames within one level of the fp64 run's.
    Measured on an MI355X (worst deviation over the steps / max(ref32_err, 1e-6); the bound is K_TOL = 4): 0.892523 (mean rollout's
    z1_mean and z; sampled: actions 0.571, z1_mean 0.478, z1_std 0.340, z 0.322, obs 0.356, frame sample 0.304; mean: actions 0.437,
    obs 0.211; frame sum and L2 norm below 0.006).  Step-0 pixels that differ from the fp64 run's: 0 of 60 000 (printed, not gated
    beyond one level).  DESIGN.md section 6b.23."""
    golden = np.load(os.path.join(HERE, "golden", "slac_imagine_fa_golden_v1.npz"))
    m, po = model, policy
    z0, noise = [t.cuda() for t in FA.make_inputs(FA.B, FA.H)]
    window = torch.from_numpy(golden["window"]).cuda()
    assert np.array_equal(golden["z0"], z0.cpu().numpy()) and np.array_equal(golden["noise"], noise.cpu().numpy())
    ratios = {}
    for rollout, sample in zip(FA.ROLLOUTS, (True, False)):
        act, mean, std, z, obs, _ = _run(m, po, z0, window, noise, H=FA.H, sample=sample, quantize=False, final_obs=True)
        frames = m.decoder(z)[0].clamp_(0.0, 1.0)                        # what the hand-off clamped, as fp32 NCHW
        got = FA.measures(dict(actions=act, z1_mean=mean, z1_std=std, z=z, obs=obs, frames=frames))
        for k in FA.QUANTITIES:
            key = "%s.%s" % (rollout, k)
            e32 = np.maximum(golden[key + ".ref32_err"], FLOOR)
            ratios[key] = float(np.max(FA.step_err(got[k], golden[key]).numpy() / e32))
    fr = _run(m, po, z0, window, noise, H=FA.H, keep_frames=True)[5][:, 0].cpu().numpy().astype(np.int64)
    want = golden["sampled.frames_u8_step0"].astype(np.int64)
    assert fr.shape == want.shape == (FA.B, 100, 100, 3)
    off = np.abs(fr - want)
    with capsys.disabled():
        for key, r in ratios.items():
            print("\n%-22s deviation / max(ref32_err, 1e-6): %.6f" % (key, r), end="")
        print("\nworst: %.6f; step-0 pixels that differ from the fp64 run's: %d of %d (%.4f %%), worst by %d level(s)"
              % (max(ratios.values()), int((off > 0).sum()), off.size, 100.0 * float((off > 0).mean()), int(off.max())))
    for key, r in ratios.items():
        assert r <= K_TOL, (key, r)
    assert int(off.max()) <= 1


# ---- the command lines ---------------------------------------------------------------------------------------------------------------------
def _dirs(tmp_path, model, policy, real_windows):
    data = real_windows[0]
    path, ldir = str(tmp_path / "real.npz"), str(tmp_path / "latent")
    np.savez(path, **data)
    model.save_model(ldir)
    pdirs = []
    for name, po in (("fa", policy), ("z", _z_policy())):
        d = str(tmp_path / name)
        os.makedirs(d)
        torch.save(po.state_dict(), os.path.join(d, "policy.pth"))
        torch.save(_critic().state_dict(), os.path.join(d, "critic.pth"))
        pdirs.append(d)
    return path, ldir, pdirs


def test_command_lines(model, policy, real_windows, tmp_path, capsys):
    import imagine_policy
    import select_policy
    path, ldir, (dfa, dz) = _dirs(tmp_path, model, policy, real_windows)
    common = ["--context", str(CONTEXT), "--horizon", str(H), "--windows", "3", "--stride", "1", "--batch", "2", "--seed", "4"]
    out = str(tmp_path / "imag.npz")
    imagine_policy.main(["--data", path, "--latent_dir", ldir, "--policy_dir", dfa, "--out", out, "--bootstrap"] + common)
    text = capsys.readouterr().out
    assert "feature_action (8 frames)" in text and "imagined return" in text and "wrote" in text
    with np.load(out) as f:
        r = {k: f[k] for k in f.files}
    assert set(r) == {"policy_return", "behaviour_return", "data_return", "bootstrap", "policy_value", "actions", "z", "starts"}
    assert r["actions"].shape == (3, H, A) and r["z"].shape == (3, H, Z) and all(np.isfinite(v).all() for v in r.values())
    # a mixed pair, ranked; --frames holds the best feature_action policy's frames
    sel, fr = str(tmp_path / "sel.npz"), str(tmp_path / "frames.npy")
    base = ["--data", path, "--latent_dir", ldir, "--out", sel] + common
    select_policy.main(base + ["--policy_dirs", dfa, dz, "--mean"])
    text = capsys.readouterr().out
    assert "feature_action (8 frames)" in text and "latent_z" in text and "rank" in text
    with np.load(sel) as f:
        s = {k: f[k] for k in f.files}
    assert set(s) == {"returns", "behaviour_return", "data_return", "order", "starts", "policy_dirs"}
    assert s["returns"].shape == (2, 3) and sorted(s["order"].tolist()) == [0, 1] and np.isfinite(s["returns"]).all()
    select_policy.main(base + ["--policy_dirs", dfa, "--frames", fr])
    frames = np.load(fr)
    assert frames.dtype == np.uint8 and frames.shape == (3, H - 1, 100, 100, 3) and len(np.unique(frames)) > 4
    quant = np.load(sel)["returns"]
    select_policy.main(base + ["--policy_dirs", dfa, "--float_frames"])
    assert not np.array_equal(np.load(sel)["returns"], quant)
    capsys.readouterr()
