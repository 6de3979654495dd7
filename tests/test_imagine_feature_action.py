"""N3o without a device: the fixture tests/golden/slac_imagine_fa_golden_v1.npz (keys, shapes, the conditions its generator asserts),
the plain-torch restatement of tests/slac_imagine_fa_ref.py against it, the window's layout and the policy-input rule of
s2p_amd/slac_imagine.py, and the exits of imagine_policy.py / select_policy.py that need no device."""
import os

import numpy as np
import pytest
import torch

import slac_imagine_fa_ref as FA
import slac_latent_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
K_TOL, FLOOR = 4.0, 1e-6
G = np.load(os.path.join(HERE, "golden", "slac_imagine_fa_golden_v1.npz"))
SHAPES = dict(actions=(FA.B, FA.H, FA.A), z1_mean=(FA.B, FA.H, 32), z1_std=(FA.B, FA.H, 32), z=(FA.B, FA.H, 288),
              obs=(FA.B, FA.H + 1, FA.OBS), frame_sum=(FA.B, FA.H), frame_l2=(FA.B, FA.H), frame_samp=(FA.B, FA.H, R.NSAMP))


def test_fixture_keys_shapes_and_conditions():
    want = {"seeds", "dims", "z0", "noise", "window", "checksum", "policy_checksum"}
    for r in FA.ROLLOUTS:
        want |= {"%s.%s" % (r, k) for k in FA.QUANTITIES} | {"%s.%s.ref32_err" % (r, k) for k in FA.QUANTITIES}
        want |= {r + ".frames_u8_step0", r + ".frame_shares"}
    assert set(G.files) == want
    assert G["dims"].tolist() == [FA.B, FA.H, FA.A, FA.W, FA.S, FA.CONTEXT] and FA.OBS == 2090
    assert G["window"].shape == (FA.B, FA.OBS) and G["window"].dtype == np.float32
    z0, noise = FA.make_inputs(FA.B, FA.H)
    assert np.array_equal(G["z0"], z0.numpy()) and np.array_equal(G["noise"], noise.numpy())
    assert float(G["checksum"]) == R.checksum(R.make_params(FA.A)) and float(G["policy_checksum"]) == R.checksum(FA.make_policy_params())
    for r in FA.ROLLOUTS:
        for k in FA.QUANTITIES:
            v, e = G["%s.%s" % (r, k)], G["%s.%s.ref32_err" % (r, k)]
            assert v.shape == SHAPES[k] and v.dtype == np.float64 and np.isfinite(v).all(), (r, k)
            assert e.shape == (SHAPES[k][1],) and (e >= 0).all() and e.max() < 1e-4, (r, k)
        assert np.array_equal(G[r + ".obs"][:, 0], G["window"].astype(np.float64))
        u8 = G[r + ".frames_u8_step0"]
        assert u8.dtype == np.uint8 and u8.shape == (FA.B, 100, 100, 3) and len(np.unique(u8)) > 4
        a = np.abs(G[r + ".actions"])
        assert a.min() <= 0.1 and a.max() >= 0.9                            # what the generator asserts: |a| spans [0.1, 0.9]
        clamped, inside = G[r + ".frame_shares"]
        assert clamped >= 0.05 and inside >= 0.05 and abs(clamped + inside - 1.0) < 1e-12      # ... clamped values, and values inside (0, 1)
    assert not np.array_equal(G["sampled.z"], G["mean.z"])
    # the window's layout is create_feature_actions': the actions of the context sit behind the S features
    _, action = FA.context_frames()
    assert np.array_equal(G["window"][:, FA.S * FA.FEAT:], action[:, -(FA.S - 1):].reshape(FA.B, -1).numpy())


@pytest.mark.parametrize("rollout,sample", list(zip(FA.ROLLOUTS, (True, False))))
def test_restatement_matches_the_reference(rollout, sample):
    """tests/slac_imagine_fa_ref.py in fp64 on the fixture's inputs against the reference's fp64 run: the rule, per step."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    p = {k: v.double() for k, v in R.make_params(FA.A).items()}
    pol = {k: v.double() for k, v in FA.make_policy_params().items()}
    z0, noise = [t.double() for t in FA.make_inputs(FA.B, FA.H)]
    if not sample:
        noise = torch.zeros_like(noise)
    out = FA.rollout(p, pol, z0, torch.from_numpy(G["window"]).double(), noise)
    got = FA.measures(out)
    for k in FA.QUANTITIES:
        key = "%s.%s" % (rollout, k)
        ratio = FA.step_err(got[k], G[key]).numpy() / np.maximum(G[key + ".ref32_err"], FLOOR)
        assert ratio.max() <= K_TOL, (key, ratio)
    # the quantised frame of step 0 is the recorded one
    q = torch.round(FA.P.decode(p, out["z"][:, :1])[:, 0] * 255.0).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    assert int((q.numpy().astype(np.int64) - G[rollout + ".frames_u8_step0"].astype(np.int64)).__abs__().max()) <= 1


def test_restatement_helpers():
    w = FA.make_window(5)
    assert w.shape == (5, FA.OBS) and torch.equal(FA.make_window(3), w[:3])
    f, a = torch.randn(5, FA.FEAT), torch.rand(5, FA.A)
    n = FA.push(w, f, a)
    nf = FA.S * FA.FEAT
    assert torch.equal(n[:, :nf - FA.FEAT], w[:, FA.FEAT:nf]) and torch.equal(n[:, nf - FA.FEAT:nf], f)
    assert torch.equal(n[:, nf:-FA.A], w[:, nf + FA.A:]) and torch.equal(n[:, -FA.A:], a)
    x = torch.tensor([-0.1, 0.0, 0.5 / 255, 1.5 / 255, 0.5, 1.0, 1.2])
    assert torch.equal(FA.quantise(x) * 255, torch.tensor([0.0, 0.0, 0.0, 2.0, 128.0, 255.0, 255.0]))      # ties to even: 0.5 -> 0, 1.5 -> 2, 127.5 -> 128


class _Latent:
    action_dim = 6

    @staticmethod
    def feature_action_frames(obs_dim, action_dim):
        from s2p_amd.slac import LatentModel
        return LatentModel.feature_action_frames(obs_dim, action_dim)


class _Pol:
    def __init__(self, obs_dim):
        self.obs_dim = obs_dim


def test_policy_input_rule_and_window_layout():
    from s2p_amd.slac import LatentModel, create_feature_actions
    from s2p_amd.slac_imagine import feature_action_window, policy_frames
    f = LatentModel.feature_action_frames
    assert f(2090, 6) == 8 and f(2 * 256 + 6, 6) == 2 and f(256, 6) is None and f(288, 6) is None and f(2091, 6) is None
    assert f(3 * 256 + 2, 1) == 3 and f(2090, 7) is None
    lat = _Latent()
    assert policy_frames(lat, _Pol(288)) is None and policy_frames(lat, _Pol(2090)) == 8 and policy_frames(lat, object()) is None
    with pytest.raises(ValueError, match="feature_action"):
        policy_frames(lat, _Pol(1536))
    g = torch.Generator().manual_seed(1)
    C, S, A = 9, 8, 6
    feat, actions = torch.randn(2, C + 1, 256, generator=g), torch.randn(2, C + 3, A, generator=g)           # (longer actions are cut)
    w = feature_action_window(feat, actions, C, S)
    assert torch.equal(w, create_feature_actions(feat[:, C - S:], actions[:, C - S:C])[1])
    # the shortest context that holds the window: all S frames, the S - 1 actions between them
    assert torch.equal(feature_action_window(feat[:, :S], actions, S - 1, S),
                       torch.cat([feat[:, :S].reshape(2, -1), actions[:, :S - 1].reshape(2, -1)], 1))
    with pytest.raises(ValueError, match="context"):
        feature_action_window(feat, actions, S - 2, S)


def _files(tmp_path, obs_dim, name, n=40, A=2):
    t = np.zeros(n, dtype=bool)
    t[-1] = True
    path, pdir = str(tmp_path / "data.npz"), str(tmp_path / name)
    np.savez(path, timeouts=t, image_observations=np.zeros((n, 1, 1, 3), dtype=np.uint8), image_observations_tp1=np.zeros((n, 1, 1, 3), dtype=np.uint8),
             actions=np.zeros((n, A), dtype=np.float32), rewards=np.zeros((n, 1), dtype=np.float32))
    os.makedirs(pdir, exist_ok=True)
    sd = {"fc0.weight": torch.zeros(32, obs_dim), "fc0.bias": torch.zeros(32), "fc1.weight": torch.zeros(32, 32), "fc1.bias": torch.zeros(32),
          "last_fc.weight": torch.zeros(A, 32), "last_fc.bias": torch.zeros(A), "last_fc_log_std.weight": torch.zeros(A, 32),
          "last_fc_log_std.bias": torch.zeros(A)}
    torch.save(sd, os.path.join(pdir, "policy.pth"))
    return path, pdir


def test_command_line_exits(tmp_path):
    """Each is an exit with its message before the device is asked for: an obs_dim that fits no S, a --context too short for the
    policy's S, --bf16_chain with a feature_action policy among --policy_dirs."""
    import imagine_policy
    import select_policy
    S8 = 8 * 256 + 7 * 2                                                   # a feature_action policy of 8 frames at A = 2
    path, none = _files(tmp_path, 1536, "none")
    _, fa = _files(tmp_path, S8, "fa")
    _, z = _files(tmp_path, 288, "z")
    tail = ["--latent_dir", str(tmp_path), "--out", str(tmp_path / "o.npz"), "--horizon", "4"]
    with pytest.raises(SystemExit, match="neither a latent_z policy .obs_dim 288. nor a feature_action policy"):
        imagine_policy.main(["--data", path, "--policy_dir", none] + tail)
    with pytest.raises(SystemExit, match="feature_action policy of 8 frames: --context \\+ 1 >= 8 is needed, not --context 6"):
        imagine_policy.main(["--data", path, "--policy_dir", fa, "--context", "6"] + tail)
    with pytest.raises(SystemExit, match="neither a latent_z policy"):
        select_policy.main(["--data", path, "--policy_dirs", z, none] + tail)
    with pytest.raises(SystemExit, match="--context \\+ 1 >= 8"):
        select_policy.main(["--data", path, "--policy_dirs", fa, "--context", "5"] + tail)
    with pytest.raises(SystemExit) as e:
        select_policy.main(["--data", path, "--policy_dirs", z, fa, "--fused_chain", "--bf16_chain"] + tail)
    assert e.value.code == 2                                               # a parser-style exit
    a = select_policy.parse_args(["--data", path, "--policy_dirs", fa, "--float_frames", "--frames", "f.npy"] + tail)
    assert a.float_frames and a.frames == "f.npy"
    b = select_policy.parse_args(["--data", path, "--policy_dirs", fa] + tail)
    assert not b.float_frames and b.frames is None
