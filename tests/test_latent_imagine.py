"""N3j on the host: the imagination chain's entry point is exported and declared and refuses bad arguments before any launch (so
without a device); the plain-torch restatement of the closed-loop rollout reproduces the recorded results of the real reference's
modules; the return / value arithmetic and `behaviour`'s window bookkeeping on stand-in models; imagine_policy.py's command line."""
import os

import numpy as np
import pytest
import torch

import slac_imagine_ref as IR
import slac_latent_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "s2p_imagine_chain_fwd"
P = 4096                                               # a non-NULL, 16-byte aligned address: refusals happen before any launch
Z1, Z = 32, 288


def test_symbol_is_exported_and_declared():
    from s2p_amd import _lib
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME]) == 22
    header = open(os.path.join(ROOT, "include", "s2p_hip.h")).read()
    assert "int %s(" % NAME in header and "} s2p_policy_mlp;" in header
    assert hasattr(_lib.lib(), NAME)
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert _lib.lib().s2p_version() == 125                 # the version stays (tests/test_slac_latent.py pins it)


def _mlps(_lib, edit=None):
    arr = (_lib.ChainMlp * 2)(_lib.ChainMlp(P, P, P, P, P, P, 256, 264), _lib.ChainMlp(P, P, P, P, P, P, 288, 288))
    if edit is not None and edit[0] in (0, 1):
        setattr(arr[edit[0]], edit[1], edit[2])
    return arr


def _policy(_lib, edit=None):
    p = _lib.PolicyMlp(P, P, P, P, P, P, 288, 256)
    if edit is not None and edit[0] == "p":
        setattr(p, edit[1], edit[2])
    return p


def test_refusals_and_the_empty_batch_without_a_device():
    import ctypes
    from s2p_amd import _lib
    L = _lib.lib()

    def call(z0=P, z0_pitch=288, eps=P, eps_pitch=288, mlps="ok", wc=P, wc_row=8, wb=P, wb_row=8, A=6, policy="ok", act=P, act_pitch=8,
             mean=P, mean_pitch=32, std=P, std_pitch=32, z=P, z_pitch=288, B=4, H=9, edit=None):
        return L.s2p_imagine_chain_fwd(z0, z0_pitch, eps, eps_pitch, _mlps(_lib, edit) if mlps == "ok" else mlps, wc, wc_row, wb, wb_row, A,
                                       ctypes.byref(_policy(_lib, edit)) if policy == "ok" else policy, act, act_pitch, mean, mean_pitch,
                                       std, std_pitch, z, z_pitch, B, H, None)

    # B == 0 (and H == 0): a successful no-op that looks at no pointer
    none = (None, 0, None, 0, None, None, 0, None, 0, 0, None, None, 0, None, 0, None, 0, None, 0)
    assert L.s2p_imagine_chain_fwd(*none, 0, 9, None) == 0
    assert L.s2p_imagine_chain_fwd(*none, 4, 0, None) == 0
    bad = dict(negative_B=dict(B=-1), negative_H=dict(H=-1), null_z0=dict(z0=None), null_eps=dict(eps=None), null_mlps=dict(mlps=None),
               null_wc=dict(wc=None), null_wb=dict(wb=None), null_policy=dict(policy=None), null_act=dict(act=None),
               null_mean=dict(mean=None), null_std=dict(std=None), null_z=dict(z=None),
               A_zero=dict(A=0), A_nine=dict(A=9), A_negative=dict(A=-1),
               z0_pitch_short=dict(z0_pitch=284), z0_pitch_z2_only=dict(z0_pitch=256), eps_pitch_short=dict(eps_pitch=287),
               act_pitch_short=dict(act_pitch=5), mean_pitch_short=dict(mean_pitch=31), std_pitch_short=dict(std_pitch=16),
               z_pitch_short=dict(z_pitch=256), z0_misaligned=dict(z0=P + 4), z0_pitch_not_4=dict(z0_pitch=290),
               wc_row_short=dict(wc_row=4), wb_row_short=dict(wb_row=4), wc_row_not_4=dict(wc_row=10), wb_row_not_4=dict(wb_row=9),
               wc_misaligned=dict(wc=P + 4), wb_misaligned=dict(wb=P + 8),
               k1_with_the_action_columns=dict(edit=(0, "k1", 262)), k1_of_the_other_head=dict(edit=(1, "k1", 256)),
               k1_swapped=dict(edit=(0, "k1", 288)), w1_row_short=dict(edit=(1, "w1_row", 284)), w1_row_not_4=dict(edit=(0, "w1_row", 262)),
               w1_misaligned=dict(edit=(0, "w1", P + 4)), w3_misaligned=dict(edit=(1, "w3", P + 4)), null_weight=dict(edit=(0, "w1", None)),
               null_bias=dict(edit=(1, "b2", None)),
               width_64=dict(edit=("p", "width", 64)), width_192=dict(edit=("p", "width", 192)), width_1152=dict(edit=("p", "width", 1152)),
               width_0=dict(edit=("p", "width", 0)), policy_w1_row_short=dict(edit=("p", "w1_row", 284)),
               policy_w1_row_not_4=dict(edit=("p", "w1_row", 290)), policy_w1_misaligned=dict(edit=("p", "w1", P + 4)),
               policy_w2_misaligned=dict(edit=("p", "w2", P + 8)), policy_w3_misaligned=dict(edit=("p", "w3", P + 4)),
               policy_null_weight=dict(edit=("p", "w2", None)), policy_null_bias=dict(edit=("p", "b3", None)))
    for name, kw in bad.items():
        assert call(**kw) != 0, name
        assert NAME.encode() in L.s2p_last_error(), name
    assert call(z_pitch=100) != 0 and b"pitch" in L.s2p_last_error()
    assert call(edit=(0, "b3", None)) != 0 and b"z1_prior" in L.s2p_last_error()
    assert call(edit=(1, "k1", 294)) != 0 and b"z2_prior" in L.s2p_last_error()
    assert call(edit=("p", "width", 320)) != 0 and b"policy" in L.s2p_last_error() and b"128" in L.s2p_last_error()


def test_the_restatement_reproduces_the_recorded_reference():
    G = np.load(os.path.join(ROOT, "tests", "golden", "slac_imagine_golden_v1.npz"))
    assert tuple(G["dims"]) == (IR.B, IR.H, IR.A, IR.W) and float(G["discount"]) == IR.DISCOUNT
    p = {k: v.double() for k, v in R.make_params(IR.A).items()}
    pol = {k: v.double() for k, v in IR.make_policy_params().items()}
    qs = [{k: v.double() for k, v in IR.make_q_params(i).items()} for i in range(2)]
    assert abs(R.checksum(p) - float(G["checksum"])) <= 1e-9 * float(G["checksum"])
    assert abs(R.checksum(pol) - float(G["policy_checksum"])) <= 1e-9 * float(G["policy_checksum"])
    assert all(abs(R.checksum(q) - float(c)) <= 1e-9 * float(c) for q, c in zip(qs, G["qf_checksum"]))
    z0, noise = IR.make_inputs()
    assert np.array_equal(G["z0"], z0.numpy()) and np.array_equal(G["noise"], noise.numpy())
    for name, sample in zip(IR.ROLLOUTS, (True, False)):
        got = IR.run_all(p, pol, qs, z0.double(), noise.double(), sample)
        for k in IR.QUANTITIES:
            want, e32 = G["%s.%s" % (name, k)], G["%s.%s.ref32_err" % (name, k)]
            assert tuple(got[k].shape) == want.shape and np.isfinite(want).all() and np.abs(want).max() > 0
            assert e32.shape == ((IR.H,) if k in IR.STEPWISE else ()) and (e32 > 0).all() and (e32 < 1e-4).all(), (name, k)
            err = R.rel_max(got[k], want)
            assert err <= 1e-9, (name, k, err)
        # what the generator asserted, so the fixture keeps its meaning
        a = np.abs(G[name + ".actions"])
        assert a.min() <= 0.1 and a.max() >= 0.9
        assert float(G[name + ".z.ref32_err"][-1]) <= 1e-4
        assert float(G[name + ".z1_std"].min()) > 0 and float(G[name + ".reward_std"].min()) > 0
    assert R.rel_max(G["sampled.z"], G["mean.z"]) > 1e-2
    # the loop is closed: z1(0) IS an input (the policy reads it), unlike the open-loop rollout's
    z0b = z0.double().clone()
    z0b[:, :Z1] += 1.0
    assert not torch.equal(IR.imagine(p, pol, z0b, noise.double())[0][:, 0], torch.as_tensor(G["sampled.actions"][:, 0]))


def test_discounted_sum_and_value():
    from s2p_amd.slac_imagine import discounted
    r = torch.tensor([[1.0, 2.0, 3.0], [0.5, -1.0, 4.0]], dtype=torch.float32)
    got = discounted(r, 0.9)
    assert got.dtype == torch.float64 and got.shape == (2,)
    want = [1.0 + 0.9 * 2.0 + 0.81 * 3.0, 0.5 - 0.9 + 0.81 * 4.0]
    assert np.allclose(got.numpy(), want, rtol=1e-14, atol=0)
    assert discounted(r, 1.0).tolist() == [6.0, 3.5] and discounted(r[:, :1], 0.3).tolist() == [1.0, 0.5]
    # fp64: a sum fp32 would round
    big = torch.tensor([[1e8, 1.0, -1e8]], dtype=torch.float32)
    assert discounted(big, 1.0).tolist() == [1.0]


class _Latent:
    """A stand-in on the CPU with LatentModel's call surface: records what it is asked, answers with simple functions of it."""
    device = torch.device("cpu")
    action_dim = 2

    def __init__(self):
        self.calls = []

    def encoder(self, frames):
        self.calls.append(("encoder", tuple(frames.shape)))
        return frames.float().mean(dim=(2, 3, 4))[..., None].expand(*frames.shape[:2], 256)

    def sample_posterior(self, feat, actions, noise):
        self.calls.append(("sample_posterior", tuple(feat.shape), tuple(actions.shape), noise is None))
        B, T = feat.shape[:2]
        z1 = feat[..., :Z1] + actions.sum(-1).sum(-1)[:, None, None]
        return None, None, z1, feat.new_zeros(B, T, 256) + feat[..., :1]

    def imagine(self, policy, z0, H, noise, sample):
        self.calls.append(("imagine", H, sample))
        B = z0.shape[0]
        act = torch.stack([policy.act(z0) * (h + 1) for h in range(H)], 1)
        z = torch.stack([z0 + h + 1 for h in range(H)], 1)
        return act, z[..., :Z1], z[..., :Z1], z

    def predict(self, z0, actions, noise, sample):
        self.calls.append(("predict", actions.clone(), sample))
        H = actions.shape[1]
        z = torch.stack([z0 + h + 1 for h in range(H)], 1)
        return z[..., :Z1], z[..., :Z1], z

    def predict_reward(self, z0, z, actions):
        return actions.sum(-1) + z[..., 0], torch.ones(actions.shape[:2])


class _Policy:
    def act(self, z):
        return torch.stack([z[:, 0], -z[:, 0]], 1) * 0.01


class _Critic:
    def q_min(self, z, a):
        return (z[:, 0] + a[:, 0]).float()


def _dataset(n=17):
    t = np.zeros(n, dtype=bool)
    t[[4, 16]] = True
    return dict(timeouts=t, image_observations=np.arange(n, dtype=np.uint8).reshape(n, 1, 1, 1).repeat(3, 3),
                image_observations_tp1=(1 + np.arange(n, dtype=np.uint8)).reshape(n, 1, 1, 1).repeat(3, 3),
                actions=np.arange(2 * n, dtype=np.float32).reshape(n, 2) / 10, rewards=np.arange(n, dtype=np.float32).reshape(n, 1))


def test_imagined_returns_arithmetic():
    from s2p_amd.slac_imagine import imagined_returns
    d, lat, C, H, g = _dataset(), _Latent(), 3, 4, 0.9
    from s2p_amd.slac_predict import gather
    frames, actions, _ = gather(d, np.array([5, 9]), C + H)
    out = imagined_returns(lat, _Policy(), frames, actions, H, discount=g, critic=_Critic(), context=C, sample=False)
    assert lat.calls[0] == ("encoder", (2, C + 1, 1, 1, 3)) and lat.calls[1] == ("sample_posterior", (2, C + 1, 256), (2, C, 2), False)
    assert lat.calls[2] == ("imagine", H, False)
    assert set(out) == {"z0", "actions", "z", "z1_mean", "z1_std", "reward_mean", "reward_std", "returns", "bootstrap", "value"}
    rm = out["reward_mean"].double()
    want = sum(g ** h * rm[:, h] for h in range(H))
    assert out["returns"].dtype == torch.float64 and torch.allclose(out["returns"], want, rtol=1e-14, atol=0)
    zH = out["z"][:, -1]
    boot = _Critic().q_min(zH, _Policy().act(zH))
    assert torch.equal(out["bootstrap"], boot)
    assert torch.allclose(out["value"], want + g ** H * boot.double(), rtol=1e-14, atol=0)
    assert "bootstrap" not in imagined_returns(lat, _Policy(), frames, actions, H, context=C)
    with pytest.raises(ValueError):
        imagined_returns(lat, _Policy(), frames, actions, 0, context=C)
    with pytest.raises(ValueError):
        imagined_returns(lat, _Policy(), frames[:, :C], actions, H, context=C)              # a frame short of the context
    with pytest.raises(ValueError):
        imagined_returns(lat, _Policy(), frames.astype(np.float32), actions, H, context=C)


def test_behaviour_window_bookkeeping():
    from s2p_amd.slac_imagine import behaviour
    from s2p_amd.slac_predict import windows
    d, lat, C, H, g = _dataset(), _Latent(), 3, 4, 0.9
    starts = windows(d, C + H, stride=2)
    assert starts.tolist() == [5, 7, 9]                    # the 5-row trajectory holds no window of 7 steps
    out = behaviour(lat, d, starts, C, H, discount=g)
    kind, acts, sample = lat.calls[-1]
    assert kind == "predict" and sample is True
    rows = starts[:, None] + C + np.arange(H)[None]        # the H rows after the context
    assert np.array_equal(acts.numpy(), d["actions"][rows]) and np.array_equal(out["actions"].numpy(), d["actions"][rows])
    assert lat.calls[0] == ("encoder", (3, C + 1, 1, 1, 3)) and lat.calls[1][2] == (3, C, 2)
    want = (d["rewards"][:, 0][rows].astype(np.float64) * g ** np.arange(H)).sum(1)
    assert out["data_returns"].dtype == torch.float64 and np.allclose(out["data_returns"].numpy(), want, rtol=1e-14, atol=0)
    rm = out["reward_mean"].double().numpy()
    assert np.allclose(out["returns"].numpy(), (rm * g ** np.arange(H)).sum(1), rtol=1e-14, atol=0)
    with pytest.raises(ValueError):
        behaviour(lat, d, starts, C, 0)


BASE = ["--data", "d.npz", "--latent_dir", "l", "--policy_dir", "p", "--out", "o.npz"]


def test_command_line_parser():
    import imagine_policy
    a = imagine_policy.parse_args(BASE)
    assert (a.context, a.horizon, a.windows, a.batch, a.stride, a.seed, a.discount) == (8, 16, 256, 256, None, 0, 0.99)
    assert not (a.mean or a.bf16 or a.fused_chain or a.bootstrap)
    a = imagine_policy.parse_args(BASE + ["--horizon", "3", "--mean", "--fused_chain", "--bootstrap", "--bf16", "--stride", "2",
                                          "--discount", "0.9"])
    assert a.horizon == 3 and a.stride == 2 and a.mean and a.fused_chain and a.bootstrap and a.bf16 and a.discount == 0.9
    for bad in (["--context", "0"], ["--windows", "0"], ["--batch", "0"], ["--stride", "0"], ["--horizon", "x"]):
        with pytest.raises(SystemExit):
            imagine_policy.parse_args(BASE + bad)
    for missing in ("--data", "--latent_dir", "--policy_dir", "--out"):
        i = BASE.index(missing)
        with pytest.raises(SystemExit):
            imagine_policy.parse_args(BASE[:i] + BASE[i + 2:])


def _files(tmp_path, obs_dim=Z, n=17):
    path, pdir = str(tmp_path / "data.npz"), str(tmp_path / ("p%d" % obs_dim))
    np.savez(path, **_dataset(n))
    os.makedirs(pdir, exist_ok=True)
    sd = {"fc0.weight": torch.zeros(32, obs_dim), "fc0.bias": torch.zeros(32), "fc1.weight": torch.zeros(32, 32), "fc1.bias": torch.zeros(32),
          "last_fc.weight": torch.zeros(2, 32), "last_fc.bias": torch.zeros(2), "last_fc_log_std.weight": torch.zeros(2, 32),
          "last_fc_log_std.bias": torch.zeros(2)}
    torch.save(sd, os.path.join(pdir, "policy.pth"))
    return ["--data", path, "--latent_dir", str(tmp_path), "--policy_dir", pdir, "--out", str(tmp_path / "o.npz")]


def test_command_line_exits(tmp_path):
    """Each is a SystemExit with a message, never a traceback; what needs no device is checked before the device is asked for."""
    import imagine_policy
    with pytest.raises(SystemExit, match="--horizon"):
        imagine_policy.main(_files(tmp_path) + ["--horizon", "0"])
    with pytest.raises(SystemExit, match="no trajectory.*14 steps"):
        imagine_policy.main(_files(tmp_path) + ["--horizon", "6"])
    with pytest.raises(SystemExit, match="latent_z.*288"):
        imagine_policy.main(_files(tmp_path, obs_dim=1536) + ["--context", "3", "--horizon", "4"])
    assert imagine_policy.net_shape(torch.load(os.path.join(str(tmp_path), "p288", "policy.pth"))) == ([32, 32], Z, 2)
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match="HIP device"):
            imagine_policy.main(_files(tmp_path) + ["--context", "3", "--horizon", "4"])
