"""N3i on the host: the prior chain's entry point is exported and declared and refuses bad arguments before any launch (so without a
device); the plain-torch restatement of the open-loop rollout reproduces the recorded results of the real reference's modules;
`windows` finds the stretches of a dataset an open-loop prediction can be asked of; predict_latent.py's command line."""
import os

import numpy as np
import pytest
import torch

import slac_latent_ref as R
import slac_predict_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "s2p_prior_chain_fwd"
K1 = (256, 288)                                        # chain columns of z1_prior's and z2_prior's first layers
P = 4096                                               # a non-NULL, 16-byte aligned address: refusals happen before any launch


def test_symbol_is_exported_and_declared():
    from s2p_amd import _lib
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME]) == 16
    header = open(os.path.join(ROOT, "include", "s2p_hip.h")).read()
    assert "int %s(" % NAME in header
    assert hasattr(_lib.lib(), NAME)
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _mlps(_lib, edit=None):
    arr = (_lib.ChainMlp * 2)(_lib.ChainMlp(P, P, P, P, P, P, 256, 264), _lib.ChainMlp(P, P, P, P, P, P, 288, 288))
    if edit is not None:
        g, field, value = edit
        setattr(arr[g], field, value)
    return arr


def test_refusals_and_the_empty_batch_without_a_device():
    from s2p_amd import _lib
    L = _lib.lib()

    def call(z2_0=P, z2_0_pitch=288, rc=P, rb=P, eps=P, eps_pitch=288, mlps="ok", mean=P, mean_pitch=32, std=P, std_pitch=32, z=P,
             z_pitch=288, B=4, H=9, edit=None):
        return L.s2p_prior_chain_fwd(z2_0, z2_0_pitch, rc, rb, eps, eps_pitch, _mlps(_lib, edit) if mlps == "ok" else mlps, mean,
                                     mean_pitch, std, std_pitch, z, z_pitch, B, H, None)

    # B == 0 (and H == 0): a successful no-op that looks at no pointer
    assert L.s2p_prior_chain_fwd(None, 0, None, None, None, 0, None, None, 0, None, 0, None, 0, 0, 9, None) == 0
    assert L.s2p_prior_chain_fwd(None, 0, None, None, None, 0, None, None, 0, None, 0, None, 0, 4, 0, None) == 0
    bad = dict(negative_B=dict(B=-1), negative_H=dict(H=-1), null_z2_0=dict(z2_0=None), null_rc=dict(rc=None), null_rb=dict(rb=None),
               null_eps=dict(eps=None), null_mlps=dict(mlps=None), null_mean=dict(mean=None), null_std=dict(std=None), null_z=dict(z=None),
               null_rc_at_H1=dict(rc=None, H=1),
               z2_0_pitch_short=dict(z2_0_pitch=252), eps_pitch_short=dict(eps_pitch=287), mean_pitch_short=dict(mean_pitch=31),
               std_pitch_short=dict(std_pitch=16), z_pitch_short=dict(z_pitch=256), z2_0_misaligned=dict(z2_0=P + 4),
               z2_0_pitch_not_4=dict(z2_0_pitch=290),
               k1_with_the_action_columns=dict(edit=(0, "k1", 262)), k1_of_the_other_head=dict(edit=(1, "k1", 256)),
               k1_swapped=dict(edit=(0, "k1", 288)),
               w1_row_short=dict(edit=(1, "w1_row", 284)), w1_row_below_k1=dict(edit=(0, "w1_row", 252)),
               w1_row_not_4=dict(edit=(0, "w1_row", 262)),
               w1_misaligned=dict(edit=(0, "w1", P + 4)), w2_misaligned=dict(edit=(1, "w2", P + 8)), w3_misaligned=dict(edit=(1, "w3", P + 4)),
               null_weight=dict(edit=(0, "w1", None)), null_bias=dict(edit=(1, "b2", None)), null_head=dict(edit=(1, "w3", None)))
    for name, kw in bad.items():
        assert call(**kw) != 0, name
        assert NAME.encode() in L.s2p_last_error(), name
    assert call(z_pitch=100) != 0 and b"pitch" in L.s2p_last_error()
    assert call(edit=(0, "b3", None)) != 0 and b"z1_prior" in L.s2p_last_error()
    assert call(edit=(1, "k1", 294)) != 0 and b"z2_prior" in L.s2p_last_error()


def test_the_restatement_reproduces_the_recorded_reference():
    G = np.load(os.path.join(ROOT, "tests", "golden", "slac_predict_golden_v1.npz"))
    assert tuple(G["dims"]) == (PR.B, PR.H, PR.A)
    p = {k: v.double() for k, v in R.make_params(PR.A).items()}
    assert abs(R.checksum(p) - float(G["checksum"])) <= 1e-9 * float(G["checksum"])
    z0, actions, noise = [t.double() for t in PR.make_inputs()]
    for name, sample in zip(PR.ROLLOUTS, (True, False)):
        got = PR.run_all(p, z0, actions, noise, sample)
        for k in PR.QUANTITIES:
            want = G["%s.%s" % (name, k)]
            assert tuple(got[k].shape) == want.shape and np.isfinite(want).all() and np.abs(want).max() > 0
            err = R.rel_max(got[k], want)
            assert err <= 1e-12, (name, k, err)
        assert float(G[name + ".z1_std"].min()) > 0
    # the two rollouts differ (the noise matters), and z1(0) is not an input
    assert R.rel_max(G["sampled.z"], G["mean.z"]) > 1e-2
    z0b = z0.clone()
    z0b[:, :PR.Z1] += 1.0
    assert torch.equal(PR.predict(p, z0b, actions, noise)[2], PR.predict(p, z0, actions, noise)[2])


def _two_trajectories():
    """Rows 0..4 and 5..16: two trajectories of 5 and 12 rows, each ending ON a timeout row."""
    t = np.zeros(17, dtype=bool)
    t[[4, 16]] = True
    return dict(timeouts=t)


def test_windows_stay_inside_one_trajectory():
    from s2p_amd.slac_predict import windows
    d = _two_trajectories()
    # a window of 5 transitions fits the 5-row trajectory exactly once: it ENDS on the timeout row 4
    assert windows(d, 5, stride=1).tolist() == [0] + list(range(5, 13))
    # length 4: starts 0, 1 in the first (rows 1..4 end on the timeout), 5..13 in the second; none holds a timeout before its last row
    w = windows(d, 4, stride=1)
    assert w.tolist() == [0, 1] + list(range(5, 14))
    for i in w:
        assert not d["timeouts"][i:i + 3].any()
    # no window starts in rows 2..4: it would run over the timeout at row 4 into the next trajectory
    assert not set(w.tolist()) & {2, 3, 4}
    # a window longer than the first trajectory comes from the second alone; the longest fits once
    assert windows(d, 6, stride=1).tolist() == list(range(5, 12))
    assert windows(d, 12, stride=1).tolist() == [5]
    assert w.dtype == np.int64


def test_windows_stride_and_limit():
    from s2p_amd.slac_predict import windows
    d = _two_trajectories()
    assert windows(d, 4).tolist() == [0, 5, 9, 13]                      # default stride = length: no overlap, from each trajectory's first row
    assert windows(d, 4, stride=3).tolist() == [0, 5, 8, 11]
    assert windows(d, 2, stride=5).tolist() == [0, 5, 10, 15]
    assert windows(d, 4, stride=1, limit=100).tolist() == windows(d, 4, stride=1).tolist()
    assert windows(d, 4, stride=1, limit=3).tolist() == [0, 8, 13]      # evenly spread over the 11 windows, ends included
    assert windows(d, 4, stride=1, limit=1).tolist() == [0]
    # `terminals` end a trajectory as `timeouts` do; rows after the last flag are a trajectory that ends at the last row
    t = dict(terminals=np.array([0, 0, 1, 0, 0, 0], dtype=np.float32).reshape(-1, 1))
    assert windows(t, 3, stride=1).tolist() == [0, 3]


def test_windows_errors():
    from s2p_amd.slac_predict import windows
    d = _two_trajectories()
    with pytest.raises(ValueError, match="no trajectory"):
        windows(d, 13)
    with pytest.raises(ValueError, match="no trajectory"):
        windows(dict(timeouts=np.zeros(0, dtype=bool)), 1)
    with pytest.raises(ValueError):
        windows(d, 0)
    with pytest.raises(ValueError):
        windows(d, 4, stride=0)
    with pytest.raises(ValueError):
        windows(d, 4, limit=0)
    with pytest.raises(ValueError, match="timeouts"):
        windows(dict(actions=np.zeros((4, 2))), 2)


def test_gather_reads_the_frames_actions_and_rewards_of_a_window():
    from s2p_amd.slac_predict import gather
    n = 17
    d = dict(_two_trajectories(), image_observations=np.arange(n, dtype=np.uint8).reshape(n, 1, 1, 1).repeat(3, 3),
             image_observations_tp1=(100 + np.arange(n, dtype=np.uint8)).reshape(n, 1, 1, 1).repeat(3, 3),
             actions=np.arange(2 * n, dtype=np.float32).reshape(n, 2), rewards=np.arange(n, dtype=np.float32).reshape(n, 1))
    frames, actions, rewards = gather(d, np.array([1, 13]), 4)
    assert frames.shape == (2, 5, 1, 1, 3) and frames.dtype == np.uint8
    assert frames[:, :, 0, 0, 0].tolist() == [[1, 2, 3, 4, 104], [13, 14, 15, 16, 116]]       # f(length) is the LAST row's tp1 frame
    assert actions[:, :, 0].tolist() == [[2, 4, 6, 8], [26, 28, 30, 32]] and rewards.tolist() == [[1, 2, 3, 4], [13, 14, 15, 16]]


def test_command_line():
    import predict_latent
    base = ["--data", "d.npz", "--latent_dir", "l", "--out", "o.npz"]
    a = predict_latent.parse_args(base)
    assert (a.context, a.horizon, a.windows, a.batch, a.stride, a.seed) == (8, 8, 64, 64, None, 0)
    assert not (a.mean or a.bf16 or a.fused_chain or a.frames)
    a = predict_latent.parse_args(base + ["--horizon", "3", "--mean", "--fused_chain", "--frames", "--bf16", "--stride", "2"])
    assert a.horizon == 3 and a.stride == 2 and a.mean and a.fused_chain and a.frames and a.bf16
    for bad in (["--horizon", "0"], ["--horizon", "-2"], ["--context", "0"], ["--windows", "0"], ["--batch", "0"], ["--stride", "0"]):
        with pytest.raises(SystemExit):
            predict_latent.parse_args(base + bad)
    for missing in ("--data", "--latent_dir", "--out"):
        i = base.index(missing)
        with pytest.raises(SystemExit):
            predict_latent.parse_args(base[:i] + base[i + 2:])


def test_a_file_without_a_long_enough_window_is_a_clear_error(tmp_path, monkeypatch):
    """Without a HIP device the tool stops there; with one it stops at the file: SystemExit either way, and never a traceback."""
    import predict_latent
    path = str(tmp_path / "short.npz")
    np.savez(path, **_two_trajectories())
    with pytest.raises(SystemExit) as e:
        predict_latent.main(["--data", path, "--latent_dir", str(tmp_path), "--out", str(tmp_path / "o.npz"), "--horizon", "5"])
    msg = str(e.value)
    assert ("no trajectory" in msg and "13 steps" in msg) if torch.cuda.is_available() else "HIP device" in msg
