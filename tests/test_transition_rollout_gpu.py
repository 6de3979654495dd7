"""N2c on the device: s2p_transition_pack (csrc/transition.hip) bit for bit against numpy's fp32 `(o - m) / s`, and
EnsembleTransition.rollout_sweep against the fixture of the real reference (tests/golden/transition_rollout_golden_v1.npz), against
the oracle at the reference's width, against rollout_step, across chunk sizes (bitwise), and end to end through rollout_dynamics.py."""
import os

import numpy as np
import pytest
import torch

import ensemble_oracle as EO

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "transition_rollout_golden_v1.npz"))
E = np.load(os.path.join(HERE, "golden", "ensemble_golden_v1.npz"))
SD = {k[3:]: torch.from_numpy(E[k]) for k in E.files if k.startswith("sd.")}
DATA = {k[3:]: G[k] for k in G.files if k.startswith("in.")}
OUT = {k[4:]: G[k] for k in G.files if k.startswith("out.")}
CFG = {k[4:]: (G[k] if G[k].ndim else float(G[k])) for k in G.files if k.startswith("cfg.")}
STATS = tuple(CFG[k] for k in ("obs_mean", "obs_std", "next_obs_mean", "next_obs_std", "reward_mean", "reward_std"))
PREDICTED = ("next_observations", "rewards", "disagreement_uncertainty", "aleatoric_uncertainty")


def close(a, b, tol):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12)) < tol


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- s2p_transition_pack ---------------------------------------------------------------------------------------------------------------
def pack_case(dev, rows, od, A, pitch, strided=False, misaligned=False, seed=0):
    """Runs the kernel into a NaN-filled buffer with slack on both sides; returns (x, expected, untouched words before / after)."""
    from s2p_amd import ops
    r = np.random.RandomState(seed)
    std = (10.0 ** r.uniform(-3, 3, od)).astype(np.float32)                 # 1e-3 .. 1e3
    mean = (r.randn(od) * 3).astype(np.float32)
    so, sa = (od + 3, A + 2) if strided else (od, A)
    obs_full = np.full((rows, so), 7.0, np.float32)
    obs_full[:, :od] = r.randn(rows, od) * std + mean
    act_full = np.full((rows, sa), 9.0, np.float32)
    act_full[:, :A] = r.uniform(-1, 1, (rows, A))
    off, slack = (1 if misaligned else 0), 64
    flat = torch.full((off + rows * pitch + slack,), float("nan"), dtype=torch.float32, device=dev)
    x = flat[off:off + rows * pitch].view(rows, pitch)
    assert (x.data_ptr() % 16 != 0) == misaligned
    obs, act = torch.from_numpy(obs_full).to(dev)[:, :od], torch.from_numpy(act_full).to(dev)[:, :A]
    assert obs.stride(0) == so and act.stride(0) == sa
    ops.transition_pack(obs, act, torch.from_numpy(mean).to(dev), torch.from_numpy(std).to(dev), x)
    expected = np.zeros((rows, pitch), np.float32)
    expected[:, :od] = (obs_full[:, :od] - mean) / std
    expected[:, od:od + A] = act_full[:, :A]
    host = flat.cpu().numpy()
    return host[off:off + rows * pitch].reshape(rows, pitch), expected, np.concatenate([host[:off], host[off + rows * pitch:]])


@pytest.mark.parametrize("rows,od,A,pitch", [(1, 17, 6, 24), (37, 17, 6, 24), (1030, 17, 6, 32), (5, 5, 3, 8)])
def test_pack_is_numpy_fp32_bit_for_bit(hip_device, rows, od, A, pitch):
    x, expected, outside = pack_case(hip_device, rows, od, A, pitch)
    assert expected.dtype == np.float32 and np.isfinite(expected).all()
    assert np.array_equal(bits(x), bits(expected))
    assert (bits(x[:, od + A:]) == 0).all()                                  # pad columns: +0 where the buffer held NaN
    assert np.isnan(outside).all() and len(outside) == 64                    # memory after the last row is untouched


def test_pack_reads_strided_sources(hip_device):
    x, expected, outside = pack_case(hip_device, 37, 17, 6, 24, strided=True, seed=1)
    assert np.array_equal(bits(x), bits(expected)) and np.isnan(outside).all()


@pytest.mark.parametrize("pitch", [24, 23, 27])
def test_pack_per_element_path(hip_device, pitch):
    """A view offset by 4 bytes (x misaligned) or a pitch that is no multiple of 4: the per-element kernel."""
    x, expected, outside = pack_case(hip_device, 37, 17, 6, pitch, misaligned=(pitch == 24), seed=2)
    assert np.array_equal(bits(x), bits(expected))
    assert np.isnan(outside).all() and len(outside) == 64 + (pitch == 24)


def test_pack_argument_checking(hip_device):
    from s2p_amd._lib import lib, ptr, stream
    L, dev = lib(), hip_device
    o, a = torch.zeros(4, 17, device=dev), torch.zeros(4, 6, device=dev)
    m, s = torch.zeros(17, device=dev), torch.ones(17, device=dev)
    x = torch.full((4, 24), float("nan"), device=dev)

    def call(rows=4, xp=ptr(x), pitch=24, op=17, ap=6, obs=ptr(o)):
        return L.s2p_transition_pack(obs, op, ptr(a), ap, ptr(m), ptr(s), rows, 17, 6, xp, pitch, stream())
    for kw, msg in ((dict(rows=-1), b"negative"), (dict(xp=None), b"null"), (dict(pitch=22), b"pitch"), (dict(op=16), b"pitch"),
                    (dict(ap=5), b"pitch"), (dict(obs=None), b"null")):
        assert call(**kw) != 0 and msg in L.s2p_last_error(), kw
    assert torch.isnan(x).all()                                              # refused before any launch
    assert call(rows=0) == 0 and call(rows=0, xp=None, obs=None) == 0
    assert torch.isnan(x).all()
    assert call() == 0 and bool((x[:, :17] == 0).all()) and bool((x[:, 23] == 0).all())


# ---- rollout_sweep ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(hip_device):
    from s2p_amd.dynamics import EnsembleTransition
    return EnsembleTransition(17, 6, 64, 3, ensemble_size=7).load_state_dict(SD)


@pytest.fixture(scope="module")
def swept(model):
    """The fixture's dataset at the default chunk: computed once, shared, left unchanged."""
    return tuple(t.cpu() for t in model.rollout_sweep(DATA["observations"], OUT["actions"], G["ensemble_idx"], *STATS))


def test_sweep_matches_the_real_reference(swept):
    assert [tuple(t.shape) for t in swept] == [(31, 17), (31,), (31, 1), (31, 1)] and all(t.dtype == torch.float32 for t in swept)
    for k, t in zip(PREDICTED, swept):
        print(k, "relative-to-max error %.3g" % float((t.double() - torch.from_numpy(OUT[k]).double()).abs().max() / np.abs(OUT[k]).max()))
        assert close(t, OUT[k], 1e-5), k


@pytest.mark.parametrize("chunk", [7, 31])
def test_a_row_does_not_depend_on_the_chunk(model, swept, chunk):
    got = model.rollout_sweep(DATA["observations"], OUT["actions"], G["ensemble_idx"], *STATS, chunk=chunk)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(got, swept))


def test_full_width_sweep_is_chunk_invariant_and_matches_the_oracle(hip_device):
    """E 7, H 256, 70 rows: chunk 33 straddles a 32-row tile; against the oracle in fp64 on the fp32-normalised input."""
    from s2p_amd.dynamics import EnsembleTransition
    g = torch.Generator().manual_seed(3)
    Em, H, N = 7, 256, 70
    sd = {}
    for i, (a, b) in enumerate([(23, H), (H, H), (H, H)]):
        sd[f"backbones.{i}.weight"] = torch.randn(Em, a, b, generator=g) / (2 * a ** 0.5)
        sd[f"backbones.{i}.bias"] = torch.randn(Em, 1, b, generator=g) * 0.1
    sd["output_layer.weight"] = torch.randn(Em, H, 36, generator=g) / (2 * H ** 0.5)
    sd["output_layer.bias"] = torch.randn(Em, 1, 36, generator=g) * 0.1
    sd["max_logstd"], sd["min_logstd"] = torch.ones(18), -5 * torch.ones(18)
    r = np.random.RandomState(4)
    scale, shift = r.uniform(0.2, 5.0, 17).astype(np.float32), r.uniform(-3, 3, 17).astype(np.float32)
    obs = (r.randn(N, 17) * scale + shift).astype(np.float32)
    act, idx = r.uniform(-1, 1, (N, 6)).astype(np.float32), r.randint(0, Em, N)
    nom, nos = r.randn(17).astype(np.float32), r.uniform(0.5, 1.5, 17).astype(np.float32)
    m = EnsembleTransition(17, 6, H, 3, ensemble_size=Em).load_state_dict(sd)
    a = m.rollout_sweep(obs, act, idx, shift, scale, nom, nos, 2.991, 1.092, chunk=33)
    b = m.rollout_sweep(obs, act, idx, shift, scale, nom, nos, 2.991, 1.092, chunk=70)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    x = torch.from_numpy(np.concatenate([(obs - shift) / scale, act], 1)).double()
    mean, std = EO.ensemble_forward({k: v.double() for k, v in sd.items()}, x, 17)
    ref = EO.rollout_postprocess(mean, std, torch.from_numpy(idx).long(), torch.from_numpy(nom).double(),
                                 torch.from_numpy(nos).double(), 2.991, 1.092)
    for name, u, v in zip(PREDICTED, a, ref):
        assert close(u.cpu(), v.reshape(u.shape), 1e-5), name


def test_sweep_agrees_with_rollout_step_per_trajectory(model, swept):
    x = np.concatenate([(DATA["observations"] - CFG["obs_mean"]) / CFG["obs_std"], OUT["actions"]], 1)
    parts = [model.rollout_step(torch.from_numpy(x[s:e]), G["ensemble_idx"][s:e], *STATS[2:]) for s, e in ((0, 9), (9, 21), (21, 31))]
    for k, (name, t) in enumerate(zip(PREDICTED, swept)):
        assert close(t, torch.cat([p[k].cpu() for p in parts], 0), 1e-5), name


def test_sweep_leaves_select_alone(hip_device, swept):
    from s2p_amd.dynamics import EnsembleTransition
    m = EnsembleTransition(17, 6, 64, 3, ensemble_size=7).load_state_dict(SD)
    m.set_select([0, 2, 3, 5, 6])
    got = m.rollout_sweep(DATA["observations"], OUT["actions"], G["ensemble_idx"], *STATS)
    assert m.select == [0, 2, 3, 5, 6]
    assert all(torch.equal(a.cpu(), b) for a, b in zip(got, swept))         # all 7 members ran and were picked from


def test_sweep_refuses_bad_inputs(model):
    with pytest.raises(ValueError, match="member indices"):
        model.rollout_sweep(DATA["observations"], OUT["actions"], np.full(31, 7), *STATS)
    with pytest.raises(ValueError, match="observations"):
        model.rollout_sweep(DATA["observations"][:, :16], OUT["actions"], G["ensemble_idx"], *STATS)
    with pytest.raises(ValueError, match="chunk"):
        model.rollout_sweep(DATA["observations"], OUT["actions"], G["ensemble_idx"], *STATS, chunk=0)


def test_command_line_end_to_end(hip_device, tmp_path):
    import rollout_dynamics
    from s2p_amd.dynamics import EnsembleTransition
    m = EnsembleTransition(17, 6, 32, 2, ensemble_size=7).init_parameters(5)
    model_dir = tmp_path / "world_model"
    model_dir.mkdir()
    torch.save(CFG, str(model_dir / "normalize_configs_dict.pkl"))
    torch.save(m.state_dict(), str(model_dir / "model_dist_state_dict_50.pkl"))
    np.savez(str(tmp_path / "real.npz"), **DATA)
    out_path = str(tmp_path / "gen_states.npz")
    rollout_dynamics.main(["--data", str(tmp_path / "real.npz"), "--model_dir", str(model_dir), "--iter", "50", "--out", out_path, "--seed",
                           str(int(G["seed"])), "--action_low"] + [str(v) for v in G["act_low"]] + ["--action_high"] +
                          [str(v) for v in G["act_high"]] + ["--chunk", "16"])
    with np.load(out_path) as z:
        written = {k: z[k] for k in z.files}
    assert set(written) == set(OUT)
    for k in OUT:
        assert written[k].dtype == OUT[k].dtype and written[k].shape == OUT[k].shape, k
        if k not in PREDICTED:
            assert np.array_equal(written[k], OUT[k]), k
    direct = m.rollout_sweep(DATA["observations"], OUT["actions"], G["ensemble_idx"], *STATS)
    for k, t in zip(PREDICTED, direct):
        assert np.array_equal(bits(written[k]), bits(t.cpu().numpy())) and np.isfinite(written[k]).all(), k
