"""Device-resident SLAC sequence replay buffer (SPEC.md N3c): s2p_window_gather_u8, s2p_amd.slac_buffer.ReplayBuffer / FrameBatch and
s2p_amd.slac_algo.SlacAlgorithm against tests/golden/slac_buffer_golden_v1.npz, which tests/golden/make_golden_slac_buffer.py
records from the REAL reference loader and buffer on the CPU.  Kernel comparisons are bitwise: uint8 against the plain-torch
`window_frames`, the compute-dtype form against (u8 as fp32) / 255 in IEEE division, cast to the dtype, pad channels zero."""
import os

import numpy as np
import pytest
import torch

import slac_buffer_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "slac_buffer_golden_v1.npz"))
SHAPE = (R.C, R.H, R.W)


def _bits(t):
    t = torch.as_tensor(t).detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same_bits(a, b):
    a, b = torch.as_tensor(a).detach().cpu(), torch.as_tensor(b).detach().cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _algo(size, device="cpu", what=(), capacity=R.FRAME_CAPACITY, **kw):
    """Our SlacAlgorithm without its 100x100 model, as the golden script builds the reference's."""
    from s2p_amd.slac_algo import SlacAlgorithm
    from s2p_amd.slac_buffer import ReplayBuffer
    algo = object.__new__(SlacAlgorithm)
    algo.buffer = ReplayBuffer(size, R.S, SHAPE, (R.A,), device, frame_capacity=capacity, **kw)
    algo.num_sequences, algo.use_seperate_buffer = R.S, False
    for k in what:
        algo.load_data_in_buffer(R.DATASETS[k](), **R.LOAD_ARGS[k])
    return algo


def _check_against_golden(name, buf, penalised_from=None):
    n, p, real_n = (int(v) for v in G[name + ".counts"])
    assert (buf._n, buf._p) == (n, p), (name, buf._n, buf._p)
    if penalised_from is not None:
        assert buf._real_n == real_n, (name, buf._real_n)
    frames = buf.window_frames(range(n))
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (n, R.S + 1, R.H, R.W, R.C)
    assert np.array_equal(frames.permute(0, 1, 4, 2, 3).cpu().numpy(), G[name + ".frames"]), name
    assert _same_bits(buf.action_[:n], torch.from_numpy(G[name + ".action_"])), name
    assert _same_bits(buf.done_[:n], torch.from_numpy(G[name + ".done_"])), name
    assert float(buf.done_[:n].abs().sum()) == 0.0
    got, want = _bits(buf.reward_[:n]).to(torch.int64), _bits(torch.from_numpy(G[name + ".reward_"])).to(torch.int64)
    ulps = (got - want).abs()
    pen = torch.zeros_like(ulps, dtype=torch.bool)                    # the penalised rewards: last step of the generated windows
    if penalised_from is not None:
        pen[penalised_from:, -1] = True
    assert int(ulps[~pen].max()) == 0 and int(ulps.max()) <= 1, (name, int(ulps.max()))


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_window_gather():
    from s2p_amd import _lib
    assert hasattr(_lib.lib(), "s2p_window_gather_u8") and "s2p_window_gather_u8" in _lib.SIGNATURES


def test_window_gather_refuses_bad_arguments_without_a_device():
    from s2p_amd import _lib
    L = _lib.lib()
    p = 4096                                   # a non-NULL, 16-byte aligned address: every refusal happens before any launch

    def call(dtype=0, pool=p, n_slots=10, fp=16, C=3, table=p, T=9, win=p, B=2, x=p, pitch=4, u8=p):
        return L.s2p_window_gather_u8(dtype, pool, n_slots, fp, C, table, T, win, B, x, pitch, u8, None)
    cases = {"bad dtype": dict(dtype=7), "negative n_slots": dict(n_slots=-1), "negative frame_pixels": dict(fp=-1),
             "negative C": dict(C=-1), "negative T": dict(T=-1), "negative B": dict(B=-1), "negative pitch": dict(pitch=-4),
             "C > x_pitch": dict(C=5), "null pool": dict(pool=None), "null table": dict(table=None), "null win": dict(win=None),
             "both outputs null": dict(x=None, u8=None), "misaligned x": dict(x=p + 8)}
    for name, kw in cases.items():
        rc = call(**kw)
        msg = L.s2p_last_error().decode()
        assert rc != 0 and msg.startswith("s2p_window_gather_u8:"), (name, rc, msg)


@pytest.mark.parametrize("name,size,what", R.SCENARIOS, ids=[s[0] for s in R.SCENARIOS])
def test_loader_matches_the_real_reference(name, size, what):
    buf = _algo(size, what=what).buffer
    first_gen = 0 if what == ("gen",) else int(G["real64.counts"][0]) if "gen" in what else size + 1
    _check_against_golden(name, buf, penalised_from=first_gen)


def test_append_surface_matches_the_real_reference():
    from s2p_amd.slac_buffer import ReplayBuffer
    buf = ReplayBuffer(R.APPEND_BUFFER, R.S, SHAPE, (R.A,), "cpu", frame_capacity=R.FRAME_CAPACITY)
    R.drive_append(buf)
    _check_against_golden("append", buf)


def test_frames_are_stored_once():
    buf = _algo(64, what=("real",)).buffer
    assert buf._head <= 2 * R.N and buf._head < buf._n * (R.S + 1)
    # every frame of the real data is shared by up to S+1 windows: 3 trajectories x (reset frame + 14 next-frames), less the
    # dropped last row
    assert buf._head == R.TRAJ * (R.ROWS + 1) - 1


def test_frame_capacity_exhaustion_raises_and_keeps_the_windows():
    from s2p_amd.slac_buffer import ReplayBuffer
    buf = ReplayBuffer(8, R.S, SHAPE, (R.A,), "cpu", frame_capacity=12)
    r = np.random.RandomState(5)
    frame = lambda: r.randint(0, 256, size=SHAPE).astype(np.uint8)
    buf.reset_episode(frame())
    for t in range(11):                                                # 12 frames, 4 windows: the ring is exactly full
        buf.append(np.zeros(R.A, np.float32), 0.0, False, frame(), t == 10)
    before = buf.window_frames(range(4)).clone()
    with pytest.raises(RuntimeError, match="frame_capacity"):
        buf.reset_episode(frame())
    assert (buf._n, buf._p) == (4, 4) and torch.equal(buf.window_frames(range(4)), before)
    # bulk loading: nothing is stored when the block does not fit
    algo = _algo(64, capacity=20)
    with pytest.raises(RuntimeError, match="frame_capacity"):
        algo.load_data_in_buffer(R.real_dataset())
    assert (algo.buffer._n, algo.buffer._p, algo.buffer._head) == (0, 0, 0)


def test_bad_indices_and_types_raise():
    algo = _algo(64, what=("real",))
    buf = algo.buffer
    for bad in ([buf._n], [-1], [0, 20]):
        with pytest.raises(IndexError):
            buf.window_frames(bad)
        with pytest.raises(IndexError):
            buf.random_batch(len(bad), idxes=bad)
    d = R.real_dataset()
    z = np.zeros((1, R.S), np.float32)
    for bad in (2 * R.N, -1):
        slots = np.zeros((1, R.S + 1), np.int64)
        slots[0, 3] = bad
        with pytest.raises(IndexError):
            buf.load_windows((d["image_observations"], d["image_observations_tp1"]), slots, np.zeros((1, R.S, R.A), np.float32), z, z)
    assert buf._n == int(G["real64.counts"][0])
    with pytest.raises(NotImplementedError):
        algo.load_data_in_buffer(R.generated_dataset(), generated_for_slac=True, data_mix_type="no_such_mix")
    with pytest.raises(NotImplementedError):
        algo.load_data_in_buffer(R.generated_dataset(), uncertainty_type="no_such_type", uncertainty_penalty_lambda=1.0,
                                 generated_for_slac=True, data_mix_type="all_state_1step_random_action")
    d = R.generated_dataset()
    d["timeouts"] = d["timeouts"].copy()
    d["timeouts"][3] = True                                            # a timeout inside a window raises, as the reference does
    with pytest.raises(NotImplementedError):
        algo.load_data_in_buffer(d, generated_for_slac=True, data_mix_type="all_state_1step_random_action",
                                 uncertainty_penalty_lambda=0.0)


@pytest.mark.parametrize("utype", [None, "aleatoric", "disagreement", "max_of_both", "min_of_both", "average_both"])
def test_uncertainty_penalty(utype):
    lam = 0.25
    d = R.generated_dataset()
    a, u = d["aleatoric_uncertainty"][:, 0], d["disagreement_uncertainty"][:, 0]
    pick = {None: 0 * a, "aleatoric": a, "disagreement": u, "max_of_both": np.maximum(a, u), "min_of_both": np.minimum(a, u),
            "average_both": 0.5 * (a + u)}[utype]
    want = d["rewards"] - np.float32(lam) * pick
    algo = _algo(64)
    algo.load_data_in_buffer(d, uncertainty_type=utype, uncertainty_penalty_lambda=lam, generated_for_slac=True,
                             data_mix_type="all_state_1step_random_action")
    rows = np.array([i for i in range(R.N - 1) if i % R.ROWS >= R.S])  # rows with a full window; the last row is a timeout
    got = algo.buffer.reward_[:len(rows), -1, 0].numpy()
    assert algo.buffer._n == len(rows)
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want[rows - 1].astype(np.float32).view(np.int32))
    assert ulps.max() <= 1, (utype, ulps.max())


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def _want_nhwc(u8, dtype, pitch):
    """[F,H,W,C] uint8 (cpu) -> (u8 as fp32) / 255 in IEEE division, cast, zero pad."""
    f = torch.from_numpy(u8.numpy().astype(np.float32) / np.float32(255.0)).to(dtype)
    out = torch.zeros(u8.shape[:-1] + (pitch,), dtype=dtype)
    out[..., :u8.shape[-1]] = f
    return out


def _gather(dev, pool, table, win, dtype, pitch, want_x=True, want_u8=True):
    """The entry point on NaN / 0xA5 pre-filled outputs, so that an element it leaves unwritten shows."""
    from s2p_amd._lib import check, dtype_id, lib, ptr, stream
    n_slots, H, W, C = pool.shape
    T, B = table.shape[1], win.numel()
    x = torch.full((B * T, H, W, pitch), float("nan"), dtype=dtype, device=dev) if want_x else None
    u8 = torch.full((B, T, H, W, C), 0xA5, dtype=torch.uint8, device=dev) if want_u8 else None
    pd, td, wd = pool.to(dev), table.to(dev), win.to(dev)
    check(lib().s2p_window_gather_u8(dtype_id(dtype), ptr(pd), n_slots, H * W, C, ptr(td), T, ptr(wd), B, ptr(x), pitch, ptr(u8),
                                     stream()), "s2p_window_gather_u8")
    torch.cuda.synchronize()
    return (None if x is None else x.cpu()), (None if u8 is None else u8.cpu())


def _case(seed, n_slots, H, W, C, T, n_win, win):
    g = torch.Generator().manual_seed(seed)
    pool = torch.randint(0, 256, (n_slots, H, W, C), generator=g, dtype=torch.uint8)
    pool.view(-1)[:6] = torch.tensor([0, 1, 127, 128, 254, 255], dtype=torch.uint8)
    table = torch.randint(0, n_slots, (n_win, T), generator=g, dtype=torch.int32)
    table[0, 0] = 0                                                   # the frame with the six marked pixel values
    win = torch.tensor(win, dtype=torch.int64)
    return pool, table, win, pool[table[win].long()]                  # oracle: plain torch indexing


GENERAL = [(5, 7, 3, torch.float32, 4), (5, 7, 3, torch.bfloat16, 8), (5, 7, 1, torch.float32, 4), (5, 7, 1, torch.bfloat16, 8),
           (5, 7, 4, torch.float32, 4), (5, 7, 4, torch.bfloat16, 8), (5, 7, 3, torch.float32, 3), (3, 1, 3, torch.bfloat16, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,C,dtype,pitch", GENERAL)
def test_gather_general_path(hip_device, H, W, C, dtype, pitch):
    pool, table, win, want = _case(21, 11, H, W, C, 3, 6, [4, 0, 2, 0, 5])      # unaligned frames, a repeated window id
    x, u8 = _gather(hip_device, pool, table, win, dtype, pitch)
    assert torch.equal(u8, want)
    assert _same_bits(x, _want_nhwc(want.reshape(-1, H, W, C), dtype, pitch))
    x1, none = _gather(hip_device, pool, table, win, dtype, pitch, want_u8=False)
    none2, u81 = _gather(hip_device, pool, table, win, dtype, pitch, want_x=False)
    assert none is None and none2 is None and _same_bits(x1, x) and torch.equal(u81, u8)
    x0, u80 = _gather(hip_device, pool, table, torch.zeros(0, dtype=torch.int64), dtype, pitch)      # B = 0
    assert x0.numel() == 0 and u80.numel() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,T,B", [(8, 6, 3, 5), (100, 100, 9, 3)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gather_fast_path(hip_device, H, W, T, B, dtype):
    from s2p_amd._lib import chunk_elems
    pool, table, win, want = _case(22, 40, H, W, 3, T, 7, [3, 0, 6, 0, 1][:B])
    assert all(int(v) in want.unique().tolist() for v in (0, 1, 127, 128, 254, 255))
    for pitch in (chunk_elems(dtype), 2 * chunk_elems(dtype)):
        x, u8 = _gather(hip_device, pool, table, win, dtype, pitch)
        assert torch.equal(u8, want)
        assert _same_bits(x, _want_nhwc(want.reshape(-1, H, W, 3), dtype, pitch))
    x1, _ = _gather(hip_device, pool, table, win, dtype, chunk_elems(dtype), want_u8=False)
    _, u81 = _gather(hip_device, pool, table, win, dtype, chunk_elems(dtype), want_x=False)
    assert _same_bits(x1, _want_nhwc(want.reshape(-1, H, W, 3), dtype, chunk_elems(dtype))) and torch.equal(u81, want)


@pytest.mark.gpu
def test_gather_every_byte_value(hip_device):
    """All 256 values through both kernels and both dtypes: u8 / 255 is a correctly rounded division (255 -> exactly 1.0)."""
    pool = torch.arange(256, dtype=torch.uint8).repeat(3).reshape(1, 16, 16, 3)
    table, win = torch.zeros((1, 1), dtype=torch.int32), torch.zeros(1, dtype=torch.int64)
    for dtype, ce in ((torch.float32, 4), (torch.bfloat16, 8)):
        for pitch in (ce, ce + 1):                                     # a whole chunk: fast kernel; else the general one
            x, _ = _gather(hip_device, pool, table, win, dtype, pitch, want_u8=False)
            assert _same_bits(x, _want_nhwc(pool, dtype, pitch)), (dtype, pitch)


@pytest.mark.gpu
def test_gather_offsets_beyond_2_31(hip_device):
    from s2p_amd import ops
    n_slots = 75000                                                    # 2.25 GB of 100x100x3 frames, uninitialised
    g = torch.Generator().manual_seed(23)
    f0, f1 = (torch.randint(0, 256, (100, 100, 3), generator=g, dtype=torch.uint8) for _ in range(2))
    pool = torch.empty((n_slots, 100, 100, 3), dtype=torch.uint8, device=hip_device)
    pool[0].copy_(f0)
    pool[n_slots - 1].copy_(f1)
    table = torch.tensor([[0, n_slots - 1], [n_slots - 1, 0]], dtype=torch.int32, device=hip_device)
    win = torch.tensor([1, 0], dtype=torch.int64, device=hip_device)
    want = torch.stack([f1, f0, f0, f1]).reshape(2, 2, 100, 100, 3)
    for dtype, pitch in ((torch.float32, 4), (torch.bfloat16, 8), (torch.float32, 5)):
        x, u8 = ops.window_gather_u8(pool, table, win, dtype, pitch)
        assert torch.equal(u8.cpu(), want)
        assert _same_bits(x, _want_nhwc(want.reshape(-1, 100, 100, 3), dtype, pitch))


@pytest.mark.gpu
def test_random_batch_matches_the_real_reference(hip_device):
    from s2p_amd.slac_buffer import FrameBatch
    np.random.seed(R.BATCH_SEED)
    idxes = np.random.randint(low=0, high=int(G["mixed64.counts"][0]), size=R.BATCH)
    want_u8 = torch.from_numpy(G["mixed64.frames"][idxes]).permute(0, 1, 3, 4, 2).contiguous()
    assert np.array_equal(G["mixed64.frames"][idxes].astype(np.float32) / np.float32(255.0), G["batch.observations"])
    for form in ("packed", "u8", "float"):
        buf = _algo(64, hip_device, ("real", "gen"), frames=form).buffer
        np.random.seed(R.BATCH_SEED)
        for b in (buf.random_batch(R.BATCH, idxes=idxes), buf.random_batch(R.BATCH)):      # given ids; the seeded host draw
            obs = b["observations"]
            if form == "packed":
                assert isinstance(obs, FrameBatch) and obs.shape == (R.BATCH, R.S + 1, R.C, R.H, R.W)
                assert torch.equal(obs.u8.cpu(), want_u8)
                assert _same_bits(obs.nhwc, _want_nhwc(want_u8.reshape(-1, R.H, R.W, R.C), torch.float32, 4))
            elif form == "u8":
                assert torch.equal(obs.cpu(), want_u8)
            else:
                assert _same_bits(obs, torch.from_numpy(G["batch.observations"]))
            assert _same_bits(b["actions"], torch.from_numpy(G["batch.actions"]))
            assert _same_bits(b["terminals"], torch.from_numpy(G["batch.terminals"]))
            ulps = (_bits(b["rewards"]).long() - _bits(torch.from_numpy(G["batch.rewards"])).long()).abs()
            assert int(ulps.max()) <= 1
    s, a, r, d = buf.sample_latent(3, idxes=[5, 0, 36])
    assert tuple(s.shape) == (3, R.S + 1, R.C, R.H, R.W) and tuple(a.shape) == (3, R.S, R.A) and tuple(r.shape) == (3, R.S, 1) \
        and tuple(d.shape) == (3, R.S, 1)
    s, a, r, d = buf.sample_sac(3, idxes=[5, 0, 36])
    assert tuple(r.shape) == (3, 1) and tuple(d.shape) == (3, 1) and _same_bits(r, buf.reward_[[5, 0, 36], -1])


def _latent_inputs(dev, dtype, B):
    """The frames of tests/slac_latent_ref.py held by a ReplayBuffer: (FrameBatch, fp32 NCHW u8 / 255, action, reward, done, noise)."""
    import slac_latent_ref as L
    from s2p_amd.slac_buffer import ReplayBuffer
    state_u8, action, reward, done, noise = L.make_inputs()
    state_u8, action, reward, done, noise = state_u8[:B], action[:B], reward[:B], done[:B], noise[:B]
    T = L.S + 1
    frames = state_u8.permute(0, 1, 3, 4, 2).reshape(B * T, 100, 100, 3).contiguous().numpy()
    buf = ReplayBuffer(8, L.S, (3, 100, 100), (L.A,), dev, dtype=dtype, frame_capacity=B * T)
    buf.load_windows(frames, np.arange(B * T).reshape(B, T), action.numpy(), reward.numpy(), done.numpy())
    fb, a, r, d = buf.sample_latent(B, idxes=range(B))
    nchw = torch.from_numpy(state_u8.numpy().astype(np.float32) / np.float32(255.0))
    assert _same_bits(a, action) and _same_bits(r, reward.reshape(B, L.S, 1)) and _same_bits(d, done.reshape(B, L.S, 1))
    return fb, nchw, a, r, d, noise


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_encoder_reads_a_frame_batch(hip_device, dtype):
    import slac_latent_ref as L
    from s2p_amd.slac import Encoder
    enc = Encoder(dtype=dtype, device=hip_device)
    enc.load_state_dict({k[len("encoder."):]: v for k, v in L.make_params().items() if k.startswith("encoder.")})
    fb, nchw, *_ = _latent_inputs(hip_device, dtype, 2)
    with torch.no_grad():
        got, want = enc(fb), enc(nchw)
    assert tuple(got.shape) == (2, L.S + 1, 256) and float(want.abs().max()) > 0 and _same_bits(got, want)


@pytest.mark.gpu
def test_losses_from_a_frame_batch(hip_device):
    """loss_kld / loss_reward bitwise; loss_image (uint8 target against fp32 target: another kernel path and summation order) within
    the bound test_slac_latent.py::test_fp32_uint8_frames_give_the_same_losses uses for this pair of target forms."""
    import slac_latent_ref as L
    from s2p_amd.slac import LatentModel
    GL = np.load(os.path.join(HERE, "golden", "slac_latent_golden_v1.npz"))
    m = LatentModel((3, 100, 100), (L.A,), image_size=100, dtype=torch.float32, device=hip_device)
    m.load_state_dict(L.full_state_dict(L.make_params()), strict=True)
    fb, nchw, a, r, d, noise = _latent_inputs(hip_device, torch.float32, L.B)
    with torch.no_grad():
        got = m.calculate_loss(fb, a, r, d, noise)
        want = m.calculate_loss(nchw, a, r, d, noise)
    assert _same_bits(got[0], want[0]) and _same_bits(got[2], want[2])
    err = abs(float(got[1]) - float(want[1])) / abs(float(want[1]))
    bound = 4.0 * max(float(GL["losses_ref32_err"][1]), 1e-6)
    print("loss_image frame batch %r fp32 %r rel err %.3e bound %.3e" % (float(got[1]), float(want[1]), err, bound))
    assert err <= bound


@pytest.mark.gpu
def test_slac_algorithm_end_to_end(hip_device):
    from s2p_amd.slac_algo import SlacAlgorithm
    traj, rows = 2, 12
    n = traj * rows
    algo = SlacAlgorithm((3, 100, 100), (R.A,), 1, hip_device, seed=0, batch_size_latent=2, buffer_size=32, num_sequences=R.S,
                         frame_capacity=128)
    algo.load_data_in_buffer(R.real_dataset(traj, rows, 100, 100), **dict(R.LOAD_ARGS["real"], data_num=n))
    n_real = algo.buffer._n
    algo.load_data_in_buffer(R.generated_dataset(traj, rows, 100, 100), **dict(R.LOAD_ARGS["gen"], data_num=n))
    assert n_real == 2 * (rows - R.S + 1) - 1 and algo.buffer._real_n == n_real and algo.buffer._n == n_real + 2 * (rows - R.S) - 1
    before = [p.detach().clone() for p in algo.latent.parameters()]
    for _ in range(2):
        losses = algo.update_latent()
        assert len(losses) == 3 and all(bool(torch.isfinite(v)) for v in losses)
    assert algo.learning_steps_latent == 2
    assert all(not torch.equal(p, q) for p, q in zip(algo.latent.parameters(), before))
    state_, action_, _, _ = algo.buffer.sample_latent(3)
    z, next_z, action, fa, next_fa = algo.prepare_batch(state_, action_)
    assert tuple(z.shape) == (3, 288) and tuple(next_z.shape) == (3, 288) and tuple(action.shape) == (3, R.A)
    assert tuple(fa.shape) == (3, R.S * 256 + (R.S - 1) * R.A) and tuple(next_fa.shape) == tuple(fa.shape)
