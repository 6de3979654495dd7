"""s2p_decoded_to_frames (csrc/replay.hip, SPEC.md N3o) through the C ABI, bit for bit against its rule evaluated by torch on the CPU
in fp32: byte = clamp(round(v * 255), 0, 255) with a NaN as 0, x = byte / 255 (or, clamp-only, min(max(v, 0), 1) with NaN and -0.0 as
+0), bf16 by `.to(torch.bfloat16)`.  Every output is a view inside a sentinel-filled byte buffer, so a write outside it is seen, and x
starts out poisoned, so a pad channel that is not written shows."""
import pytest
import torch

from s2p_amd import _lib

pytestmark = pytest.mark.gpu
BAND, SENT = 256, 0xA5
DTYPES = {"fp32": (torch.float32, 4), "bf16": (torch.bfloat16, 8)}         # dtype, the pitch of y and x (one 16-byte chunk)


@pytest.fixture(autouse=True)
def _needs_a_device(hip_device):
    """Every test here launches the kernel: without a HIP device each is skipped, as the suite's other GPU tests are."""


def _values(n, seed):
    """n fp32 inputs: the special values, every k / 255, every tie (k + 0.5) / 255 as fp32 computes it, values below 0 and above 1
    and random ones -- all of them when n allows, else a seeded choice that keeps the special values first."""
    k = torch.arange(256, dtype=torch.float32)
    special = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0, 0.0, -1e-3, -0.5, -3.0, 1.0, 1.0 + 1e-6, 1.5, 40.0, 1e30, -1e30,
                            0.5 / 255, 254.5 / 255, 1e-40, -1e-40], dtype=torch.float32)
    g = torch.Generator().manual_seed(seed)
    pool = torch.cat([special, k / 255.0, (k + 0.5) / 255.0, torch.rand(512, generator=g) * 1.4 - 0.2])
    if n >= pool.numel():
        out = torch.cat([pool, torch.rand(n - pool.numel(), generator=g) * 1.4 - 0.2])
        return out[torch.randperm(n, generator=g)]
    rest = pool[special.numel():][torch.randperm(pool.numel() - special.numel(), generator=g)]
    return torch.cat([special, rest])[:n]


def _reference(v, quantize, dtype):
    """v fp32 [pixels, C] (the values the kernel reads, already rounded to the dtype) -> (x [pixels, C] in dtype, u8 [pixels, C])."""
    r = torch.round(v * 255.0)                                           # one fp32 multiply, ties to even
    q = torch.nan_to_num(r, nan=0.0, posinf=255.0, neginf=0.0).clamp(0.0, 255.0).to(torch.uint8)
    if quantize:
        x = q.to(torch.float32) / 255.0
    else:
        x = torch.where(v > 0, v, torch.zeros_like(v)).clamp(max=1.0)
    return x.to(dtype), q


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


class Out:
    """`nbytes` of output at byte offset `off` behind a guard band, inside a buffer filled with the sentinel byte."""

    def __init__(self, nbytes, off=0):
        self.buf = torch.full((2 * BAND + off + nbytes,), SENT, dtype=torch.uint8, device="cuda")
        self.lo, self.hi = BAND + off, BAND + off + nbytes
        self.v = self.buf[self.lo:self.hi]

    def guards_intact(self):
        return bool((self.buf[:self.lo] == SENT).all()) and bool((self.buf[self.hi:] == SENT).all())

    def untouched(self):
        return bool((self.buf == SENT).all())


def _launch(y, pixels, C, quantize, x, x_pitch, u8):
    rc = _lib.lib().s2p_decoded_to_frames(_lib.dtype_id(y.dtype), y.data_ptr(), y.shape[1], pixels, C, int(quantize),
                                          x.v.data_ptr() if x is not None else None, x_pitch, u8.v.data_ptr() if u8 is not None else None,
                                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().s2p_last_error()


def _input(pixels, C, dtype, pitch, seed):
    """y [pixels, pitch] in dtype on the device (channels >= C hold a value no output may show) and what the kernel reads, fp32."""
    y = torch.full((pixels, pitch), 0.7071, dtype=torch.float32)
    y[:, :C] = _values(pixels * C, seed).reshape(pixels, C)
    y = y.to(dtype)
    return y.cuda(), y[:, :C].to(torch.float32)


def _check(y, v, pixels, C, quantize, dtype, pitch, want_x, want_u8, u8_off=0):
    es = 4 if dtype == torch.float32 else 2
    x = Out(pixels * pitch * es) if want_x else None
    u8 = Out(pixels * C, off=u8_off) if want_u8 else None
    _launch(y, pixels, C, quantize, x, pitch, u8)
    ref_x, ref_u8 = _reference(v, quantize, dtype)
    what = (pixels, C, quantize, dtype, want_x, want_u8, u8_off)
    if want_x:
        got = x.v.view(dtype).view(pixels, pitch).cpu()
        assert x.guards_intact(), what
        assert torch.equal(_bits(got[:, :C]), _bits(ref_x)), what
        assert torch.equal(_bits(got[:, C:]), torch.zeros_like(_bits(got[:, C:]))), what           # exact zeros over the poison
    if want_u8:
        assert u8.guards_intact(), what
        assert torch.equal(u8.v.view(pixels, C).cpu(), ref_u8), what
    return x, u8


@pytest.mark.parametrize("quantize", [True, False], ids=["quantize", "clamp"])
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("pixels", [1, 5, 12, 10000])
@pytest.mark.parametrize("name", list(DTYPES))
def test_bitwise_against_the_rule(name, pixels, C, quantize):
    dtype, pitch = DTYPES[name]
    y, v = _input(pixels, C, dtype, pitch, seed=pixels + C)
    for want_x, want_u8 in ((True, True), (True, False), (False, True)):
        _check(y, v, pixels, C, quantize, dtype, pitch, want_x, want_u8)
    if pixels == 10000 and C == 3:
        # what the large case is there for: its bytes take all 256 values, inputs sit exactly on a tie (every fp32 (k + 0.5) / 255
        # does; in bf16 0.5 and -0.5 are left), and there are NaN, infinities and -0.0 among them
        assert len(torch.unique(_reference(v, True, dtype)[1])) == 256
        t = v * 255.0
        assert int(((t - torch.floor(t)) == 0.5).sum()) >= (200 if dtype == torch.float32 else 1)
        assert bool(torch.isnan(v).any()) and bool(torch.isinf(v).any()) and bool(((v == 0) & torch.signbit(v)).any())


@pytest.mark.parametrize("quantize", [True, False], ids=["quantize", "clamp"])
@pytest.mark.parametrize("name", list(DTYPES))
def test_u8_out_at_an_odd_byte_offset_takes_the_slow_form(name, quantize):
    dtype, pitch = DTYPES[name]
    for pixels in (12, 10000):
        y, v = _input(pixels, 3, dtype, pitch, seed=77)
        _check(y, v, pixels, 3, quantize, dtype, pitch, True, True, u8_off=1)
        _check(y, v, pixels, 3, quantize, dtype, pitch, False, True, u8_off=3)


@pytest.mark.parametrize("name", list(DTYPES))
def test_wider_pitches_and_an_output_not_asked_for(name):
    """y and x with two chunks per pixel (the fast form zeroes the second chunk of x, reads only the first of y); an output that is
    NULL is not written: a sentinel buffer of its size beside the call stays whole."""
    dtype, ce = DTYPES[name]
    pixels, C, pitch = 12, 3, 2 * ce
    y, v = _input(pixels, C, dtype, pitch, seed=5)
    _check(y, v, pixels, C, True, dtype, pitch, True, True)
    spare = Out(pixels * C)
    _check(y, v, pixels, C, True, dtype, pitch, True, False)
    assert spare.untouched()


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("pixels", [5, 12, 10000])
@pytest.mark.parametrize("name", list(DTYPES))
def test_x_is_what_the_replay_buffer_gathers_for_the_same_bytes(name, pixels, C):
    """The kernel's own u8_out as a one-window, one-frame pool of s2p_window_gather_u8: its x equals the kernel's x bit for bit."""
    dtype, pitch = DTYPES[name]
    es = 4 if dtype == torch.float32 else 2
    y, v = _input(pixels, C, dtype, pitch, seed=31)
    x, u8 = _check(y, v, pixels, C, True, dtype, pitch, True, True)
    table = torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    win = torch.zeros(1, dtype=torch.int64, device="cuda")
    gx = Out(pixels * pitch * es)
    rc = _lib.lib().s2p_window_gather_u8(_lib.dtype_id(dtype), u8.v.data_ptr(), 1, pixels, C, table.data_ptr(), 1, win.data_ptr(), 1,
                                         gx.v.data_ptr(), pitch, None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and gx.guards_intact()
    assert torch.equal(gx.v.cpu(), x.v.cpu())


def test_ops_wrapper_writes_both_forms():
    from s2p_amd import ops
    g = torch.Generator().manual_seed(3)
    y = (torch.rand(2, 6, 6, 4, generator=g) * 1.4 - 0.2).cuda()
    x, u8 = torch.full((2, 6, 6, 4), 9.0, device="cuda"), torch.zeros((2, 6, 6, 3), dtype=torch.uint8, device="cuda")
    rx, ru = ops.decoded_to_frames(y, 3, True, x=x, u8_out=u8)
    assert rx is x and ru is u8
    ref_x, ref_u8 = _reference(y.cpu().reshape(72, 4)[:, :3], True, torch.float32)
    assert torch.equal(u8.cpu().reshape(72, 3), ref_u8) and torch.equal(_bits(x.cpu().reshape(72, 4)[:, :3]), _bits(ref_x))
    assert float(x[..., 3].abs().max()) == 0.0
    with pytest.raises(ValueError):
        ops.decoded_to_frames(y, 3, True, x=x[..., :2])
    with pytest.raises(RuntimeError):
        ops.decoded_to_frames(y, 3, True)
