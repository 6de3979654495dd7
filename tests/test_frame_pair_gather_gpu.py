"""s2p_frame_pair_gather (csrc/replay.hip, SPEC.md N1d) through the C ABI, bit for bit against what the host path computes on the CPU:
`images_to_tensor` (`.float() / 127.5 - 1.0`, `F.interpolate(mode="nearest")`) of frames t and t + 1 and row t + 1 of the states.
The pool sits at a chosen byte offset inside a larger allocation filled with a sentinel byte, so a read outside it shows as a wrong
value and not as a fault; every output is a guard_region.Region, so a write outside it is seen."""
import numpy as np
import pytest
import torch

from guard_region import Region
from s2p_amd import _lib
from s2p_amd.data import images_to_tensor

pytestmark = pytest.mark.gpu
PAD, SENT_BYTE = 1024, 0xA5


def _frames(n, H, W, C, seed):
    """Random uint8 [n,H,W,C]; a frame of at least 256 bytes holds every byte value."""
    r = np.random.RandomState(seed)
    f = r.randint(0, 256, size=(n, H * W * C)).astype(np.uint8)
    if H * W * C >= 256:
        for k in range(n):
            f[k, r.permutation(H * W * C)[:256]] = np.arange(256, dtype=np.uint8)
    return f.reshape(n, H, W, C)


def _bits(t):
    return t.contiguous().view(torch.int32)


class Case:
    """One launch: operands on the device, outputs in Regions, the CPU reference beside them."""

    def __init__(self, n, H, W, C, size, idx, S=17, pool_off=0, out_off=0, want_image=True, want_state=True, seed=0):
        self.n, self.H, self.W, self.C, self.S, self.size = n, H, W, C, S, size
        self.frames = _frames(n, H, W, C, seed)
        self.states = np.random.RandomState(seed + 1).randn(n, S).astype(np.float32)
        self.idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        B, (oh, ow) = len(self.idx), (size if size is not None else (H, W))
        self.B, self.oh, self.ow = B, oh, ow
        raw = torch.full((2 * PAD + pool_off + self.frames.size,), SENT_BYTE, dtype=torch.uint8, device="cuda")
        self.raw = raw
        self.pool = raw[PAD + pool_off:PAD + pool_off + self.frames.size]
        self.pool.copy_(torch.from_numpy(self.frames.reshape(-1)))
        sraw = torch.full((2 * PAD + n * S,), 7.5e33, dtype=torch.float32, device="cuda")
        self.sraw = sraw
        self.dstates = sraw[PAD:PAD + n * S]
        self.dstates.copy_(torch.from_numpy(self.states.reshape(-1)))
        self.didx = torch.from_numpy(self.idx).cuda()
        self.prev = Region(1, max(B * C * oh * ow, 1), off=out_off)
        self.image = Region(1, max(B * C * oh * ow, 1), off=out_off) if want_image else None
        self.state = Region(1, max(B * S, 1), off=out_off) if want_state else None

    def launch(self, **over):
        a = dict(pool=self.pool.data_ptr(), n=self.n, H=self.H, W=self.W, C=self.C, states=self.dstates.data_ptr(), S=self.S,
                 idx=self.didx.data_ptr() if self.B else None, B=self.B, oh=self.oh, ow=self.ow, prev=self.prev.ptr,
                 image=self.image.ptr if self.image else None, state=self.state.ptr if self.state else None)
        a.update(over)
        rc = _lib.lib().s2p_frame_pair_gather(a["pool"], a["n"], a["H"], a["W"], a["C"], a["states"], a["S"], a["idx"], a["B"], a["oh"],
                                              a["ow"], a["prev"], a["image"], a["state"], torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    def reference(self):
        """(prev, image) fp32 [B,C,oh,ow] and state [B,S] of the host path; rows out of range are zeros."""
        if self.size is None:
            allf = images_to_tensor(self.frames)
        else:
            assert self.oh == self.ow
            allf = images_to_tensor(self.frames, self.oh)
        assert tuple(allf.shape) == (self.n, self.C, self.oh, self.ow)
        ok = (self.idx >= 0) & (self.idx + 1 < self.n)
        t = torch.from_numpy(np.where(ok, self.idx, 0))
        m = torch.from_numpy(ok)
        prev = allf[t] * m.view(-1, 1, 1, 1)
        image = allf[t + 1] * m.view(-1, 1, 1, 1)
        state = torch.from_numpy(self.states)[t + 1] * m.view(-1, 1)
        z = lambda x: torch.where(x == 0, torch.zeros_like(x), x)               # a masked row is +0, never -0
        return z(prev), z(image), z(state), ok

    def check(self, what):
        assert self.launch() == 0, _lib.lib().s2p_last_error()
        prev, image, state, ok = self.reference()
        shape = (self.B, self.C, self.oh, self.ow)
        got = self.prev.bits(what + " prev").view(shape)
        assert torch.equal(_bits(got), _bits(prev)), what + " prev"
        if self.image is not None:
            got = self.image.bits(what + " image").view(shape)
            assert torch.equal(_bits(got), _bits(image)), what + " image"
        if self.state is not None:
            got = self.state.bits(what + " state").view(self.B, self.S)
            assert torch.equal(_bits(got), _bits(state)), what + " state"          # int32 bit patterns
        # the operands are as they were
        assert bool((self.raw[:PAD] == SENT_BYTE).all()) and np.array_equal(self.pool.cpu().numpy(), self.frames.reshape(-1))
        return ok


def test_all_byte_values_without_resize(hip_device):
    c = Case(5, 16, 16, 3, None, [0, 3, 1, 2])
    assert all(len(np.unique(f)) == 256 for f in c.frames)
    c.check("16x16 C3")
    # the value rule itself, on the CPU reference: two roundings, 255 -> exactly 1, 0 -> exactly -1
    v = images_to_tensor(np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1))
    assert float(v.max()) == 1.0 and float(v.min()) == -1.0


@pytest.mark.parametrize("H,W,out,n", [(25, 25, 20, 4), (12, 12, 20, 4), (10, 14, 12, 4), (100, 100, 84, 2)],
                         ids=["25to20", "12to20", "10x14to12", "100to84"])
def test_nearest_resize(hip_device, H, W, out, n):
    c = Case(n, H, W, 3, (out, out), list(range(n - 1)), seed=H)
    c.check("%dx%d -> %d" % (H, W, out))


OFF_CASES = [
    ("W18", dict(H=16, W=18, C=3, size=None)),                    # out_w % 4 != 0, two blocks a frame
    ("W18to20", dict(H=16, W=18, C=3, size=(20, 20))),            # (still the 4-pixel path: source rows of 54 bytes, no dword multiple)
    ("W15to20", dict(H=5, W=15, C=3, size=(20, 20))),             # 225-byte frames: the later frames start on no dword
    ("C1", dict(H=16, W=16, C=1, size=None)),
    ("C4", dict(H=16, W=16, C=4, size=None)),
    ("C1to20", dict(H=12, W=12, C=1, size=(20, 20))),
    ("pool+1", dict(H=16, W=16, C=3, size=None, pool_off=1)),
    ("pool+1to20", dict(H=25, W=25, C=3, size=(20, 20), pool_off=1)),
    ("out+4", dict(H=16, W=16, C=3, size=None, out_off=1)),       # outputs 4-byte but not 16-byte aligned
    ("out+4to20", dict(H=25, W=25, C=3, size=(20, 20), out_off=3)),
]


@pytest.mark.parametrize("name,kw", OFF_CASES, ids=[c[0] for c in OFF_CASES])
def test_shapes_and_alignments_off_the_production_case(hip_device, name, kw):
    Case(4, idx=[2, 0, 1], seed=11, **kw).check(name)


STRIDE_CASES = [
    ("rgb4_same", dict(n=2, H=264, W=256, C=3, size=None, idx=[0])),           # 16 896 quads a frame > 64 blocks x 256
    ("rgb4_resize", dict(n=2, H=100, W=100, C=3, size=(264, 256), idx=[0])),
    ("general", dict(n=2, H=130, W=130, C=1, size=None, idx=[0])),             # 16 900 pixels a frame > 64 blocks x 256
]


@pytest.mark.parametrize("name,kw", STRIDE_CASES, ids=[c[0] for c in STRIDE_CASES])
def test_grid_stride_loops(hip_device, name, kw):
    c = Case(seed=5, **kw)
    if c.size is not None:                       # (a non-square target: the reference resizes with F.interpolate directly)
        allf = torch.nn.functional.interpolate(images_to_tensor(c.frames), size=c.size, mode="nearest").contiguous()
        assert c.launch() == 0
        shape = (1, 3) + tuple(c.size)
        assert torch.equal(_bits(c.prev.bits(name).view(shape)), _bits(allf[0:1]))
        assert torch.equal(_bits(c.image.bits(name).view(shape)), _bits(allf[1:2]))
    else:
        c.check(name)


def test_more_rows_than_the_grid_has_planes(hip_device):
    """B > 65535: blockIdx.z strides over the batch."""
    n, B = 7, 65536 + 9
    idx = np.random.RandomState(2).randint(0, n - 1, size=B)
    Case(n, 2, 2, 1, None, idx, S=1).check("B 65545")


def test_index_handling(hip_device):
    n = 6
    Case(n, 16, 16, 3, None, [1, 1, 4, 1, 4, 0]).check("duplicates")
    Case(n, 16, 16, 3, None, [n - 2]).check("t = n_frames - 2, B 1")
    Case(n, 25, 25, 3, (20, 20), [n - 2, 0]).check("t = n_frames - 2, resized")
    for bad in (-1, n - 1, n):                                          # zero rows; the neighbouring rows stay right
        for kw in (dict(), dict(size=(20, 20)), dict(out_off=1)):
            c = Case(n, 16, 16, 3, kw.get("size"), [2, bad, 3, 0], out_off=kw.get("out_off", 0))
            ok = c.check("t = %d %s" % (bad, kw))
            assert ok.tolist() == [True, False, True, True]
    c = Case(n, 16, 16, 3, None, [-(2 ** 40), 2 ** 40, 0])               # far outside: nothing is dereferenced
    assert c.check("far outside").tolist() == [False, False, True]


def test_empty_batch_touches_nothing(hip_device):
    c = Case(4, 16, 16, 3, None, [])
    assert c.launch() == 0
    assert c.launch(pool=None, states=None, prev=None, image=None, state=None) == 0
    assert c.prev.untouched() and c.image.untouched() and c.state.untouched()


def test_nullable_outputs(hip_device):
    for kw in (dict(want_image=False), dict(want_state=False), dict(want_image=False, want_state=False)):
        Case(4, 16, 16, 3, None, [2, 0], **kw).check("null %s" % sorted(kw))
        Case(4, 25, 25, 3, (20, 20), [2, 0], **kw).check("null, resized %s" % sorted(kw))
        Case(4, 16, 18, 1, None, [2, 0], **kw).check("null, general %s" % sorted(kw))
    c = Case(4, 16, 16, 3, None, [2, 0], S=17)
    assert c.launch(S=0, states=None) == 0 and c.state.untouched()       # S == 0: there is no state to write


@pytest.mark.parametrize("S", [17, 1])
def test_state_rows(hip_device, S):
    Case(9, 4, 4, 3, None, [7, 0, 3, 3], S=S).check("S %d" % S)
    Case(9, 4, 4, 3, None, [7, 0, 3, 3], S=S, out_off=1).check("S %d, offset" % S)


def test_refusals_launch_nothing(hip_device):
    c = Case(4, 16, 16, 3, None, [2, 0])
    L = _lib.lib()
    cases = {"negative n_frames": dict(n=-1), "negative H": dict(H=-1), "negative W": dict(W=-1), "negative S": dict(S=-1),
             "negative B": dict(B=-1), "negative out_h": dict(oh=-1), "negative out_w": dict(ow=-1), "C 0": dict(C=0),
             "null pool": dict(pool=None), "null idx": dict(idx=None), "null prev": dict(prev=None), "null states": dict(states=None),
             "misaligned prev": dict(prev=c.prev.ptr + 2), "misaligned image": dict(image=c.image.ptr + 1),
             "misaligned state": dict(state=c.state.ptr + 3), "empty frame": dict(W=0)}
    for name, kw in cases.items():
        rc = c.launch(**kw)
        assert rc != 0 and L.s2p_last_error().decode().startswith("s2p_frame_pair_gather:"), name
        assert c.prev.untouched() and c.image.untouched() and c.state.untouched(), name
    c.check("after the refusals")
