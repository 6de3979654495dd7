"""Kernel-level tests of csrc/actor.hip through the C ABI (SPEC.md N3f): the uint8 CHW -> NHWC [0, 1] conversion (bitwise against
torch's `.float().div(255)`), the feature / action push (bitwise against a numpy deque model) and the skinny grouped linear layer
(against the fp64 product at the project's rule of tests/test_ensemble_train_gpu.py -- K_TOL x max(err of torch's own fp32 matmul
on the CPU, 1e-6), K_TOL = 4 -- plus the bitwise properties: row invariance and repeatability).  Outputs live in the sentinel-guarded
regions of tests/guard_region.py; every refusal is checked to have written nothing."""
import math
from collections import deque

import numpy as np
import pytest
import torch

from guard_region import Region

pytestmark = pytest.mark.gpu
K_TOL, FLOOR = 4.0, 1e-6
F32, BF16, ACT_NONE, ACT_RELU = 0, 1, 0, 1


def _L():
    from s2p_amd import _lib
    return _lib


def _st():
    return torch.cuda.current_stream().cuda_stream


def _rel_max(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


# ---- s2p_u8_chw_to_nhwc01 -------------------------------------------------------------------------------------------------------------
def _frames(offset=0, N=2, C=3, H=5, W=7):
    """Bytes counting up from `offset` (mod 256).  A 2 x 3 x 5 x 7 block holds 210 bytes, so the tests run two of them, from 0 and from
    46: all 256 byte values occur."""
    n = N * C * H * W
    return torch.arange(n, dtype=torch.int64).add(offset).remainder(256).to(torch.uint8).reshape(N, C, H, W)


@pytest.mark.parametrize("dtype,pitch", [(torch.float32, 4), (torch.bfloat16, 8), (torch.float32, 3), (torch.bfloat16, 5)])
def test_u8_chw_to_nhwc01_bitwise(hip_device, dtype, pitch):
    """N 2, C 3, H 5, W 7 (35 pixels per plane: the byte-wise kernel) and H 6, W 6 (36: the dword kernel), every byte value in each;
    fp32 bitwise `x.float().div(255)` permuted, bf16 bitwise that `.to(bfloat16)`; the pad exactly 0 over a NaN fill."""
    L = _L()
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    for H, W in ((5, 7), (6, 6)):
        seen = set()
        for offset in (0, 46):
            x = _frames(offset, 2, 3, H, W)
            seen |= set(x.view(-1).tolist())
            want = x.float().div(255).permute(0, 2, 3, 1).contiguous()              # [N,H,W,C] fp32
            xd = x.to(hip_device)
            elems = 2 * H * W * pitch
            if dtype == torch.float32:
                reg = Region(2 * H * W, pitch, pitch=pitch, fill=torch.full((2 * H * W, pitch), float("nan")))
                L.check(L.lib().s2p_u8_chw_to_nhwc01(F32, xd.data_ptr(), 2, 3, H, W, reg.ptr, pitch, _st()), "u8")
                got = reg.bits("u8_chw fp32").view(2, H, W, pitch)
            else:
                buf = torch.full((elems + 512,), float("nan"), dtype=torch.bfloat16, device=hip_device)
                y = buf[256:256 + elems]
                L.check(L.lib().s2p_u8_chw_to_nhwc01(BF16, xd.data_ptr(), 2, 3, H, W, y.data_ptr(), pitch, _st()), "u8")
                torch.cuda.synchronize()
                assert bool(buf[:256].isnan().all()) and bool(buf[256 + elems:].isnan().all()), "guard band overwritten"
                got = y.cpu().view(2, H, W, pitch)
                want = want.to(torch.bfloat16)
            assert torch.equal(got[..., :3].contiguous().view(bits), want.view(bits)), (H, W, offset)
            assert bool((got[..., 3:] == 0).all()) and not bool(got.float().isnan().any())    # the pad: exactly 0 over the NaN fill
        assert len(seen) == 256


def test_u8_chw_to_nhwc01_arguments(hip_device):
    L = _L()
    x = _frames().to(hip_device)
    reg = Region(70, 4, pitch=4)
    fn = L.lib().s2p_u8_chw_to_nhwc01
    assert fn(F32, None, 0, 3, 5, 7, None, 4, _st()) == 0                          # N = 0: a no-op that looks at no pointer
    assert fn(F32, None, 2, 3, 0, 7, None, 4, _st()) == 0
    assert fn(F32, x.data_ptr(), 2, 3, 5, 7, reg.ptr, 2, _st()) != 0                # a short pitch
    assert b"pitch" in L.lib().s2p_last_error()
    assert fn(F32, x.data_ptr(), -1, 3, 5, 7, reg.ptr, 4, _st()) != 0
    assert fn(F32, None, 2, 3, 5, 7, reg.ptr, 4, _st()) != 0
    assert fn(F32, x.data_ptr(), 2, 3, 5, 7, None, 4, _st()) != 0
    assert fn(7, x.data_ptr(), 2, 3, 5, 7, reg.ptr, 4, _st()) != 0
    assert reg.untouched()


# ---- s2p_feature_action_push ------------------------------------------------------------------------------------------------------------
class _DequeModel:
    """`SlacObservation` per row in numpy: deques of S features and S - 1 actions."""

    def __init__(self, N, S, F, A):
        self.N, self.S, self.F, self.A = N, S, F, A
        self.f = [deque([np.zeros(F, np.float32)] * S, maxlen=S) for _ in range(N)]
        self.a = [deque([np.zeros(A, np.float32)] * (S - 1), maxlen=S - 1) for _ in range(N)]

    def step(self, feat, action, code, fill):
        for n in range(self.N):
            if code[n] == 0:
                self.f[n].append(feat[n]); self.a[n].append(action[n])
            else:
                first = fill if code[n] == 1 else feat[n]
                self.f[n] = deque([first] * (self.S - 1) + [feat[n]], maxlen=self.S)
                self.a[n] = deque([np.zeros(self.A, np.float32)] * (self.S - 1), maxlen=self.S - 1)

    def rows(self):
        return np.stack([np.concatenate(list(self.f[n]) + list(self.a[n])) for n in range(self.N)])


@pytest.mark.parametrize("A", [2, 3])
def test_feature_action_push_bitwise(hip_device, A):
    """N 3, S 3, F 8: A 2 gives an unpadded row (28), A 3 a padded one (30 in a pitch of 32).  6 steps, reset codes 0 / 1 / 2 mixed per
    row and per step; every step bitwise the deque model, `src` unchanged, the pad 0, the guards untouched."""
    L = _L()
    N, S, F = 3, 3, 8
    P = S * F + (S - 1) * A
    pitch = (P + 3) // 4 * 4
    g = torch.Generator().manual_seed(40 + A)
    codes = [[1, 2, 1], [0, 0, 0], [0, 1, 0], [2, 0, 0], [0, 0, 1], [0, 2, 0]]
    model = _DequeModel(N, S, F, A)
    fill = torch.randn(F, generator=g)
    # start from rows full of junk, pad included: the first step resets every row and must leave the pad 0
    regs = [Region(N, pitch, pitch=pitch, fill=torch.randn(N, pitch, generator=g)) for _ in range(2)]
    fill_d = fill.to(hip_device)
    cur = 0
    for step, code in enumerate(codes):
        feat, action = torch.randn(N, F + 4, generator=g), torch.randn(N, A + 1, generator=g)      # pitches wider than the rows
        feat_d, act_d = feat.to(hip_device), action.to(hip_device)
        code_d = torch.tensor(code, dtype=torch.int32, device=hip_device)
        src, dst = regs[cur], regs[1 - cur]
        before = src.bits("src before")
        L.check(L.lib().s2p_feature_action_push(src.ptr, dst.ptr, pitch, N, S, F, A, feat_d.data_ptr(), F + 4, act_d.data_ptr(), A + 1,
                                                code_d.data_ptr(), fill_d.data_ptr(), _st()), "push")
        model.step(feat[:, :F].numpy(), action[:, :A].numpy(), code, fill.numpy())
        got = dst.bits("push step %d" % step).numpy()
        assert np.array_equal(got[:, :P].view(np.int32), model.rows().view(np.int32)), step
        assert (got[:, P:] == 0).all()
        assert torch.equal(src.bits("src after"), before)
        cur = 1 - cur
    # reset == NULL is an append for every row
    feat, action = torch.randn(N, F, generator=g), torch.randn(N, A, generator=g)
    src, dst = regs[cur], regs[1 - cur]
    feat_d, act_d = feat.to(hip_device), action.to(hip_device)
    L.check(L.lib().s2p_feature_action_push(src.ptr, dst.ptr, pitch, N, S, F, A, feat_d.data_ptr(), F, act_d.data_ptr(), A, None, None,
                                            _st()), "push")
    model.step(feat.numpy(), action.numpy(), [0, 0, 0], fill.numpy())
    assert np.array_equal(dst.bits("append").numpy()[:, :P].view(np.int32), model.rows().view(np.int32))


def test_feature_action_push_arguments(hip_device):
    L = _L()
    N, S, F, A, pitch = 3, 3, 8, 2, 28
    src, dst = Region(N, pitch, pitch=pitch), Region(N, pitch, pitch=pitch)
    feat, act = torch.zeros(N, F, device=hip_device), torch.zeros(N, A, device=hip_device)
    code, fill = torch.zeros(N, dtype=torch.int32, device=hip_device), torch.zeros(F, device=hip_device)
    fn = L.lib().s2p_feature_action_push

    def call(s=src.ptr, d=dst.ptr, p=pitch, n=N, fp=F, ap=A, f=feat.data_ptr(), a=act.data_ptr(), c=code.data_ptr(), fl=fill.data_ptr()):
        return fn(s, d, p, n, S, F, A, f, fp, a, ap, c, fl, _st())

    assert call(s=None, d=None, n=0, f=None, a=None, c=None, fl=None) == 0          # N = 0: a no-op that looks at no pointer
    assert call(d=src.ptr) != 0 and b"overlap" in L.lib().s2p_last_error()          # src == dst
    assert call(d=src.ptr + 16) != 0                                                # ... or any overlap
    assert call(p=24) != 0 and call(fp=F - 1) != 0 and call(ap=A - 1) != 0          # short pitches
    assert call(p=30) != 0                                                          # a pitch that is no multiple of 4
    assert call(n=-1) != 0 and call(s=None) != 0 and call(d=None) != 0 and call(f=None) != 0 and call(a=None) != 0
    assert call(fl=None) != 0                                                       # reset codes without the fill vector
    assert call(s=src.ptr + 4) != 0                                                 # misaligned
    assert src.untouched() and dst.untouched()


# ---- s2p_mlp_linear_fwd_skinny ------------------------------------------------------------------------------------------------------------
class _Layer:
    """One group's host data and device copies: x [rows][K] in a wider pitch, w [N][K], bias; outputs in guarded regions."""

    def __init__(self, rows, K, N, dev, g, pre=True, act=True):
        self.rows, self.K, self.N = rows, K, N
        self.x = torch.randn(rows, K, generator=g)
        self.w = torch.randn(N, K, generator=g) / math.sqrt(K)
        self.b = torch.randn(N, generator=g) * 0.1
        self.xp = K + 4
        xd = torch.zeros(max(rows, 1), self.xp)
        xd[:rows, :K] = self.x
        self.xd, self.wd, self.bd = xd.to(dev), self.w.contiguous().to(dev), self.b.to(dev)
        self.pre = Region(max(rows, 1), N, pitch=N + 3) if pre else None
        self.act = Region(max(rows, 1), N, pitch=N + 3) if act else None

    def group(self, L, rows=None, row0=0, pre=None, act=None):
        pre, act = pre or self.pre, act or self.act
        return L.MlpFwdGroup(self.xd[row0:].data_ptr(), self.wd.data_ptr(), self.bd.data_ptr(), pre.ptr if pre else None,
                             act.ptr if act else None, self.xp, (pre or act).pitch, self.rows if rows is None else rows, self.K)

    def refs(self):
        f64 = self.x.double() @ self.w.double().t() + self.b.double()
        f32 = self.x @ self.w.t() + self.b
        return f64, f32


def _run(L, groups, N, act):
    tab = (L.MlpFwdGroup * len(groups))(*groups)
    return L.lib().s2p_mlp_linear_fwd_skinny(tab, len(groups), N, act, _st())


def _check(got, f64, f32, what):
    err, ref = _rel_max(got, f64), max(_rel_max(f32, f64), FLOOR)
    print("%-40s err %.3e  ref32_err %.3e  ratio %.3f" % (what, err, ref, err / ref))
    assert err <= K_TOL * ref, (what, err, K_TOL * ref)


@pytest.mark.parametrize("N", [1, 12, 65])
@pytest.mark.parametrize("K", [4, 52, 260, 2092])
def test_skinny_against_fp64(hip_device, K, N):
    """rows 1 / 5 / 16, ReLU and none, `pre` and / or `act`; K = 260 crosses the 256-wide lane stride, N = 65 the four waves of a
    workgroup."""
    L = _L()
    g = torch.Generator().manual_seed(1000 + K + N)
    for rows in (1, 5, 16):
        for act, (want_pre, want_act) in ((ACT_RELU, (True, True)), (ACT_NONE, (False, True)), (ACT_RELU, (True, False))):
            ly = _Layer(rows, K, N, hip_device, g, want_pre, want_act)
            L.check(_run(L, [ly.group(L)], N, act), "skinny")
            f64, f32 = ly.refs()
            what = "rows %d K %d N %d act %d" % (rows, K, N, act)
            if want_pre:
                _check(ly.pre.get(what), f64, f32, what + " pre")
            if want_act:
                relu = (lambda v: v.clamp(min=0)) if act == ACT_RELU else (lambda v: v)
                _check(ly.act.get(what), relu(f64), relu(f32), what + " act")


def test_skinny_two_groups_of_unequal_shape(hip_device):
    """G = 3: K 52 on 5 rows, K 260 on 16 rows, and a group of 0 rows whose pointers are never looked at."""
    L = _L()
    g = torch.Generator().manual_seed(7)
    a, b = _Layer(5, 52, 12, hip_device, g), _Layer(16, 260, 12, hip_device, g)
    empty = L.MlpFwdGroup(None, None, None, None, None, 0, 0, 0, 52)
    L.check(_run(L, [a.group(L), empty, b.group(L)], 12, ACT_RELU), "skinny")
    for ly, name in ((a, "group 0"), (b, "group 2")):
        f64, f32 = ly.refs()
        _check(ly.pre.get(name), f64, f32, name + " pre")
        _check(ly.act.get(name), f64.clamp(min=0), f32.clamp(min=0), name + " act")


@pytest.mark.parametrize("K,N", [(2092, 65), (260, 12)])
def test_skinny_row_invariance_and_repeatability(hip_device, K, N):
    """Every row of the 16-row launch (and of a 5- and a 3-row launch: the other two instantiations) is BITWISE its own 1-row launch;
    two identical calls are bitwise equal."""
    L = _L()
    g = torch.Generator().manual_seed(3)
    ly = _Layer(16, K, N, hip_device, g, pre=True, act=False)
    L.check(_run(L, [ly.group(L)], N, ACT_NONE), "skinny")
    full = ly.pre.bits("16 rows")
    again = Region(16, N, pitch=N + 3)
    L.check(_run(L, [ly.group(L, pre=again)], N, ACT_NONE), "skinny")
    assert torch.equal(again.bits("again").view(torch.int32), full.view(torch.int32))
    for r in range(16):
        one = Region(1, N, pitch=N + 3)
        L.check(_run(L, [ly.group(L, rows=1, row0=r, pre=one)], N, ACT_NONE), "skinny")
        assert torch.equal(one.bits("row %d" % r)[0].view(torch.int32), full[r].view(torch.int32)), r
    for rows in (5, 3):
        part = Region(rows, N, pitch=N + 3)
        L.check(_run(L, [ly.group(L, rows=rows, row0=2, pre=part)], N, ACT_NONE), "skinny")
        assert torch.equal(part.bits("%d rows" % rows).view(torch.int32), full[2:2 + rows].view(torch.int32)), rows


def test_skinny_arguments(hip_device):
    L = _L()
    g = torch.Generator().manual_seed(5)
    ly = _Layer(16, 52, 12, hip_device, g)
    big = _Layer(17, 52, 12, hip_device, g)
    ok = ly.group(L)
    assert _run(L, [ok], 0, ACT_RELU) == 0 and L.lib().s2p_mlp_linear_fwd_skinny(None, 0, 12, ACT_RELU, _st()) == 0
    assert _run(L, [ok, big.group(L)], 12, ACT_RELU) != 0 and b"17 rows" in L.lib().s2p_last_error()      # refused before ANY launch
    bad_k = ly.group(L); bad_k.K = 50
    bad_w = ly.group(L); bad_w.w = ly.wd.data_ptr() + 4
    bad_x = ly.group(L); bad_x.x = ly.xd.data_ptr() + 8
    short = ly.group(L); short.y_pitch = 11
    null = ly.group(L); null.bias = None
    neg = ly.group(L); neg.rows = -1
    for bad in (bad_k, bad_w, bad_x, short, null, neg):
        assert _run(L, [ok, bad], 12, ACT_RELU) != 0
    assert _run(L, [ok], 12, 3) != 0 and _run(L, [ok] * 9, 12, ACT_RELU) != 0 and _run(L, [ok], -1, ACT_RELU) != 0
    assert ly.pre.untouched() and ly.act.untouched() and big.pre.untouched() and big.act.untouched()
