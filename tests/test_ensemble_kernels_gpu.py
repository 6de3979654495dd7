"""Kernel-level parity of the ensemble dynamics family through the C ABI against float64 torch on the CPU: s2p_ensemble_linear_fwd /
_bwd (Swish) and s2p_ensemble_nll (csrc/ensemble_train.hip), s2p_ensemble_head (csrc/misc.hip).  The model-level modules reach them at
one configuration (D 18, K 24); here: the ends of the accepted D range, k tails past the 64-wide tile, a member table that is not
increasing, the three x forms (shared, per member, chained from a previous layer), every optional output alone, saturating log-stds
and Swish derivatives, refusals, no-ops and bitwise repeatability.  Every tensor is a pitched, column-offset view inside a
sentinel-filled buffer (guard_region.Region): no byte outside a declared view may change, and the [E] slots of dw / db that a call does
not list keep their sentinel bits.

Reference: the same formula in float64 torch (plain matmuls, F.softplus through oracle/ensemble_oracle.py's soft_clamp, autograd for
the gradients; the head's post-processing is ensemble_oracle.rollout_postprocess).  Tolerance: the project's rule
(tests/test_ensemble_train_gpu.py) -- per quantity K_TOL x max(ref32_err, 1e-6), K_TOL = 4, ref32_err being the deviation of the SAME
formula run in fp32 torch on the CPU from its fp64 run, both relative to the fp64 maximum.  Worst observed ratios: DESIGN.md section
6b.7 (printed by test_zz_report_worst_ratios)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import ensemble_oracle as O
from ensemble_train_ref import rel_max
from guard_region import SENT, Region

pytestmark = pytest.mark.gpu
K_TOL, FLOOR = 4.0, 1e-6
WORST = {}
SENT32 = float(torch.tensor(SENT, dtype=torch.float32))
F64, F32 = torch.float64, torch.float32


def _check(group, got, f64, f32, what=""):
    assert bool(torch.isfinite(torch.as_tensor(got)).all()), (group, what)
    err, ref = rel_max(got, f64), max(rel_max(f32, f64), FLOOR)
    WORST[group] = max(WORST.get(group, 0.0), err / ref)
    print("%-16s %-46s err %.3e  ref32_err %.3e  ratio %.3f" % (group, what, err, ref, err / ref))
    assert err <= K_TOL * ref, (group, what, err, K_TOL * ref)


def _L():
    from s2p_amd import _lib
    return _lib


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(r):
    return None if r is None else r.ptr


def _member(m):
    return None if m is None else (ctypes.c_int32 * len(m))(*m)


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x.bits(), y.bits()) for x, y in zip(a, b))


# ---- s2p_ensemble_linear_fwd / s2p_ensemble_linear_bwd -----------------------------------------------------------------------------------
class Layer:
    """One grouped layer: host data (fp32) and guarded device views.  x in one of the three forms of the header; its last two columns
    are the zero padding of an input width that is no multiple of 4 (K > 4); pre_prev holds +-30 and +-100."""

    def __init__(self, G, E, member, B, K, N, form, seed):
        g = torch.Generator().manual_seed(seed)
        self.G, self.E, self.B, self.K, self.N, self.member = G, E, B, K, N, member
        self.mem = list(member) if member is not None else list(range(G))
        self.k_real = K - 2 if K > 4 else K
        x = torch.randn(1 if form == "shared" else G, B, K, generator=g)
        x[..., self.k_real:] = 0
        self.x = x.expand(G, B, K).contiguous()
        self.w = torch.randn(E, N, K, generator=g) / math.sqrt(K)
        self.b = torch.randn(E, N, generator=g) * 0.1
        self.dpre = torch.randn(G, B, N, generator=g)
        self.pre_prev = torch.randn(G, B, K, generator=g)
        for (gi, bi, ki), v in zip(((0, 0, 0), (G - 1, B - 1, K - 1), (0, B // 2, 1), (G - 1, 0, 2)), (30.0, -30.0, 100.0, -100.0)):
            self.pre_prev[gi, bi, ki] = v
        rows = lambda t: t.permute(1, 0, 2).reshape(B, -1)                     # [G, B, n] -> [B, G n]: group g at columns g n
        if form == "shared":
            self.x_r, self.xg = Region(B, K, pitch=K + 8, off=4, fill=self.x[0]), 0
        elif form == "member":
            self.x_r = Region(G * B, K, pitch=K + 8, off=4, fill=self.x.reshape(G * B, K))
            self.xg = B * (K + 8)
        else:                                                                  # chained: the previous layer's activations, with slack
            self.x_r, self.xg = Region(B, G * K, pitch=G * K + 12, off=4, fill=rows(self.x)), K
        self.w_r = Region(E * N, K, pitch=K, fill=self.w.reshape(E * N, K))
        self.b_r = Region(E, N, pitch=N, fill=self.b)
        self.dpre_r = Region(B, G * N, pitch=G * N + 8, off=4, fill=rows(self.dpre))
        self.pp_r = Region(B, G * K, pitch=G * K + 12, off=4, fill=rows(self.pre_prev))
        self.rows = rows

    def inputs_intact(self):
        for r in (self.x_r, self.w_r, self.b_r, self.dpre_r, self.pp_r):
            r.get("an input's guard band")

    def fwd(self, pre=True, act=True):
        pre_r = Region(self.B, self.G * self.N, pitch=self.G * self.N + 12, off=4) if pre else None
        act_r = Region(self.B, self.G * self.N, pitch=self.G * self.N + 12, off=8) if act else None
        L = _L()
        L.check(L.lib().s2p_ensemble_linear_fwd(self.x_r.ptr, self.xg, self.x_r.pitch, self.w_r.ptr, self.b_r.ptr, _member(self.member), self.G,
                                                self.E, self.B, self.K, self.N, _p(pre_r), _p(act_r), self.G * self.N + 12, _st()),
                "s2p_ensemble_linear_fwd")
        return pre_r, act_r

    def bwd(self, dprev=True):
        dw_r, db_r = Region(self.E * self.N, self.K, pitch=self.K), Region(self.E, self.N, pitch=self.N)
        dprev_r = Region(self.B, self.G * self.K, pitch=self.G * self.K + 12, off=8) if dprev else None
        L = _L()
        L.check(L.lib().s2p_ensemble_linear_bwd(self.x_r.ptr, self.xg, self.x_r.pitch, self.dpre_r.ptr, self.dpre_r.pitch,
                                                self.w_r.ptr if dprev else None, _member(self.member), self.G, self.E, self.B, self.K, self.N,
                                                dw_r.ptr, db_r.ptr, self.pp_r.ptr if dprev else None, _p(dprev_r), self.G * self.K + 12, _st()),
                "s2p_ensemble_linear_bwd")
        return dw_r, db_r, dprev_r

    def ref_fwd(self, dt):
        pre = torch.einsum("gbk,gnk->gbn", self.x.to(dt), self.w[self.mem].to(dt)) + self.b[self.mem].to(dt)[:, None]
        return self.rows(pre), self.rows(O.swish(pre))

    def ref_bwd(self, dt):
        d, x, w = self.dpre.to(dt), self.x.to(dt), self.w[self.mem].to(dt)
        p = self.pre_prev.to(dt).requires_grad_(True)
        O.swish(p).backward(torch.einsum("gbn,gnk->gbk", d, w))               # dprev = (dpre . w) * swish'(pre_prev), by autograd
        return torch.einsum("gbn,gbk->gnk", d, x), d.sum(1), self.rows(p.grad)


LAYERS = [  # G, E, member, B, (K, N), x form
    (1, 1, None, 1, (4, 36), "shared"), (1, 1, None, 129, (100, 4), "member"), (1, 1, None, 33, (24, 32), "chained"),
    (3, 7, [6, 0, 3], 33, (24, 32), "chained"), (3, 7, [6, 0, 3], 129, (68, 96), "shared"), (3, 7, [6, 0, 3], 1, (36, 100), "member"),
    (3, 7, [6, 0, 3], 33, (4, 36), "member"), (3, 7, [6, 0, 3], 129, (100, 4), "chained"),
    (8, 8, None, 33, (68, 96), "member"), (8, 8, None, 129, (36, 100), "chained"), (8, 8, None, 1, (100, 4), "shared"),
    (8, 8, None, 129, (24, 32), "shared"),
]


@pytest.mark.parametrize("G,E,member,B,KN,form", LAYERS)
def test_grouped_swish_layer(hip_device, G, E, member, B, KN, form):
    """K = 68: a k tail of 4 past the 64-wide tile; K = 100: a second 32-wide k half with four columns live; B = 129: one row past
    the 128-row tile; member [6, 0, 3]: a table that is not increasing."""
    K, N = KN
    lay = Layer(G, E, member, B, K, N, form, seed=1000 * G + 10 * B + K)
    tag = "G %d B %d K %d N %d %s" % (G, B, K, N, form)
    # forward
    pre_r, act_r = lay.fwd()
    (p64, a64), (p32, a32) = lay.ref_fwd(F64), lay.ref_fwd(F32)
    _check("layer forward", pre_r.get("pre"), p64, p32, tag + " pre")
    _check("layer forward", act_r.get("act"), a64, a32, tag + " act")
    assert _same(lay.fwd(), (pre_r, act_r))                                    # two identical calls: equal bits
    assert torch.equal(lay.fwd(act=False)[0].bits("pre alone"), pre_r.bits())
    assert torch.equal(lay.fwd(pre=False)[1].bits("act alone"), act_r.bits())
    # backward
    dw_r, db_r, dprev_r = lay.bwd()
    (w64, b64, d64), (w32, b32, d32) = lay.ref_bwd(F64), lay.ref_bwd(F32)
    dw, db = dw_r.get("dw").view(E, N, K), db_r.get("db")
    _check("layer backward", dw[lay.mem], w64, w32, tag + " dw")
    _check("layer backward", db[lay.mem], b64, b32, tag + " db")
    _check("layer backward", dprev_r.get("dprev"), d64, d32, tag + " dprev")
    assert bool((dw[lay.mem][:, :, lay.k_real:] == 0).all())                   # the K padding's gradient is exactly zero
    others = [e for e in range(E) if e not in lay.mem]
    assert bool((dw[others] == SENT32).all()) and bool((db[others] == SENT32).all())      # slots not listed keep their bits
    assert _same(lay.bwd(), (dw_r, db_r, dprev_r))
    dw2, db2, none = lay.bwd(dprev=False)                                      # dprev == NULL with w == NULL (and pre_prev == NULL)
    assert none is None and torch.equal(dw2.bits("dw alone"), dw_r.bits()) and torch.equal(db2.bits("db alone"), db_r.bits())
    lay.inputs_intact()


def _flat(v):
    return torch.full((1 << 16,), v, device="cuda")


def _untouched(outs, what):
    torch.cuda.synchronize()
    assert all(bool((o == SENT32).all()) for o in outs), ("an output was written", what)


def _refused(lib, rc, outs, what):
    assert rc != 0 and lib.s2p_last_error(), what
    _untouched(outs, what)


def test_grouped_layer_refusals_and_no_ops(hip_device):
    """Every buffer is far larger than the largest geometry a case claims (E = 9 slots of 8 x 8): a call accepted by mistake stays
    inside it.  The out-of-range member is E, never a negative one."""
    L = _L()
    lib = L.lib()
    zin, pre, act, dw, db, dprev = _flat(0.0), _flat(SENT), _flat(SENT), _flat(SENT), _flat(SENT), _flat(SENT)
    z = zin.data_ptr()

    def fwd(**kw):
        a = dict(x=z, xg=0, xp=8, w=z, bias=z, member=None, G=2, E=7, B=8, K=8, N=8, pre=pre.data_ptr(), act=act.data_ptr(), yp=16)
        a.update(kw)
        a["member"] = _member(a["member"])
        return lib.s2p_ensemble_linear_fwd(*a.values(), _st())

    def bwd(**kw):
        a = dict(x=z, xg=0, xp=8, dpre=z, dp=16, w=z, member=None, G=2, E=7, B=8, K=8, N=8, dw=dw.data_ptr(), db=db.data_ptr(), pre_prev=z,
                 dprev=dprev.data_ptr(), pp=16)
        a.update(kw)
        a["member"] = _member(a["member"])
        return lib.s2p_ensemble_linear_bwd(*a.values(), _st())

    for bad in (dict(G=8, yp=64), dict(G=2, E=9), dict(member=[0, 7]), dict(K=6), dict(xp=4), dict(yp=12), dict(x=z + 4), dict(w=z + 8),
                dict(pre=None, act=None), dict(x=None), dict(bias=None), dict(B=-1), dict(xg=2)):
        _refused(lib, fwd(**bad), (pre, act), ("fwd", bad))
    for bad in (dict(G=8, dp=64, pp=64), dict(G=2, E=9), dict(member=[7, 0]), dict(K=6), dict(N=6), dict(xp=4), dict(dp=12), dict(pp=12),
                dict(dpre=z + 4), dict(w=None), dict(pre_prev=None), dict(dw=None), dict(db=None), dict(x=None), dict(N=-8)):
        _refused(lib, bwd(**bad), (dw, db, dprev), ("bwd", bad))
    # a size of 0 returns 0 with every pointer NULL
    for zero in (dict(G=0), dict(B=0), dict(N=0)):
        null = dict(x=None, w=None, bias=None, pre=None, act=None)
        null.update(zero)
        assert fwd(**null) == 0, zero
        null = dict(x=None, dpre=None, w=None, dw=None, db=None, pre_prev=None, dprev=None)
        null.update(zero)
        assert bwd(**null) == 0, zero
    assert bwd(x=None, dpre=None, w=None, dw=None, db=None, pre_prev=None, dprev=None, K=0) == 0
    _untouched((pre, act, dw, db, dprev), "by a no-op")
    assert fwd() == 0 and bwd() == 0                                           # the baseline itself is accepted
    torch.cuda.synchronize()
    assert float(pre[:16].abs().max()) == 0.0 and float(dw[:64].abs().max()) == 0.0


# ---- the two heads: common inputs ------------------------------------------------------------------------------------------------------
PLANTED = (21.5, -21.5, 30.0, -30.0, 60.0, -60.0)


def head_inputs(B, G, D, seed):
    """raw [G, B, 2 D] with log-stds planted on both sides of both soft-clamp softplus thresholds, bounds as
    ensemble_train_ref.make_params draws them -- but for the LAST output, whose lower bound is -26: max - min > 20 is the only way into
    the linear branch of the lower clamp's softplus.  The planted values stay off that output (exp(26) would swamp every sum)."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(G, B, 2 * D, generator=g)
    raw[..., D:] = raw[..., D:] * 1.5 - 1.0
    for i, v in enumerate(PLANTED):
        raw[i % G, (5 * i) % B, D + (3 * i) % (D - 1)] = v
    mx = torch.rand(D, generator=g) * 1.5 - 0.5
    mn = -torch.rand(D, generator=g) * 3 - 2
    mn[D - 1] = -26.0
    x = torch.randn(G, B, D + 1, generator=g)                                  # (obs, action): D - 1 columns are read
    t = torch.cat([x[..., :D - 1], torch.zeros(G, B, 1)], -1) + raw[..., :D] + 0.5 * torch.randn(G, B, D, generator=g)
    return raw, mn, mx, x, t


def mean_logstd(raw, mn, mx, x, D):
    mu = torch.cat([raw[..., :D - 1] + x[..., :D - 1], raw[..., D - 1:D]], -1)  # 'local' mode: the obs part is a delta
    return mu, O.soft_clamp(raw[..., D:], mn, mx)


def test_planted_log_stds_take_every_softplus_branch():
    raw, mn, mx, x, t = head_inputs(129, 5, 18, 0)
    up = (mx - raw[..., 18:]).double()
    lo = (mx - torch.nn.functional.softplus(up)) - mn
    assert bool((up > 20).any()) and bool((up < -20).any()) and bool((lo > 20).any()) and bool((lo < -20).any())


# ---- s2p_ensemble_nll ------------------------------------------------------------------------------------------------------------------
NLL_OUTS = ("sums", "loss", "draw", "dmin", "dmax", "mean", "std")


class Nll:
    def __init__(self, B, G, D, shared, seed):
        self.B, self.G, self.D, self.shared = B, G, D, shared
        self.raw, self.mn, self.mx, x, t = head_inputs(B, G, D, seed)
        if shared:
            x, t = x[:1].expand(G, B, D + 1).contiguous(), t[:1].expand(G, B, D).contiguous()
        self.x, self.t = x, t
        self.scale, self.reg = 1.0 / (G * B * D), 0.01 / D
        rows = lambda v: v.permute(1, 0, 2).reshape(B, -1)
        self.rows = rows
        self.raw_r = Region(B, G * 2 * D, pitch=G * 2 * D + 5, off=3, fill=rows(self.raw))
        n = 1 if shared else G
        self.x_r = Region(n * B, D + 1, pitch=D + 4, off=1, fill=x[:n].reshape(n * B, D + 1))
        self.t_r = Region(n * B, D, pitch=D + 3, off=2, fill=t[:n].reshape(n * B, D))
        self.xg, self.tg = (0, 0) if shared else (B * self.x_r.pitch, B * self.t_r.pitch)
        self.mn_r, self.mx_r = Region(1, D, off=1, fill=self.mn[None]), Region(1, D, off=3, fill=self.mx[None])

    def run(self, want=NLL_OUTS, target=True):
        B, G, D = self.B, self.G, self.D
        shapes = dict(sums=(1, 2 * G, None, 1), loss=(1, 1, None, 1), draw=(B, G * 2 * D, G * 2 * D + 7, 2), dmin=(1, D, None, 1),
                      dmax=(1, D, None, 3), mean=(G * B, D, D, 0), std=(G * B, D, D, 0))
        o = {k: (Region(m, w, pitch=p, off=off) if k in want else None) for k, (m, w, p, off) in shapes.items()}
        L = _L()
        L.check(L.lib().s2p_ensemble_nll(self.raw_r.ptr, self.raw_r.pitch, self.x_r.ptr, self.xg, self.x_r.pitch,
                                         self.t_r.ptr if target else None, self.tg, self.t_r.pitch, B, G, D, self.mn_r.ptr, self.mx_r.ptr,
                                         self.scale, self.reg, _p(o["sums"]), _p(o["loss"]), _p(o["draw"]), G * 2 * D + 7, _p(o["dmin"]),
                                         _p(o["dmax"]), _p(o["mean"]), _p(o["std"]), _st()), "s2p_ensemble_nll")
        return o

    def ref(self, dt):
        raw, mn, mx = [v.to(dt).clone().requires_grad_(True) for v in (self.raw, self.mn, self.mx)]
        mu, ls = mean_logstd(raw, mn, mx, self.x.to(dt), self.D)
        t = self.t.to(dt)
        nll = 0.5 * ((t - mu) / torch.exp(ls)) ** 2 + ls + 0.5 * math.log(2 * math.pi)
        loss = self.scale * nll.sum() + self.reg * (mx - mn).sum()
        loss.backward()
        return dict(nll=nll.sum((1, 2)).detach(), se=((mu - t) ** 2).sum((1, 2)).detach(), loss=loss.detach().reshape(1), draw=self.rows(raw.grad),
                    dmin=mn.grad, dmax=mx.grad, mean=mu.detach().reshape(-1, self.D), std=torch.exp(ls).detach().reshape(-1, self.D))


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("B,G,D", [(1, 1, 2), (3, 8, 33), (129, 5, 18), (300, 7, 2), (37, 3, 33)])
def test_nll_head(hip_device, B, G, D, shared):
    c = Nll(B, G, D, shared, seed=100 * B + D)
    tag = "B %d G %d D %d %s" % (B, G, D, "shared" if shared else "per member")
    o = c.run()
    r64, r32 = c.ref(F64), c.ref(F32)
    got = {k: v.get(k) for k, v in o.items()}
    got.update(nll=got["sums"][0, :G], se=got["sums"][0, G:], loss=got["loss"][0], dmin=got["dmin"][0], dmax=got["dmax"][0])
    for k in ("nll", "se", "loss", "draw", "dmin", "dmax", "mean", "std"):
        _check("nll " + k, got[k], r64[k], r32[k], tag)
    assert _same(c.run().values(), o.values())                                 # two identical calls: equal bits
    for alone in (("sums",), ("loss",), ("draw",), ("dmin", "dmax"), ("mean",), ("std",)):
        a = c.run(want=alone)
        assert all(torch.equal(a[k].bits(k + " alone"), o[k].bits()) for k in alone), alone
    f = c.run(want=("mean", "std"), target=False)                              # the forward alone: no target
    assert torch.equal(f["mean"].bits(), o["mean"].bits()) and torch.equal(f["std"].bits(), o["std"].bits())
    for r in (c.raw_r, c.x_r, c.t_r, c.mn_r, c.mx_r):
        r.get("an input's guard band")


def test_nll_head_refusals_and_no_op(hip_device):
    L = _L()
    lib = L.lib()
    zin = _flat(0.0)
    outs = {k: _flat(SENT) for k in NLL_OUTS}
    z = zin.data_ptr()

    def nll(**kw):
        a = dict(raw=z, rp=36, xin=z, xg=0, xp=8, target=z, tg=0, tp=6, B=4, G=3, D=6, mn=z, mx=z, scale=1.0, reg=0.0,
                 sums=outs["sums"].data_ptr(), loss=outs["loss"].data_ptr(), draw=outs["draw"].data_ptr(), dwp=36,
                 dmin=outs["dmin"].data_ptr(), dmax=outs["dmax"].data_ptr(), mean=outs["mean"].data_ptr(), std=outs["std"].data_ptr())
        a.update(kw)
        return lib.s2p_ensemble_nll(*a.values(), _st())

    no_out = dict(sums=None, loss=None, draw=None, dmin=None, dmax=None, mean=None, std=None)
    for bad in (dict(D=1, rp=64), dict(D=34, rp=204, xp=36, tp=36, dwp=204), dict(G=9, rp=108, dwp=108), dict(dmin=None), dict(dmax=None),
                dict(target=None), dict(target=None, sums=None, loss=None, draw=None, dmin=None, dmax=None, mean=None, std=None), no_out,
                dict(rp=35), dict(xp=4), dict(tp=5), dict(dwp=35), dict(raw=None), dict(xin=None), dict(mn=None), dict(B=-1)):
        _refused(lib, nll(**bad), outs.values(), ("nll", bad))
    null = dict(raw=None, xin=None, target=None, mn=None, mx=None, **no_out)
    for zero in (dict(B=0), dict(G=0), dict(D=0)):
        assert nll(**dict(null, **zero)) == 0, zero
    _untouched(outs.values(), "by a no-op")
    assert nll() == 0                                                          # the baseline itself is accepted
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs["loss"][:1]).all())


# ---- s2p_ensemble_head -----------------------------------------------------------------------------------------------------------------
HEAD_SETS = (("mean", "std"), ("next_obs", "reward"), ("dis", "ale"))


class Head:
    def __init__(self, B, E, D, seed, slots=None):
        self.B, self.E, self.D = B, E, D
        self.raw, self.mn, self.mx, x, _ = head_inputs(B, E, D, seed)
        self.x = x[0]
        g = torch.Generator().manual_seed(seed + 1)
        self.om, self.os = torch.randn(D - 1, generator=g), torch.rand(D - 1, generator=g) + 0.5
        self.rm, self.rs = 0.3, 1.7
        self.pick = (E - 1 - torch.arange(B) % E).to(torch.int32)              # every member, E - 1 and 0 included
        cols = (slots or E) * 2 * D
        self.raw_r = Region(B, cols, pitch=cols + 5, off=3, fill=torch.zeros(B, cols))
        self.raw_r.v[:, :E * 2 * D] = self.raw.permute(1, 0, 2).reshape(B, -1).cuda()
        self.x_r = Region(B, D + 1, pitch=D + 4, off=1, fill=self.x)
        self.mn_r, self.mx_r = Region(1, D, off=1, fill=self.mn[None]), Region(1, D, off=3, fill=self.mx[None])
        self.om_r, self.os_r = Region(1, D - 1, off=1, fill=self.om[None]), Region(1, D - 1, off=2, fill=self.os[None])

    def run(self, want=sum(HEAD_SETS, ()), pick=None):
        B, E, D = self.B, self.E, self.D
        shapes = dict(mean=(E * B, D), std=(E * B, D), next_obs=(B, D - 1), reward=(1, B), dis=(1, B), ale=(1, B))
        o = {k: (Region(m, w, pitch=w) if k in want else None) for k, (m, w) in shapes.items()}       # dense by contract: guard bands at both ends
        pk = (self.pick if pick is None else pick).cuda() if "next_obs" in want else None
        L = _L()
        L.check(L.lib().s2p_ensemble_head(self.raw_r.ptr, self.raw_r.pitch, self.x_r.ptr, self.x_r.pitch, B, E, D, self.mn_r.ptr, self.mx_r.ptr,
                                          _p(o["mean"]), _p(o["std"]), pk.data_ptr() if pk is not None else None, self.om_r.ptr, self.os_r.ptr,
                                          self.rm, self.rs, _p(o["next_obs"]), _p(o["reward"]), _p(o["dis"]), _p(o["ale"]), _st()),
                "s2p_ensemble_head")
        return o

    def ref(self, dt):
        mu, ls = mean_logstd(self.raw.to(dt), self.mn.to(dt), self.mx.to(dt), self.x.to(dt)[None], self.D)
        std = torch.exp(ls)
        nobs, rew, dis, ale = O.rollout_postprocess(mu, std, self.pick.long(), self.om.to(dt), self.os.to(dt), self.rm, self.rs)
        return dict(mean=mu.reshape(-1, self.D), std=std.reshape(-1, self.D), next_obs=nobs, reward=rew[None], dis=dis[:, 0][None], ale=ale[:, 0][None])


@pytest.mark.parametrize("B,E,D", [(1, 1, 2), (127, 7, 18), (129, 8, 33), (300, 3, 2)])
def test_rollout_head(hip_device, B, E, D):
    """D = 33 is the case that found the kernel indexing one register past its 32-entry running average."""
    c = Head(B, E, D, seed=10 * B + E)
    assert sorted(set(c.pick.tolist())) == list(range(E))
    tag = "B %d E %d D %d" % (B, E, D)
    o = c.run()
    r64, r32 = c.ref(F64), c.ref(F32)
    for k in o:
        _check("head " + k, o[k].get(k), r64[k], r32[k], tag)
    if E == 1:
        assert float(o["dis"].get().abs().max()) == 0.0                        # one member: it is its own average, exactly
    assert _same(c.run().values(), o.values())                                 # two identical calls: equal bits
    for alone in HEAD_SETS:
        a = c.run(want=alone)
        assert all(torch.equal(a[k].bits(k + " alone"), o[k].bits()) for k in alone), alone
    for r in (c.raw_r, c.x_r, c.mn_r, c.mx_r, c.om_r, c.os_r):
        r.get("an input's guard band")


def test_rollout_head_poisons_the_rows_of_an_out_of_range_pick(hip_device):
    """pick[b] == E (raw holds E + 1 slots, so even a kernel that followed the index would stay inside it): that row of next_obs and
    its reward are NaN, every other row and the two uncertainties keep the bits of the call with valid picks."""
    B, E, D = 40, 3, 6
    c = Head(B, E, D, seed=5, slots=E + 1)
    good = c.run()
    bad_rows = [0, 17, 39]
    pick = c.pick.clone()
    pick[bad_rows] = E
    o = c.run(pick=pick)
    nobs, rew = o["next_obs"].bits(), o["reward"].bits()[0]
    assert bool(torch.isnan(nobs[bad_rows]).all()) and bool(torch.isnan(rew[bad_rows]).all())
    keep = [b for b in range(B) if b not in bad_rows]
    assert torch.equal(nobs[keep], good["next_obs"].bits()[keep]) and torch.equal(rew[keep], good["reward"].bits()[0][keep])
    assert all(torch.equal(o[k].bits(), good[k].bits()) for k in ("mean", "std", "dis", "ale"))


def test_rollout_head_refusals_and_no_op(hip_device):
    L = _L()
    lib = L.lib()
    zin, ones = _flat(0.0), _flat(1.0)
    outs = {k: _flat(SENT) for k in sum(HEAD_SETS, ())}
    pick = torch.zeros(1 << 12, dtype=torch.int32, device="cuda")
    z = zin.data_ptr()

    def head(**kw):
        a = dict(raw=z, rp=36, xin=z, xp=8, B=4, E=3, D=6, mn=z, mx=z, mean=outs["mean"].data_ptr(), std=outs["std"].data_ptr(),
                 pick=pick.data_ptr(), om=z, os=ones.data_ptr(), rm=0.0, rs=1.0, next_obs=outs["next_obs"].data_ptr(),
                 reward=outs["reward"].data_ptr(), dis=outs["dis"].data_ptr(), ale=outs["ale"].data_ptr())
        a.update(kw)
        return lib.s2p_ensemble_head(*a.values(), _st())

    for bad in (dict(B=-1), dict(rp=35), dict(xp=4), dict(D=1), dict(D=34, rp=204, xp=36), dict(E=0), dict(raw=None), dict(xin=None), dict(mn=None),
                dict(mx=None), dict(next_obs=None), dict(reward=None), dict(om=None)):
        _refused(lib, head(**bad), outs.values(), ("head", bad))
    null = {k: None for k in ("raw", "xin", "mn", "mx", "mean", "std", "pick", "om", "os", "next_obs", "reward", "dis", "ale")}
    assert head(B=0, **null) == 0                                              # B == 0 returns 0 with every pointer NULL
    _untouched(outs.values(), "by a no-op")
    assert head() == 0                                                         # the baseline itself is accepted
    torch.cuda.synchronize()
    assert float(outs["reward"][:4].abs().max()) == 0.0 and float(outs["dis"][:4].abs().max()) == 0.0


# ---- the callers of the head -----------------------------------------------------------------------------------------------------------
def _small_model():
    from s2p_amd.dynamics import EnsembleTransition
    return EnsembleTransition(5, 2, 32, 3, ensemble_size=7).init_parameters(seed=1)


def test_rollout_step_on_an_empty_batch(hip_device):
    m = _small_model()
    nobs, rew, dis, ale = m.rollout_step(torch.zeros(0, 7), np.zeros(0, np.int32), np.zeros(5, np.float32), np.ones(5, np.float32), 0.0, 1.0)
    assert nobs.shape == (0, 5) and rew.shape == (0,) and dis.shape == (0, 1) and ale.shape == (0, 1)
    assert all(t.is_cuda and t.dtype == torch.float32 for t in (nobs, rew, dis, ale))


def test_rollout_sweep_shows_a_bad_device_index_as_a_nan_row(hip_device):
    """rollout_sweep range-checks host indices only (no device sync): a device index tensor with one bad entry used to leave that row
    of the generated dataset uninitialised."""
    m = _small_model()
    g = torch.Generator().manual_seed(2)
    obs, act = torch.randn(9, 5, generator=g), torch.rand(9, 2, generator=g) * 2 - 1
    norm = (np.zeros(5, np.float32), np.ones(5, np.float32), np.zeros(5, np.float32), np.ones(5, np.float32), 0.0, 1.0)
    idx = torch.arange(9) % 7
    good = m.rollout_sweep(obs, act, idx, *norm)
    idx_dev = idx.clone()
    idx_dev[4] = 7
    bad = m.rollout_sweep(obs, act, idx_dev.to(hip_device), *norm, chunk=4)
    keep = [0, 1, 2, 3, 5, 6, 7, 8]
    assert bool(torch.isnan(bad[0][4]).all()) and bool(torch.isnan(bad[1][4]))
    assert all(torch.equal(a[keep], b[keep]) for a, b in zip(good, bad)) and torch.equal(good[2], bad[2]) and torch.equal(good[3], bad[3])
    assert bool(torch.isfinite(good[0]).all()) and bool(torch.isfinite(good[1]).all())


def test_zz_report_worst_ratios(hip_device):
    print("\nworst deviation / max(ref32_err, 1e-6) per group:", {k: round(v, 3) for k, v in WORST.items()})
    assert WORST and max(WORST.values()) <= K_TOL
