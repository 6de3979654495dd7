"""Kernel-level parity of csrc/cql.hip and the CQL half of csrc/mlp.hip through the C ABI against float64 torch on the CPU: the input-gradient half of the grouped
backward (bitwise against s2p_mlp_linear_bwd), the row-split backward (S = 1 bitwise, S > 1 against fp64), the reparameterised TanhNormal sample and its backward, the fused SAC policy head
with the entropy-temperature step, the fused CQL critic head, the refused arguments, and bitwise repeatability of every entry point.

Tolerance: the project's rule (tests/test_ensemble_train_gpu.py) -- per quantity K_TOL x max(ref32_err, 1e-6), K_TOL = 4, ref32_err
being the deviation of the SAME formula run in fp32 torch on the CPU from its fp64 run (relative to the fp64 maximum).
Worst observed ratios: DESIGN.md section 6b.5 (printed by test_zz_report_worst_ratios)."""
import math

import pytest
import torch

import iql_ref as R
from test_iql_kernels_gpu import Group, _L, _ptr, _st, run_bwd

pytestmark = pytest.mark.gpu
K_TOL, FLOOR = 4.0, 1e-6
WORST = {}


def _check(group, got, f64, f32, what=""):
    got, f64, f32 = (torch.as_tensor(v).detach().cpu().double().reshape(-1) for v in (got, f64, f32))
    err, ref = R.rel_max(got, f64), max(R.rel_max(f32, f64), FLOOR)
    WORST[group] = max(WORST.get(group, 0.0), err / ref)
    print("%-16s %-40s err %.3e  ref32_err %.3e  ratio %.3f" % (group, what, err, ref, err / ref))
    assert err <= K_TOL * ref, (group, what, err, K_TOL * ref)


def _call(name, *args):
    L = _L()
    L.check(getattr(L.lib(), name)(*args), name)
    torch.cuda.synchronize()


def _rc(name, *args):
    return getattr(_L().lib(), name)(*args)


# ---- s2p_mlp_linear_dgrad -----------------------------------------------------------------------------------------------------------
def run_dgrad(groups, N, relu, dev, canaries=True):
    L = _L()
    outs = [(torch.full((N, g.kp), 7.0, device=dev) if canaries else None, torch.full((N,), 7.0, device=dev) if canaries else None,
             torch.full((g.rows, g.pp), 7.0, device=dev)) for g in groups]
    arr = (L.MlpBwdGroup * len(groups))(*[
        L.MlpBwdGroup(None, _ptr(g.dpd), _ptr(g.wd), _ptr(dw), _ptr(db), _ptr(g.ppd) if relu else None, _ptr(dp), g.xp, g.dp, g.pp, g.rows,
                      g.kp) for g, (dw, db, dp) in zip(groups, outs)])
    _call("s2p_mlp_linear_dgrad", arr, len(groups), N, L.ACT_RELU if relu else L.ACT_NONE, _st())
    return outs


@pytest.mark.parametrize("N", [36, 1])
@pytest.mark.parametrize("relu", [True, False])
def test_dgrad_is_the_dprev_of_the_full_backward_bitwise(hip_device, N, relu):
    """K = 44 and K = 28 in one launch, 130 and 37 rows (one row past the 128-row tile, a row tail), N = 36 on the MFMA tiles and
    N = 1 on the dot-product form; relu = False is the first layer (act_prev NONE, pre_prev NULL)."""
    g = torch.Generator().manual_seed(N * 2 + relu)
    groups = [Group(130, 44, N, hip_device, g, zero_pre=N > 2), Group(37, 28, N, hip_device, g)]
    full = run_bwd(groups, N, relu, hip_device)
    for canaries in (True, False):
        got = run_dgrad(groups, N, relu, hip_device, canaries)
        for grp, (_, _, want), (dw, db, dprev) in zip(groups, full, got):
            assert torch.equal(dprev, want)                                          # bitwise, the untouched pitch columns included
            assert float(dprev[:, :grp.K].abs().max()) > 0
            if canaries:
                assert bool((dw == 7.0).all()) and bool((db == 7.0).all())           # the weight-gradient buffers are not touched
    d64, d32 = groups[0].ref_bwd(torch.float64, relu)[2], groups[0].ref_bwd(torch.float32, relu)[2]
    _check("dgrad", got[0][2][:, :44], d64, d32, "N %d relu %d" % (N, relu))
    again = run_dgrad(groups, N, relu, hip_device)
    assert all(torch.equal(a[2], b[2]) for a, b in zip(got, again))


def test_dgrad_skips_an_empty_group_and_refuses_bad_arguments(hip_device):
    L, g = _L(), torch.Generator().manual_seed(3)
    grp = Group(37, 44, 36, hip_device, g)
    dp = torch.full((37, grp.pp), 7.0, device=hip_device)

    def group(**kw):
        f = dict(x=None, dpre=_ptr(grp.dpd), w=_ptr(grp.wd), dw=None, db=None, pre_prev=_ptr(grp.ppd), dprev=_ptr(dp), x_pitch=0,
                 dpre_pitch=grp.dp, prev_pitch=grp.pp, rows=37, K=grp.kp)
        f.update(kw)
        return L.MlpBwdGroup(*[f[k] for k in ("x", "dpre", "w", "dw", "db", "pre_prev", "dprev", "x_pitch", "dpre_pitch", "prev_pitch", "rows", "K")])

    def rc(gs, N=36, act=L.ACT_RELU, G=None):
        return _rc("s2p_mlp_linear_dgrad", (L.MlpBwdGroup * len(gs))(*gs), len(gs) if G is None else G, N, act, _st())

    assert rc([group(rows=0, dpre=None, w=None, dprev=None), group()]) == 0           # an empty group looks at no pointer
    assert rc([group()], G=0) == 0 and rc([group()], N=0) == 0 and _rc("s2p_mlp_linear_dgrad", None, 0, 36, L.ACT_RELU, _st()) == 0
    for bad in (group(rows=-1), group(K=-4), group(dpre=None), group(w=None), group(dprev=None), group(pre_prev=None),
                group(dpre_pitch=32), group(prev_pitch=40), group(dpre=_ptr(grp.dpd) + 4), group(dpre_pitch=grp.dp + 1)):
        assert rc([bad]) != 0
    assert rc([group()], G=-1) != 0 and rc([group()], N=-1) != 0 and rc([group()], act=3) != 0 and rc([group()] * 9) != 0
    assert _rc("s2p_mlp_linear_dgrad", None, 1, 36, L.ACT_RELU, _st()) != 0 and rc([group()], N=38) != 0
    assert rc([group(pre_prev=None)], act=L.ACT_NONE) == 0                            # the first layer needs no pre_prev
    torch.cuda.synchronize()


# ---- s2p_mlp_linear_bwd_split ----------------------------------------------------------------------------------------------------------
def run_split(groups, N, relu, S, dev, short=0):
    L = _L()
    outs = [(torch.full((N, g.kp), 7.0, device=dev), torch.full((N,), 7.0, device=dev), torch.full((g.rows, g.pp), 7.0, device=dev)) for g in groups]
    arr = (L.MlpBwdGroup * len(groups))(*[
        L.MlpBwdGroup(_ptr(g.xd), _ptr(g.dpd), _ptr(g.wd), _ptr(dw), _ptr(db), _ptr(g.ppd) if relu else None, _ptr(dp), g.xp, g.dp, g.pp,
                      g.rows, g.kp) for g, (dw, db, dp) in zip(groups, outs)])
    need = L.lib().s2p_mlp_linear_bwd_split_workspace(arr, len(groups), N, S)
    assert need == 4 * S * sum((N * g.kp + N) for g in groups if g.rows)
    ws = torch.full((need // 4 + 8,), float("nan"), device=dev)
    rc = L.lib().s2p_mlp_linear_bwd_split(arr, len(groups), N, L.ACT_RELU if relu else L.ACT_NONE, S, _ptr(ws), need - short, _st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[need // 4:]).all())                                    # nothing written past the stated size
    return rc, outs


@pytest.mark.parametrize("rows,S", [(481, 3), (481, 5), (20, 4), (481, 1)])
@pytest.mark.parametrize("relu", [True, False])
def test_split_backward(hip_device, rows, S, relu):
    """Two groups of unequal rows and widths (K = 44 and K = 28, N = 36) and a group with 0 rows; 481 rows in 3 and 5 chunks (176 and
    112 rows: the last chunk shorter), 20 rows in 4 chunks of 16 (two chunks receive no row); S = 1 is s2p_mlp_linear_bwd bitwise."""
    g, N = torch.Generator().manual_seed(rows + S), 36
    groups = [Group(rows, 44, N, hip_device, g, zero_pre=True), Group(0, 44, N, hip_device, g), Group(max(rows // 3, 1), 28, N, hip_device, g)]
    full = run_bwd(groups, N, relu, hip_device)
    rc, got = run_split(groups, N, relu, S, hip_device)
    assert rc == 0
    for grp, (dw0, db0, dp0), (dw, db, dp) in zip(groups, full, got):
        assert torch.equal(dp, dp0)                                                   # the input-gradient tiles are unchanged
        if S == 1 or grp.rows == 0:
            assert torch.equal(dw, dw0) and torch.equal(db, db0)
            continue
        (w64, b64, _), (w32, b32, _) = grp.ref_bwd(torch.float64, relu), grp.ref_bwd(torch.float32, relu)
        _check("split backward", dw[:, :grp.K], w64, w32, "dw rows %d S %d K %d" % (grp.rows, S, grp.K))
        _check("split backward", db, b64, b32, "db")
        assert bool((dw[:, grp.K:] == 0).all())
    rc2, again = run_split(groups, N, relu, S, hip_device)
    assert rc2 == 0 and all(torch.equal(a, b) for x, y in zip(got, again) for a, b in zip(x, y))
    rc3, untouched = run_split(groups, N, relu, S, hip_device, short=1)               # a workspace one byte short is refused
    assert rc3 != 0 and all(bool((t == 7.0).all()) for x in untouched for t in x)


def test_split_backward_refusals(hip_device):
    L, g = _L(), torch.Generator().manual_seed(9)
    grp = Group(37, 44, 36, hip_device, g)
    dw, db, ws = torch.zeros(36, grp.kp, device=hip_device), torch.zeros(36, device=hip_device), torch.zeros(4 * (36 * grp.kp + 36), device=hip_device)

    def rc(N=36, S=2, G=1, act=L.ACT_RELU, ws=ws, **kw):
        f = dict(x=_ptr(grp.xd), dpre=_ptr(grp.dpd), w=_ptr(grp.wd), dw=_ptr(dw), db=_ptr(db), pre_prev=None, dprev=None, x_pitch=grp.xp,
                 dpre_pitch=grp.dp, prev_pitch=0, rows=37, K=grp.kp)
        f.update(kw)
        arr = (L.MlpBwdGroup * 1)(L.MlpBwdGroup(*[f[k] for k in ("x", "dpre", "w", "dw", "db", "pre_prev", "dprev", "x_pitch", "dpre_pitch", "prev_pitch", "rows", "K")]))
        return L.lib().s2p_mlp_linear_bwd_split(arr, G, N, act, S, _ptr(ws), ws.numel() * 4 if ws is not None else 0, _st())

    assert rc() == 0 and rc(G=0) == 0 and rc(N=0) == 0 and rc(rows=0, x=None, dpre=None, dw=None, db=None, ws=None) == 0
    for bad in (dict(S=0), dict(S=65), dict(N=1), dict(N=38), dict(G=-1), dict(N=-1), dict(act=3), dict(ws=None), dict(rows=-1), dict(x=None),
                dict(dpre=None), dict(dw=None), dict(db=None), dict(x_pitch=40), dict(dpre_pitch=32), dict(dpre=_ptr(grp.dpd) + 4),
                dict(dprev=_ptr(dw), prev_pitch=grp.kp), dict(S=8)):
        assert rc(**bad) != 0, bad                                                    # (the last two: dprev without pre_prev under relu; S = 8 needs twice this workspace)
    assert L.lib().s2p_mlp_linear_bwd_split_workspace(None, 1, 36, 2) == 0
    one = (L.MlpBwdGroup * 1)(L.MlpBwdGroup(None, None, None, None, None, None, None, 0, 0, 0, 37, grp.kp))
    query = L.lib().s2p_mlp_linear_bwd_split_workspace
    assert query(one, 1, 36, 2) == 4 * 2 * (36 * grp.kp + 36)                        # sizes only: no pointer is looked at
    assert all(query(one, G, N, S) == 0 for G, N, S in ((0, 36, 2), (9, 36, 2), (1, 1, 2), (1, 16, 2), (1, 38, 2), (1, 36, 0), (1, 36, 65)))
    torch.cuda.synchronize()


# ---- s2p_tanh_gauss_rsample and its backward ---------------------------------------------------------------------------------------------
def sample_inputs(M, A, rep, seed):
    """raw log sigma below -20, inside, above 2 and exactly at both ends; pre-tanh values up to about +-15."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.cat([torch.randn(M, A, generator=g), torch.randn(M, A, generator=g) * 1.5 - 1.0], 1)
    eps = torch.randn(M * rep, A, generator=g)
    ls = raw[:, A:]
    ls[0], ls[1 % M], ls[2 % M], ls[3 % M] = -25.0, 3.5, -20.0, 2.0
    raw[4 % M, 0], raw[5 % M, A - 1] = 14.5, -14.0
    raw[4 % M, A], raw[5 % M, 2 * A - 1] = -21.0, -6.0                              # (a tiny sigma: u stays near the mean)
    return raw, eps


def sample_ref(raw, eps, rep, dtype):
    raw, eps = raw.to(dtype), eps.to(dtype)
    A = eps.shape[1]
    mean, ls = raw[:, :A].repeat_interleave(rep, 0), torch.clamp(raw[:, A:], -20.0, 2.0).repeat_interleave(rep, 0)
    u = mean + torch.exp(ls) * eps
    log2 = float(torch.tensor(math.log(2.0), dtype=torch.float32))
    logp = (-0.5 * eps ** 2 - ls - 0.5 * math.log(2 * math.pi)).sum(1) - 2.0 * (log2 - u - R.softplus(-2.0 * u)).sum(1)
    return torch.tanh(u), logp, u


@pytest.mark.parametrize("A", [1, 3, 8])
@pytest.mark.parametrize("rep", [1, 4])
def test_rsample_forward(hip_device, A, rep):
    """M * rep = 300 rows (more than one 256-thread block); the action goes to a column offset of a wider buffer, in one of three
    column blocks of a [M][3 rep] row group, and nothing else of that buffer changes."""
    dev, M = hip_device, 300 // rep
    raw, eps = sample_inputs(M, A, rep, 10 * A + rep)
    rawd = torch.full((M, 2 * A + 3), 9.0, device=dev); rawd[:, :2 * A] = raw.to(dev)
    epsd = torch.full((M * rep, A + 1), 9.0, device=dev); epsd[:, :A] = eps.to(dev)
    pitch, col, group, blk = 20, 5, 3 * rep, 1
    buf = torch.full((M * group, pitch), 7.0, device=dev)
    logp = torch.full((M, 2 * rep), 7.0, device=dev)
    u = torch.full((M * rep, A + 2), 7.0, device=dev)
    args = (_ptr(rawd), 2 * A + 3, _ptr(epsd), A + 1, M, A, rep, buf[blk * rep:, col:].data_ptr(), pitch, group,
            logp[:, rep:].data_ptr(), 2 * rep, _ptr(u), A + 2, _st())
    _call("s2p_tanh_gauss_rsample", *args)
    (a64, l64, u64), (a32, l32, u32) = sample_ref(raw, eps, rep, torch.float64), sample_ref(raw, eps, rep, torch.float32)
    assert float(u64.abs().max()) > 13
    view = buf.view(M, group, pitch)
    got_a = view[:, blk * rep:(blk + 1) * rep, col:col + A].reshape(M * rep, A)
    _check("rsample", got_a, a64, a32, "action A %d rep %d" % (A, rep))
    _check("rsample", logp[:, rep:].reshape(-1), l64, l32, "logp")
    _check("rsample", u[:, :A], u64, u32, "u")
    keep = torch.ones_like(view, dtype=torch.bool)
    keep[:, blk * rep:(blk + 1) * rep, col:col + A] = False
    assert bool((view[keep] == 7.0).all()) and bool((logp[:, :rep] == 7.0).all()) and bool((u[:, A:] == 7.0).all())
    first = (buf.clone(), logp.clone(), u.clone())
    _call("s2p_tanh_gauss_rsample", *args)
    assert all(torch.equal(a, b) for a, b in zip(first, (buf, logp, u)))
    only = torch.full((M * rep,), 7.0, device=dev)                                    # logp alone, compact
    _call("s2p_tanh_gauss_rsample", _ptr(rawd), 2 * A + 3, _ptr(epsd), A + 1, M, A, rep, None, 0, 0, _ptr(only), rep, None, 0, _st())
    assert torch.equal(only, logp[:, rep:].reshape(-1))


@pytest.mark.parametrize("A", [1, 3, 8])
def test_rsample_backward(hip_device, A):
    dev, M = hip_device, 300
    raw, eps = sample_inputs(M, A, 1, 77 + A)
    g = torch.Generator().manual_seed(A)
    dlogp, da, da2 = torch.randn(M, generator=g), torch.randn(M, A, generator=g), torch.randn(M, A, generator=g)

    def ref(dtype, with_action):
        r = raw.to(dtype).requires_grad_(True)
        act, logp, _ = sample_ref(r, eps, 1, dtype)
        loss = (logp * dlogp.to(dtype)).sum()
        if with_action:
            loss = loss + (act * (da + da2).to(dtype)).sum()
        return torch.autograd.grad(loss, r)[0]

    rawd, epsd, dld = raw.to(dev), eps.to(dev), dlogp.to(dev)
    dad = torch.zeros(2, M, A + 5, device=dev); dad[0, :, 2:2 + A] = da.to(dev); dad[1, :, 2:2 + A] = da2.to(dev)
    for with_action in (True, False):
        draw = torch.full((M, 2 * A + 1), 7.0, device=dev)
        args = (_ptr(rawd), 2 * A, _ptr(epsd), A, _ptr(dld), dad[0, :, 2:].data_ptr() if with_action else None,
                dad[1, :, 2:].data_ptr() if with_action else None, A + 5, M, A, _ptr(draw), 2 * A + 1)
        _call("s2p_tanh_gauss_rsample_bwd", *args, 0, _st())
        d64, d32 = ref(torch.float64, with_action), ref(torch.float32, with_action)
        _check("rsample bwd", draw[:, :2 * A], d64, d32, "A %d daction %d overwrite" % (A, with_action))
        outside = (raw[:, A:] < -20) | (raw[:, A:] > 2)
        assert outside.any() and bool((draw[:, A:2 * A].cpu()[outside] == 0).all()) and bool((draw[:, 2 * A] == 7.0).all())
        at_end = (raw[:, A:] == -20) | (raw[:, A:] == 2)
        assert at_end.any() and bool((draw[:, A:2 * A].cpu()[at_end] != 0).all())       # the clamp's ends pass the gradient
        first = draw.clone()
        _call("s2p_tanh_gauss_rsample_bwd", *args, 0, _st())
        assert torch.equal(first, draw)
        base = torch.randn(M, 2 * A + 1, generator=g)
        acc = base.to(dev)
        _call("s2p_tanh_gauss_rsample_bwd", _ptr(rawd), 2 * A, _ptr(epsd), A, _ptr(dld), args[5], args[6], A + 5, M, A, _ptr(acc), 2 * A + 1, 1, _st())
        _check("rsample bwd", acc[:, :2 * A], base[:, :2 * A].double() + d64, base[:, :2 * A] + d32, "add")
        assert torch.equal(acc[:, 2 * A].cpu(), base[:, 2 * A])


def test_rsample_refusals(hip_device):
    dev, M, A = hip_device, 8, 3
    raw, eps, out, lp = (torch.zeros(s, device=dev) for s in ((M, 2 * A), (M * 2, A), (M * 2, A), (M * 2,)))

    def fwd(raw=raw, rp=2 * A, eps=eps, ep=A, M=M, A=A, rep=2, action=out, ap=A, ag=2, logp=lp, lg=2, u=None, up=0):
        return _rc("s2p_tanh_gauss_rsample", _ptr(raw), rp, _ptr(eps), ep, M, A, rep, _ptr(action), ap, ag, _ptr(logp), lg, _ptr(u), up, _st())

    assert fwd() == 0
    assert fwd(M=0, raw=None, eps=None, action=None, logp=None) == 0 and fwd(A=0, raw=None, eps=None) == 0 and fwd(rep=0, raw=None) == 0
    for bad in (dict(M=-1), dict(A=-1), dict(rep=-1), dict(raw=None), dict(eps=None), dict(action=None, logp=None), dict(rp=2 * A - 1),
                dict(ep=A - 1), dict(ap=A - 1), dict(ag=1), dict(lg=1), dict(u=out, up=A - 1)):
        assert fwd(**bad) != 0, bad
    draw, dl = torch.zeros(M, 2 * A, device=dev), torch.zeros(M, device=dev)

    def bwd(raw=raw, rp=2 * A, eps=eps, ep=A, dlogp=dl, da=None, da2=None, dap=A, M=M, A=A, draw=draw, dwp=2 * A):
        return _rc("s2p_tanh_gauss_rsample_bwd", _ptr(raw), rp, _ptr(eps), ep, _ptr(dlogp), _ptr(da), _ptr(da2), dap, M, A, _ptr(draw), dwp, 0, _st())

    assert bwd() == 0 and bwd(M=0, raw=None, eps=None, dlogp=None, draw=None) == 0 and bwd(A=0, raw=None) == 0
    for bad in (dict(M=-1), dict(A=-1), dict(raw=None), dict(eps=None), dict(dlogp=None), dict(draw=None), dict(rp=5), dict(ep=2),
                dict(dwp=5), dict(da=out, dap=2), dict(da2=out)):
        assert bwd(**bad) != 0, bad
    torch.cuda.synchronize()


# ---- s2p_sac_policy_head --------------------------------------------------------------------------------------------------------------------
LR, TE = 1e-4, -3.0


def sac_ref(logp, q1, q2, la0, dtype, tune, steps=1):
    """-> (losses [4], alpha, dlogp, dq1, dq2, log_alpha) after `steps` identical calls (torch.optim.Adam on the scalar)."""
    lp = logp.to(dtype).requires_grad_(True)
    la = torch.full((1,), la0, dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([la], lr=LR)
    alpha_loss, alpha = torch.zeros((), dtype=dtype), torch.ones(1, dtype=dtype)
    for _ in range(steps):
        if tune:
            alpha_loss = -(la * (lp + TE).detach()).mean()
            opt.zero_grad()
            alpha_loss.backward()
            opt.step()
            alpha = la.detach().exp()
    if q1 is None:
        loss = (alpha * lp).mean()
        dlp, = torch.autograd.grad(loss, lp)
        return torch.stack([alpha_loss.detach(), loss.detach(), loss.detach(), lp.mean().detach()]), alpha, dlp, None, None, la.detach()
    a, b = q1.to(dtype).requires_grad_(True), q2.to(dtype).requires_grad_(True)
    qm = torch.min(a, b)
    loss = (alpha * lp - qm).mean()
    dlp, da, db = torch.autograd.grad(loss, (lp, a, b))
    return (torch.stack([alpha_loss.detach(), loss.detach(), (alpha * lp).mean().detach(), (lp - qm).mean().detach()]), alpha, dlp, da, db,
            la.detach())


@pytest.mark.parametrize("B", [1, 37, 1030])
@pytest.mark.parametrize("tune", [1, 0])
@pytest.mark.parametrize("cloning", [False, True])
def test_sac_policy_head(hip_device, B, tune, cloning):
    dev, g = hip_device, torch.Generator().manual_seed(B + tune)
    logp, q1, q2 = torch.randn(B, generator=g) * 3 - 2, torch.randn(B, generator=g) * 5, torch.randn(B, generator=g) * 5
    q2[0] = q1[0]                                                                     # a tie: the gradient is split in halves
    if B > 2:
        q2[1], q2[2] = q1[1] + 1, q1[2] - 1
    la0 = 0.3
    qa, qb = (None, None) if cloning else (q1, q2)
    state = torch.tensor([la0, 0.0, 0.0], device=dev)
    step, alpha, losses = torch.zeros(1, dtype=torch.int32, device=dev), torch.full((1,), 7.0, device=dev), torch.full((5,), 7.0, device=dev)
    dlp, d1, d2 = (torch.full((B,), 7.0, device=dev) for _ in range(3))
    lpd, q1d, q2d = logp.to(dev), None if cloning else q1.to(dev), None if cloning else q2.to(dev)
    args = (_ptr(lpd), _ptr(q1d), _ptr(q2d), B, tune, TE, LR, 0.9, 0.999, 1e-8, _ptr(state), _ptr(step), _ptr(alpha), _ptr(losses), _ptr(dlp),
            None if cloning else _ptr(d1), None if cloning else _ptr(d2), _st())
    _call("s2p_sac_policy_head", *args)
    r64, r32 = sac_ref(logp, qa, qb, la0, torch.float64, tune), sac_ref(logp, qa, qb, la0, torch.float32, tune)
    tag = "B %d tune %d cloning %d" % (B, tune, cloning)
    for i, name in enumerate(("alpha_loss", "policy_loss", "alpha logp", "statistic")):
        _check("sac head", losses[i], r64[0][i], r32[0][i], "%s %s" % (name, tag))
    assert float(losses[4]) == 7.0
    _check("sac head", alpha, r64[1], r32[1], "alpha")
    _check("sac head", dlp, r64[2], r32[2], "dlogp")
    if not cloning:
        _check("sac head", d1, r64[3], r32[3], "dq1")
        _check("sac head", d2, r64[4], r32[4], "dq2")
        assert float(d1[0]) == float(d2[0]) and abs(float(d1[0]) + 0.5 / B) < 1e-7 / B and bool(((d1 == 0) != (d2 == 0))[1:].all())
    assert int(step) == tune and (tune or torch.equal(state.cpu(), torch.tensor([la0, 0.0, 0.0])))
    if tune:
        _check("sac head", state[0], r64[5], r32[5], "log_alpha after one step")
        _call("s2p_sac_policy_head", *args)
        _call("s2p_sac_policy_head", *args)
        t64, t32 = sac_ref(logp, qa, qb, la0, torch.float64, 1, 3), sac_ref(logp, qa, qb, la0, torch.float32, 1, 3)
        _check("sac head", state[0], t64[5], t32[5], "log_alpha after three steps against torch.optim.Adam")
        assert int(step) == 3
    # repeatability: the same state in, the same bits out
    outs = []
    for _ in range(2):
        state.copy_(torch.tensor([la0, 0.01, 0.002])); step.fill_(4)
        _call("s2p_sac_policy_head", *args)
        outs.append([x.clone() for x in (state, alpha, losses, dlp, d1, d2)])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_sac_policy_head_refusals(hip_device):
    dev, B = hip_device, 8
    lp, q, state, alpha, losses = (torch.zeros(n, device=dev) for n in (B, B, 3, 1, 4))
    step = torch.zeros(1, dtype=torch.int32, device=dev)

    def rc(logp=lp, q1=q, q2=q, B=B, tune=1, state=state, step=step, alpha=alpha, dq1=None, dq2=None):
        return _rc("s2p_sac_policy_head", _ptr(logp), _ptr(q1), _ptr(q2), B, tune, TE, LR, 0.9, 0.999, 1e-8, _ptr(state), _ptr(step), _ptr(alpha),
                   _ptr(losses), None, _ptr(dq1), _ptr(dq2), _st())

    assert rc() == 0 and rc(B=0, logp=None, alpha=None, state=None, step=None) == 0 and rc(tune=0, state=None, step=None) == 0
    for bad in (dict(B=-1), dict(logp=None), dict(alpha=None), dict(q1=None), dict(q2=None), dict(state=None), dict(step=None),
                dict(q1=None, q2=None, dq1=q)):
        assert rc(**bad) != 0, bad
    torch.cuda.synchronize()


# ---- s2p_cql_critic_head --------------------------------------------------------------------------------------------------------------------
def cql_ref_head(x, A, temp, w, det, dtype, rs=1.5, disc=0.99):
    qp, qs = x["q_pred"].to(dtype).requires_grad_(True), x["q_samp"].to(dtype).requires_grad_(True)
    lps, tq, nlp, alpha, r, t = (x[k].to(dtype) for k in ("logp_samp", "tq", "new_log_pi", "alpha", "reward", "terminal"))
    Rn = lps.shape[1] // 2
    tqv = torch.min(tq[0], tq[1])
    if not det:
        tqv = tqv - alpha * nlp
    qt = rs * r + (1.0 - t) * disc * tqv
    density = math.log(0.5 ** A)
    losses, mins, stds = [], [], []
    for i in range(2):
        rand, nxt, cur = qs[i][:, :Rn], qs[i][:, Rn:2 * Rn], qs[i][:, 2 * Rn:]
        stds.append(torch.std(torch.cat([rand, qp[i][:, None], nxt, cur], 1), dim=1).mean())
        cat = torch.cat([rand - density, nxt - lps[:, :Rn], cur - lps[:, Rn:]], 1)
        mins.append(torch.logsumexp(cat / temp, dim=1).mean() * w * temp - qp[i].mean() * w)
        losses.append(((qp[i] - qt) ** 2).mean() + mins[i])
    dqp, dqs = torch.autograd.grad(losses[0] + losses[1], (qp, qs))
    return torch.stack(losses + mins).detach(), dqp, dqs, qt, torch.stack(stds).detach()


@pytest.mark.parametrize("B", [1, 37, 1030])
@pytest.mark.parametrize("Rn", [1, 4, 10])
def test_cql_critic_head(hip_device, B, Rn):
    """Q values of magnitude 80 (an unshifted exp overflows fp32 at 89 / temp), terminals, both temperatures and both backup forms;
    the two networks' blocks lie a stride wider than the block apart, and the gap keeps its canary."""
    dev, A, w = hip_device, 3, 5.0
    g = torch.Generator().manual_seed(B * 100 + Rn)
    x = dict(q_pred=torch.randn(2, B, generator=g) * 40 + 60, q_samp=torch.randn(2, B, 3 * Rn, generator=g) * 30 + 70,
             logp_samp=torch.randn(B, 2 * Rn, generator=g) * 3, tq=torch.randn(2, B, generator=g) * 40,
             new_log_pi=torch.randn(B, generator=g) * 2, alpha=torch.tensor([0.7]), reward=torch.randn(B, generator=g),
             terminal=(torch.rand(B, generator=g) < 0.4).float())
    x["terminal"][0] = 1.0
    assert float(x["q_samp"].abs().max()) >= 80 or B == 1
    d = {k: v.to(dev) for k, v in x.items()}
    sp, ss = B + 3, B * 3 * Rn + 5
    qp = torch.full((2, sp), 7.0, device=dev); qp[:, :B] = d["q_pred"]
    qs = torch.full((2, ss), 7.0, device=dev); qs[:, :B * 3 * Rn] = d["q_samp"].reshape(2, -1)
    for temp in (0.5, 1.0):
        for det in (0, 1):
            losses, std, qt = torch.full((5,), 7.0, device=dev), torch.full((2,), 7.0, device=dev), torch.full((B,), 7.0, device=dev)
            dqp, dqs = torch.full((2, sp), 7.0, device=dev), torch.full((2, ss), 7.0, device=dev)
            args = (_ptr(qp), sp, _ptr(qs), ss, _ptr(d["logp_samp"]), _ptr(d["tq"]), None if det else _ptr(d["new_log_pi"]),
                    None if det else _ptr(d["alpha"]), _ptr(d["reward"]), _ptr(d["terminal"]), B, Rn, A, 1.5, 0.99, temp, w, det, _ptr(losses),
                    _ptr(dqp), sp, _ptr(dqs), ss, _ptr(qt), _ptr(std), _st())
            _call("s2p_cql_critic_head", *args)
            r64, r32 = cql_ref_head(x, A, temp, w, det, torch.float64), cql_ref_head(x, A, temp, w, det, torch.float32)
            tag = "B %d R %d temp %.1f det %d" % (B, Rn, temp, det)
            for i, name in enumerate(("qf1", "qf2", "min_qf1", "min_qf2")):
                _check("cql head", losses[i], r64[0][i], r32[0][i], "%s %s" % (name, tag))
            _check("cql head", dqp[:, :B], r64[1], r32[1], "dq_pred")
            _check("cql head", dqs[:, :B * 3 * Rn].reshape(2, B, -1), r64[2], r32[2], "dq_samp")
            _check("cql head", qt, r64[3], r32[3], "q_target")
            for i in range(2):
                _check("cql head", std[i], r64[4][i], r32[4][i], "std %d" % i)
            assert float(losses[4]) == 7.0 and bool((dqp[:, B:] == 7.0).all()) and bool((dqs[:, B * 3 * Rn:] == 7.0).all())
            assert bool(torch.isfinite(losses[:4]).all())
            first = [v.clone() for v in (losses, dqp, dqs, qt, std)]
            _call("s2p_cql_critic_head", *args)
            assert all(torch.equal(a, b) for a, b in zip(first, (losses, dqp, dqs, qt, std)))
    only = torch.full((4,), 7.0, device=dev)                                          # one output alone
    _call("s2p_cql_critic_head", *args[:18], _ptr(only), None, 0, None, 0, None, None, _st())
    assert torch.equal(only, losses[:4])


def test_cql_critic_head_refusals(hip_device):
    dev, B, Rn = hip_device, 8, 2
    z = {k: torch.zeros(n, device=dev) for k, n in dict(qp=2 * B, qs=2 * B * 3 * Rn, lps=B * 2 * Rn, tq=2 * B, v=B, one=1, out=4).items()}

    def rc(qp=z["qp"], sp=B, qs=z["qs"], ss=B * 3 * Rn, lps=z["lps"], tq=z["tq"], nlp=z["v"], alpha=z["one"], r=z["v"], t=z["v"], B=B, Rn=Rn, A=3,
           temp=1.0, det=0, losses=z["out"], dqp=None, dsp=0, dqs=None, dss=0):
        return _rc("s2p_cql_critic_head", _ptr(qp), sp, _ptr(qs), ss, _ptr(lps), _ptr(tq), _ptr(nlp), _ptr(alpha), _ptr(r), _ptr(t), B, Rn, A, 1.0,
                   0.99, temp, 5.0, det, _ptr(losses), _ptr(dqp), dsp, _ptr(dqs), dss, None, None, _st())

    assert rc() == 0 and rc(B=0, qp=None, qs=None, lps=None, tq=None, r=None, t=None, losses=None) == 0
    assert rc(det=1, nlp=None, alpha=None) == 0
    for bad in (dict(B=-1), dict(Rn=-1), dict(Rn=0), dict(A=-1), dict(qp=None), dict(qs=None), dict(lps=None), dict(tq=None), dict(r=None),
                dict(t=None), dict(nlp=None), dict(alpha=None), dict(losses=None), dict(temp=0.0), dict(temp=-1.0), dict(sp=B - 1),
                dict(ss=B * 3 * Rn - 1), dict(dqp=z["qp"], dsp=B - 1), dict(dqs=z["qs"], dss=1)):
        assert rc(**bad) != 0, bad
    torch.cuda.synchronize()


def test_zz_report_worst_ratios(hip_device):
    print("\nworst deviation / max(ref32_err, 1e-6) per group:", {k: round(v, 3) for k, v in WORST.items()})
    assert WORST and max(WORST.values()) <= K_TOL
