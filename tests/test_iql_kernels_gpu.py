"""Kernel-level parity of csrc/mlp.hip and csrc/iql.hip through the C ABI against float64 torch on the CPU: the grouped ReLU linear layer forward and
backward (MFMA tiles for N > 16, dot-product kernels for the N = 1 / N = 2 A last layers), the two fused loss heads, the Polyak
update, the refused arguments, and bitwise repeatability of every entry point.

Tolerance: the project's rule (tests/test_ensemble_train_gpu.py) -- per quantity K_TOL x max(ref32_err, 1e-6), K_TOL = 4, ref32_err
being the deviation of the SAME formula run in fp32 torch on the CPU from its fp64 run (relative to the fp64 maximum): the kernels
are the same fp32 arithmetic in another summation order.  s2p_soft_update is compared BITWISE with `t * (1 - tau) + s * tau` in fp32
torch on the host: the kernel rounds both products and the sum separately (no fused multiply-add), and 1 - tau is formed in double
and rounded once on both sides, so there is nothing left to differ by.
Worst observed ratios: DESIGN.md section 6b.4 (printed by test_zz_report_worst_ratios)."""
import math

import numpy as np
import pytest
import torch

import iql_ref as R

pytestmark = pytest.mark.gpu
K_TOL, FLOOR = 4.0, 1e-6
WORST = {}


def _check(group, got, f64, f32, what=""):
    err, ref = R.rel_max(got.cpu(), f64), max(R.rel_max(f32, f64), FLOOR)
    WORST[group] = max(WORST.get(group, 0.0), err / ref)
    print("%-16s %-34s err %.3e  ref32_err %.3e  ratio %.3f" % (group, what, err, ref, err / ref))
    assert err <= K_TOL * ref, (group, what, err, K_TOL * ref)


def _L():
    from s2p_amd import _lib
    return _lib


def _ptr(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def pad4(n):
    return (n + 3) // 4 * 4


class Group:
    """One group's host data (fp32) and device copies; K is padded to a multiple of 4 with zeros, pitches are wider than the rows."""

    def __init__(self, rows, K, N, dev, g, zero_pre=False):
        self.rows, self.K, self.N, self.kp = rows, K, N, pad4(K)
        self.x = torch.randn(rows, K, generator=g)
        self.w = torch.randn(N, K, generator=g) / math.sqrt(K)
        self.b = torch.randn(N, generator=g) * 0.1
        self.dpre = torch.randn(rows, N, generator=g)
        self.pre_prev = torch.randn(rows, K, generator=g)
        if zero_pre:                                   # exact zeros in the forward's pre-activation and in the backward's mask
            self.w[1] = 0; self.b[1] = 0
            self.pre_prev[:, 2] = 0
            self.pre_prev[0] = 0
        self.xp, self.yp, self.dp, self.pp = self.kp + 4, N + 3, pad4(N) + 4, self.kp + 8
        self.xd = torch.zeros(rows, self.xp, device=dev); self.xd[:, :K] = self.x.to(dev)
        self.wd = torch.zeros(N, self.kp, device=dev); self.wd[:, :K] = self.w.to(dev)
        self.bd = self.b.to(dev)
        self.dpd = torch.zeros(rows, self.dp, device=dev); self.dpd[:, :N] = self.dpre.to(dev)
        self.ppd = torch.zeros(rows, self.pp, device=dev); self.ppd[:, :K] = self.pre_prev.to(dev)

    def ref_fwd(self, dtype, relu):
        pre = self.x.to(dtype) @ self.w.to(dtype).t() + self.b.to(dtype)
        return pre, (torch.relu(pre) if relu else pre)

    def ref_bwd(self, dtype, relu):
        d, x, w = self.dpre.to(dtype), self.x.to(dtype), self.w.to(dtype)
        dprev = d @ w
        if relu:
            dprev = dprev * (self.pre_prev.to(dtype) > 0)
        return d.t() @ x, d.sum(0), dprev


def run_fwd(groups, N, relu, dev, want_pre=True, want_act=True):
    L = _L()
    outs = [(torch.full((g.rows, g.yp), 7.0, device=dev) if want_pre else None, torch.full((g.rows, g.yp), 7.0, device=dev) if want_act else None)
            for g in groups]
    arr = (L.MlpFwdGroup * len(groups))(*[L.MlpFwdGroup(_ptr(g.xd), _ptr(g.wd), _ptr(g.bd), _ptr(p), _ptr(a), g.xp, g.yp, g.rows, g.kp)
                                          for g, (p, a) in zip(groups, outs)])
    L.check(L.lib().s2p_mlp_linear_fwd(arr, len(groups), N, L.ACT_RELU if relu else L.ACT_NONE, _st()), "s2p_mlp_linear_fwd")
    torch.cuda.synchronize()
    return outs


def run_bwd(groups, N, relu, dev, want_dprev=True):
    L = _L()
    outs = [(torch.full((N, g.kp), 7.0, device=dev), torch.full((N,), 7.0, device=dev),
             torch.full((g.rows, g.pp), 7.0, device=dev) if want_dprev else None) for g in groups]
    arr = (L.MlpBwdGroup * len(groups))(*[
        L.MlpBwdGroup(_ptr(g.xd), _ptr(g.dpd), _ptr(g.wd), _ptr(dw), _ptr(db), _ptr(g.ppd) if relu else None, _ptr(dp), g.xp, g.dp, g.pp,
                      g.rows, g.kp) for g, (dw, db, dp) in zip(groups, outs)])
    L.check(L.lib().s2p_mlp_linear_bwd(arr, len(groups), N, L.ACT_RELU if relu else L.ACT_NONE, _st()), "s2p_mlp_linear_bwd")
    torch.cuda.synchronize()
    return outs


def check_layer(groups, N, relu, dev, tag):
    for g, (pre, act) in zip(groups, run_fwd(groups, N, relu, dev)):
        (p64, a64), (p32, a32) = g.ref_fwd(torch.float64, relu), g.ref_fwd(torch.float32, relu)
        _check("layer forward", pre[:, :N], p64, p32, "%s pre rows %d K %d N %d" % (tag, g.rows, g.K, N))
        _check("layer forward", act[:, :N], a64, a32, "%s act" % tag)
        assert bool((pre[:, N:] == 7.0).all()) and bool((act[:, N:] == 7.0).all())           # nothing written beyond the row
        if relu:
            assert bool(((act[:, :N] == 0) == (pre[:, :N] <= 0)).all())
    for g, (dw, db, dprev) in zip(groups, run_bwd(groups, N, relu, dev)):
        (w64, b64, d64), (w32, b32, d32) = g.ref_bwd(torch.float64, relu), g.ref_bwd(torch.float32, relu)
        _check("layer backward", dw[:, :g.K], w64, w32, "%s dw rows %d K %d N %d" % (tag, g.rows, g.K, N))
        assert bool((dw[:, g.K:] == 0).all())                                                # the K padding's gradient is exactly zero
        _check("layer backward", db, b64, b32, "%s db" % tag)
        _check("layer backward", dprev[:, :g.K], d64, d32, "%s dprev" % tag)
        assert bool((dprev[:, g.kp:] == 7.0).all())
        if relu:
            assert bool((dprev[:, :g.K].cpu()[g.pre_prev <= 0] == 0).all())                  # masked where pre_prev <= 0, zeros included


@pytest.mark.parametrize("B", [37, 130])
@pytest.mark.parametrize("N", [64, 96])
def test_grouped_layer_unequal_widths_and_a_two_b_row_group(hip_device, B, N):
    """Q-like groups of K = 52 on B rows beside a vf-like group of K = 44 on 2 B rows: the row tail (37), one row past the 128-row
    tile (130, and 260 in the 2 B group), the column tail of the 64-wide wave tile (96), exact zeros in pre and in the mask."""
    g = torch.Generator().manual_seed(B * 1000 + N)
    groups = [Group(B, 52, N, hip_device, g, zero_pre=True), Group(B, 52, N, hip_device, g), Group(2 * B, 44, N, hip_device, g, zero_pre=True)]
    check_layer(groups, N, True, hip_device, "tile")
    check_layer(groups[1:], N, False, hip_device, "tile identity")


@pytest.mark.parametrize("N", [1, 6])
def test_last_layers_on_the_dot_product_kernels(hip_device, N):
    g = torch.Generator().manual_seed(N)
    groups = [Group(37, 64, N, hip_device, g, zero_pre=(N > 2)), Group(260, 96, N, hip_device, g), Group(130, 1024, N, hip_device, g)]
    check_layer(groups, N, True, hip_device, "dot")          # (the forward's activation argument is honoured here too)
    check_layer(groups[:2], N, False, hip_device, "dot identity")


def test_one_group_and_optional_outputs(hip_device):
    g = torch.Generator().manual_seed(5)
    grp = Group(37, 44, 64, hip_device, g)
    check_layer([grp], 64, True, hip_device, "G = 1")
    (pre, act), = run_fwd([grp], 64, True, hip_device, want_pre=False)
    assert pre is None and R.rel_max(act[:, :64].cpu(), grp.ref_fwd(torch.float64, True)[1]) < 1e-5
    (dw, db, dprev), = run_bwd([grp], 64, True, hip_device, want_dprev=False)
    assert dprev is None and R.rel_max(dw[:, :44].cpu(), grp.ref_bwd(torch.float64, True)[0]) < 1e-5


def test_sizes_of_zero_are_no_ops(hip_device):
    L = _L()
    lib = L.lib()
    assert lib.s2p_mlp_linear_fwd(None, 0, 64, L.ACT_RELU, _st()) == 0 and lib.s2p_mlp_linear_fwd(None, 3, 0, L.ACT_RELU, _st()) == 0
    assert lib.s2p_mlp_linear_bwd(None, 0, 64, L.ACT_RELU, _st()) == 0 and lib.s2p_mlp_linear_bwd(None, 3, 0, L.ACT_RELU, _st()) == 0
    empty = L.MlpFwdGroup(None, None, None, None, None, 0, 0, 0, 44)       # rows == 0: the group is skipped, no pointer looked at
    g = torch.Generator().manual_seed(6)
    grp = Group(5, 44, 64, hip_device, g)
    out = torch.full((5, grp.yp), 7.0, device=hip_device)
    arr = (L.MlpFwdGroup * 2)(empty, L.MlpFwdGroup(_ptr(grp.xd), _ptr(grp.wd), _ptr(grp.bd), _ptr(out), None, grp.xp, grp.yp, 5, grp.kp))
    assert lib.s2p_mlp_linear_fwd(arr, 2, 64, L.ACT_NONE, _st()) == 0
    assert R.rel_max(out[:, :64].cpu(), grp.ref_fwd(torch.float64, False)[0]) < 1e-5
    assert lib.s2p_mlp_linear_fwd((L.MlpFwdGroup * 1)(empty), 1, 64, L.ACT_NONE, _st()) == 0
    bempty = L.MlpBwdGroup(None, None, None, None, None, None, None, 0, 0, 0, 0, 44)
    assert lib.s2p_mlp_linear_bwd((L.MlpBwdGroup * 1)(bempty), 1, 64, L.ACT_NONE, _st()) == 0
    assert lib.s2p_iql_critic_head(*([None] * 8), 0, 1.0, 0.99, 0.7, 0.1, 100.0, *([None] * 7), _st()) == 0
    assert lib.s2p_tanh_gauss_policy_head(None, 0, None, 0, None, 0, 3, None, None, 0, None, _st()) == 0
    assert lib.s2p_soft_update(None, None, 0, 0.005, _st()) == 0
    torch.cuda.synchronize()


def test_refused_arguments(hip_device):
    L = _L()
    lib, dev = L.lib(), hip_device
    g = torch.Generator().manual_seed(7)
    grp = Group(8, 44, 64, dev, g)
    out = torch.empty(8, grp.yp, device=dev)

    def fwd(**kw):
        f = dict(x=_ptr(grp.xd), w=_ptr(grp.wd), bias=_ptr(grp.bd), pre=_ptr(out), act=None, x_pitch=grp.xp, y_pitch=grp.yp, rows=8, K=grp.kp)
        f.update(kw)
        return lib.s2p_mlp_linear_fwd((L.MlpFwdGroup * 1)(L.MlpFwdGroup(*f.values())), 1, 64, L.ACT_RELU, _st())

    assert fwd() == 0
    for bad in (dict(x=None), dict(w=None), dict(bias=None), dict(pre=None), dict(x_pitch=40), dict(y_pitch=60), dict(x_pitch=grp.kp + 2),
                dict(K=42), dict(x=_ptr(grp.xd) + 4), dict(w=_ptr(grp.wd) + 8), dict(rows=-1)):
        assert fwd(**bad) != 0, bad
        assert lib.s2p_last_error()
    arr1 = (L.MlpFwdGroup * 1)(L.MlpFwdGroup(_ptr(grp.xd), _ptr(grp.wd), _ptr(grp.bd), _ptr(out), None, grp.xp, grp.yp, 8, grp.kp))
    assert lib.s2p_mlp_linear_fwd(arr1, 1, 64, L.ACT_SWISH, _st()) != 0            # relu and none only
    assert lib.s2p_mlp_linear_fwd(arr1, 9, 64, L.ACT_RELU, _st()) != 0             # at most 8 groups
    assert lib.s2p_mlp_linear_fwd(None, 1, 64, L.ACT_RELU, _st()) != 0 and lib.s2p_mlp_linear_fwd(arr1, -1, 64, L.ACT_RELU, _st()) != 0
    dw, db, dprev = torch.empty(64, grp.kp, device=dev), torch.empty(64, device=dev), torch.empty(8, grp.pp, device=dev)

    def bwd(N=64, **kw):
        f = dict(x=_ptr(grp.xd), dpre=_ptr(grp.dpd), w=_ptr(grp.wd), dw=_ptr(dw), db=_ptr(db), pre_prev=_ptr(grp.ppd), dprev=_ptr(dprev),
                 x_pitch=grp.xp, dpre_pitch=grp.dp, prev_pitch=grp.pp, rows=8, K=grp.kp)
        f.update(kw)
        return lib.s2p_mlp_linear_bwd((L.MlpBwdGroup * 1)(L.MlpBwdGroup(*f.values())), 1, N, L.ACT_RELU, _st())

    assert bwd() == 0
    for bad in (dict(x=None), dict(dpre=None), dict(dw=None), dict(db=None), dict(w=None), dict(pre_prev=None), dict(x_pitch=40),
                dict(dpre_pitch=60), dict(prev_pitch=40), dict(dpre_pitch=grp.dp + 2), dict(dpre=_ptr(grp.dpd) + 4), dict(N=18)):
        assert bwd(**bad) != 0, bad
    v = torch.zeros(8, device=dev)
    p = [_ptr(v)] * 8

    def critic(inputs=p, B=8, beta=0.1, outs=None):
        return lib.s2p_iql_critic_head(*inputs, B, 1.0, 0.99, 0.7, beta, 100.0, *(outs or [_ptr(torch.empty(3, device=dev))] + [None] * 6), _st())

    assert critic() == 0
    assert critic(inputs=[None] + p[1:]) != 0 and critic(inputs=p[:7] + [None]) != 0 and critic(B=-1) != 0 and critic(beta=0.0) != 0
    assert critic(outs=[None] * 7) != 0
    raw, act, w = torch.zeros(8, 6, device=dev), torch.zeros(8, 3, device=dev), torch.ones(8, device=dev)
    loss = torch.empty(1, device=dev)

    def pol(raw_=_ptr(raw), rp=6, act_=_ptr(act), ap=3, w_=_ptr(w), loss_=_ptr(loss), draw=None, dwp=0):
        return lib.s2p_tanh_gauss_policy_head(raw_, rp, act_, ap, w_, 8, 3, loss_, draw, dwp, None, _st())

    assert pol() == 0
    assert pol(raw_=None) != 0 and pol(act_=None) != 0 and pol(w_=None) != 0 and pol(rp=5) != 0 and pol(ap=2) != 0 and pol(loss_=None) != 0
    assert pol(draw=_ptr(raw), dwp=5) != 0
    t = torch.zeros(16, device=dev)
    assert lib.s2p_soft_update(_ptr(t), _ptr(t[8:]), 4, 0.005, _st()) == 0
    assert lib.s2p_soft_update(None, _ptr(t), 4, 0.005, _st()) != 0 and lib.s2p_soft_update(_ptr(t), None, 4, 0.005, _st()) != 0
    assert lib.s2p_soft_update(_ptr(t) + 4, _ptr(t[8:]), 4, 0.005, _st()) != 0 and lib.s2p_soft_update(_ptr(t), _ptr(t) + 4, 4, 0.005, _st()) != 0
    assert lib.s2p_soft_update(_ptr(t), _ptr(t[8:]), -1, 0.005, _st()) != 0
    torch.cuda.synchronize()


# ---- the heads ---------------------------------------------------------------------------------------------------------------------
CRITIC = dict(reward_scale=1.5, discount=0.99, quantile=0.7, beta=0.1, clip=100.0)


def critic_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    t = {k: torch.randn(B, generator=g) for k in ("q1", "q2", "tq1", "tq2", "v", "v_next", "reward")}
    t["v"] = torch.minimum(t["tq1"], t["tq2"]) + torch.randn(B, generator=g) * 0.4       # adv / beta on both sides of log(100) = 4.6
    t["terminal"] = (torch.rand(B, generator=g) < 0.4).float()
    return t


def critic_ref(t, dtype, c=CRITIC):
    t = {k: v.to(dtype) for k, v in t.items()}
    qt = c["reward_scale"] * t["reward"] + (1.0 - t["terminal"]) * c["discount"] * t["v_next"]
    qp = torch.min(t["tq1"], t["tq2"])
    err = t["v"] - qp
    w = torch.where(err > 0, torch.tensor(1 - np.float32(c["quantile"]), dtype=dtype), torch.tensor(np.float32(c["quantile"]), dtype=dtype))
    B = len(qt)
    return dict(losses=torch.stack([((t["q1"] - qt) ** 2).mean(), ((t["q2"] - qt) ** 2).mean(), (w * err ** 2).mean()]),
                dq1=2 * (t["q1"] - qt) / B, dq2=2 * (t["q2"] - qt) / B, dv=2 * w * err / B,
                weights=torch.clamp(torch.exp(-err / c["beta"]), max=c["clip"]), adv=-err, q_target=qt)


def run_critic(t, dev, c=CRITIC, optional=True):
    L = _L()
    B = len(t["q1"])
    d = {k: v.to(dev) for k, v in t.items()}
    out = dict(losses=torch.full((3,), 7.0, device=dev), **{k: torch.full((B,), 7.0, device=dev) for k in ("dq1", "dq2", "dv", "weights")})
    if optional:
        out.update(adv=torch.full((B,), 7.0, device=dev), q_target=torch.full((B,), 7.0, device=dev))
    L.check(L.lib().s2p_iql_critic_head(*[_ptr(d[k]) for k in ("q1", "q2", "tq1", "tq2", "v", "v_next", "reward", "terminal")], B,
                                        c["reward_scale"], c["discount"], c["quantile"], c["beta"], c["clip"],
                                        *[_ptr(out.get(k)) for k in ("losses", "dq1", "dq2", "dv", "weights", "adv", "q_target")], _st()),
            "s2p_iql_critic_head")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B", [1, 37, 1025])
def test_critic_head(hip_device, B):
    t = critic_inputs(B, B)
    r64, r32 = critic_ref(t, torch.float64), critic_ref(t, torch.float32)
    if B > 1:
        err = r64["adv"]
        assert (err > 0).any() and (err < 0).any() and (r64["weights"] == 100).any() and (r64["weights"] < 100).any() and t["terminal"].sum() > 0
    out = run_critic(t, hip_device)
    for k in r64:
        _check("critic head", out[k], r64[k], r32[k], "B %d %s" % (B, k))
    assert sorted(run_critic(t, hip_device, optional=False)) == ["dq1", "dq2", "dv", "losses", "weights"]
    no_clip = run_critic(t, hip_device, dict(CRITIC, clip=float("inf")))
    assert R.rel_max(no_clip["weights"].cpu(), torch.exp(r64["adv"] / 0.1)) < 1e-4


def policy_inputs(B, A, seed):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(B, 2 * A, generator=g)
    raw[:, A:] = raw[:, A:] * 1.5 - 0.5
    raw[0, A], raw[B - 1, 2 * A - 1] = 2.5, -21.0                       # both sides of the clamp on the log std
    if B > 2:
        raw[1, A], raw[2, A] = 2.0, -20.0                                # ... and exactly on it: the gradient passes
    action = torch.rand(B, A, generator=g) * 1.96 - 0.98
    action[0, 0], action[B - 1, A - 1] = 1.0, -0.9999995                 # beyond the clamp on the action
    return raw, action, torch.rand(B, generator=g) * 3


def policy_ref(raw, action, weights, dtype):
    """The formula of SPEC.md N3d.  v = clamp(action) and 1 + v, 1 - v are formed in fp32 in BOTH precisions: they are inputs of the
    logarithms whose fp32 rounding (6 % of 1 - v at the clamp) is the reference's own, not an error of the kernel."""
    A = action.shape[1]
    raw = raw.to(dtype).clone().requires_grad_(True)
    v = torch.clamp(action, -0.999999, 0.999999)
    u = torch.log((1 + v).to(dtype)) / 2 - torch.log((1 - v).to(dtype)) / 2
    ls = torch.clamp(raw[:, A:], -20.0, 2.0)
    logp = (-0.5 * ((u - raw[:, :A]) / torch.exp(ls)) ** 2 - ls - 0.5 * math.log(2 * math.pi)).sum(1) \
        - 2.0 * (math.log(2.0) - u - R.softplus(-2.0 * u)).sum(1)
    loss = (-logp * weights.to(dtype)).mean()
    loss.backward()
    return dict(loss=loss.detach(), logp=logp.detach(), draw=raw.grad)


def run_policy(raw, action, weights, dev, want=("loss", "draw", "logp")):
    L = _L()
    B, A = action.shape
    rp, ap, dwp = 2 * A + 3, A + 1, 2 * A + 2
    rd = torch.zeros(B, rp, device=dev); rd[:, :2 * A] = raw.to(dev)
    ad = torch.zeros(B, ap, device=dev); ad[:, :A] = action.to(dev)
    out = dict(loss=torch.full((1,), 7.0, device=dev), draw=torch.full((B, dwp), 7.0, device=dev), logp=torch.full((B,), 7.0, device=dev))
    out = {k: v for k, v in out.items() if k in want}
    L.check(L.lib().s2p_tanh_gauss_policy_head(_ptr(rd), rp, _ptr(ad), ap, _ptr(weights.to(dev)), B, A, _ptr(out.get("loss")),
                                               _ptr(out.get("draw")), dwp, _ptr(out.get("logp")), _st()), "s2p_tanh_gauss_policy_head")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B,A", [(1, 3), (37, 3), (1025, 6)])
def test_policy_head(hip_device, B, A):
    raw, action, w = policy_inputs(B, A, B)
    r64, r32 = policy_ref(raw, action, w, torch.float64), policy_ref(raw, action, w, torch.float32)
    out = run_policy(raw, action, w, hip_device)
    _check("policy head", out["loss"][0], r64["loss"], r32["loss"], "B %d loss" % B)
    _check("policy head", out["logp"], r64["logp"], r32["logp"], "B %d logp" % B)
    _check("policy head", out["draw"][:, :2 * A], r64["draw"], r32["draw"], "B %d draw" % B)
    assert bool((out["draw"][:, 2 * A:] == 7.0).all())
    d = out["draw"].cpu()
    assert float(d[0, A]) == 0.0 and float(d[B - 1, 2 * A - 1]) == 0.0                      # no gradient outside the clamp
    if B > 2:
        assert float(d[1, A]) != 0.0 and float(d[2, A]) != 0.0                              # ... and the gradient on its two ends
    assert sorted(run_policy(raw, action, w, hip_device, want=("logp",))) == ["logp"]


@pytest.mark.parametrize("n", [0, 1, 3, 4, 1027])
def test_soft_update_is_bitwise_the_written_out_fp32_arithmetic(hip_device, n):
    L = _L()
    g = torch.Generator().manual_seed(n)
    t, s, tau = torch.randn(n + 8, generator=g), torch.randn(n + 8, generator=g), 0.005
    td, sd = t.to(hip_device), s.to(hip_device)
    L.check(L.lib().s2p_soft_update(_ptr(td), _ptr(sd), n, tau, _st()), "s2p_soft_update")
    want = t.clone()
    want[:n] = t[:n] * (1.0 - tau) + s[:n] * tau                          # three fp32 element-wise operations, as the reference's
    assert torch.equal(td.cpu(), want)                                    # bitwise, and nothing beyond n touched


def test_two_identical_calls_are_bitwise_identical(hip_device):
    dev = hip_device
    g = torch.Generator().manual_seed(11)
    for N, groups in ((96, [Group(130, 52, 96, dev, g), Group(260, 44, 96, dev, g)]), (6, [Group(130, 1024, 6, dev, g), Group(37, 64, 6, dev, g)])):
        a, b = run_fwd(groups, N, True, dev), run_fwd(groups, N, True, dev)
        assert all(torch.equal(x, y) for pa, pb in zip(a, b) for x, y in zip(pa, pb))
        a, b = run_bwd(groups, N, True, dev), run_bwd(groups, N, True, dev)
        assert all(torch.equal(x, y) for pa, pb in zip(a, b) for x, y in zip(pa, pb))
    t = critic_inputs(1025, 3)
    a, b = run_critic(t, dev), run_critic(t, dev)
    assert all(torch.equal(a[k], b[k]) for k in a)
    p = policy_inputs(1025, 6, 4)
    a, b = run_policy(*p, dev), run_policy(*p, dev)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_zz_report_worst_ratios(hip_device):
    print("\nworst deviation / max(ref32_err, 1e-6) per group:", {k: round(v, 3) for k, v in WORST.items()})
    assert WORST and max(WORST.values()) <= K_TOL
