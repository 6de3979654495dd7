"""Kernel-level parity of csrc/gauss.hip (the SLAC latent model's entry points) against float64 torch on the CPU: ragged sizes,
pitches larger than the row, column offsets != 0, and sentinel-filled guard bands around (and between the rows of) every output.
Tolerances come from the formats: fp32 element-wise results 1e-5 relative (a few ulp of 2^-24 through exp / log), fp32 GEMMs and
sums of up to ~600 terms 2e-5 of the largest magnitude involved, bf16 gradients 2^-8."""
import math

import pytest
import torch
import torch.nn.functional as F

from guard_region import SENT, Region

pytestmark = pytest.mark.gpu

MS = (1, 3, 32, 33, 288)
DS = (1, 32, 256)


def inp(M, width, gen, pitch=None, off=0, scale=1.0):
    x = torch.randn(M, width, generator=gen, dtype=torch.float64) * scale
    return x.float().double(), Region(M, width, pitch, off, fill=x)


def close(got, want, tol, what=""):
    err = float((got - want).abs().max() / (want.abs().max() + 1e-30))
    assert err <= tol, (what, err)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("M", MS)
def test_gauss_head_forward_and_backward(hip_device, M, D):
    from s2p_amd import ops
    g = torch.Generator().manual_seed(1000 * M + D)
    raw, raw_r = inp(M, 2 * D, g, off=4, scale=3.0)
    for i, v in enumerate((40.0, -40.0, 100.0, -100.0)):                     # softplus must neither overflow nor fall below the floor
        raw[(i * 7) % M, D + (i * 5) % D] = v
    raw_r.v.copy_(raw.float())
    eps, eps_r = inp(M, D, g, off=8)
    mean_r, std_r, z_r, z2_r = Region(M, D, off=4), Region(M, D), Region(M, D, off=32, pitch=D + 40), Region(M, D, off=12)
    ops.gauss_head_fwd(raw_r.v, D, eps=eps_r.v, mean=mean_r.v, std=std_r.v, z=z_r.v, z2=z2_r.v)
    mu, sd = raw[:, :D], F.softplus(raw[:, D:]) + 1e-5
    std = std_r.get("std")
    assert torch.equal(mean_r.get("mean"), mu) and bool(torch.isfinite(std).all()) and float(std.min()) >= float(torch.tensor(1e-5))   # (the fp32 floor)
    close(std, sd, 1e-5, "std")
    close(z_r.get("z"), mu + eps * sd, 1e-5, "z")
    assert torch.equal(z2_r.get("z2"), z_r.get())
    # mean / std only (no eps), and the sample alone
    m2, s2 = Region(M, D), Region(M, D)
    ops.gauss_head_fwd(raw_r.v, D, mean=m2.v, std=s2.v)
    assert torch.equal(m2.get(), mu) and torch.equal(s2.get(), std)
    z3 = Region(M, D)
    ops.gauss_head_fwd(raw_r.v, D, eps=eps_r.v, z=z3.v)
    assert torch.equal(z3.get(), z_r.get())
    # backward
    (dmean, dmean_r), (dstd, dstd_r), (dz, dz_r), (dz2, dz2_r) = [inp(M, D, g, off=4 * k) for k in range(4)]
    sig = torch.sigmoid(raw[:, D:])
    for use in ((1, 1, 1, 1), (1, 1, 0, 0), (0, 0, 1, 0), (0, 1, 0, 1)):
        draw_r = Region(M, 2 * D, off=4)
        ops.gauss_head_bwd(raw_r.v, D, draw_r.v, eps=eps_r.v if (use[2] or use[3]) else None, dmean=dmean_r.v if use[0] else None,
                           dstd=dstd_r.v if use[1] else None, dz=dz_r.v if use[2] else None, dz2=dz2_r.v if use[3] else None)
        gz = dz * use[2] + dz2 * use[3]
        want = torch.cat([dmean * use[0] + gz, (dstd * use[1] + gz * eps) * sig], dim=1)
        got = draw_r.get("draw")
        assert bool(torch.isfinite(got).all())
        close(got, want, 1e-5, ("draw", use))


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("Kz,Kr,N", [(256, 264, 256), (288, 8, 256), (32, 4, 64), (4, 12, 20)])
def test_linear_add_forward_and_backward(hip_device, M, Kz, Kr, N):
    """A first layer on cat(x_row, x_z) run as: row term = one plain GEMM, then the additive launch on the z columns."""
    from s2p_amd import ops
    from s2p_amd._lib import ACT_LRELU, ACT_NONE
    g = torch.Generator().manual_seed(M + Kz + N)
    w = (torch.randn(N, Kr + Kz, generator=g, dtype=torch.float64) / (Kr + Kz) ** 0.5).float().double()
    b = (torch.randn(N, generator=g, dtype=torch.float64) * 0.1).float().double()
    xz, xz_r = inp(M, Kz, g, off=32, pitch=Kz + 40)
    xr, xr_r = inp(M, Kr, g)
    wz, wr = w[:, Kr:].float().contiguous().cuda(), w[:, :Kr].float().contiguous().cuda()
    row_r = Region(M, N, off=4)
    ops.linear_fwd_into(xr_r.v, wr, None, N, row_r.v)
    for act in (ACT_LRELU, ACT_NONE):
        y_r = Region(M, N, off=8)
        ops.linear_fwd_into(xz_r.v, wz, b.float().cuda(), N, y_r.v, act, 0.2, add=row_r.v)
        pre = F.linear(torch.cat([xr, xz], dim=1), w, b)
        want = F.leaky_relu(pre, 0.2) if act == ACT_LRELU else pre
        y = y_r.get("y")
        close(y, want, 2e-5, ("fwd", act))
        # n_store > N: the padding columns are written as zeros
        if act == ACT_NONE:
            yp_r = Region(M, N + 4)
            ops.linear_fwd_into(xz_r.v, wz, b.float().cuda(), N, yp_r.v, act, 0.2, add=row_r.v)
            yp = yp_r.get()
            assert torch.equal(yp[:, :N], y) and bool((yp[:, N:] == 0).all())
        # backward: dpre, dx (overwrite and accumulate), dw / db
        dy, dy_r = inp(M, N, g)
        dpre = dy * (torch.where(y > 0, 1.0, 0.2) if act == ACT_LRELU else 1.0)
        yact = y_r.v if act == ACT_LRELU else None
        dadd_r, dx_r = Region(M, N, off=4), Region(M, Kz, off=32, pitch=Kz + 40)
        ops.linear_add_bwd(dy_r.v, yact, N, act, 0.2, w_bwd=wz.t().contiguous(), dx=dx_r.v, dadd=dadd_r.v)
        close(dadd_r.get("dadd"), dpre, 1e-6, "dadd")
        dx = dx_r.get("dx")
        close(dx, dpre @ w[:, Kr:], 2e-5, "dx")
        prev, acc_r = inp(M, Kz, g, off=32, pitch=Kz + 40)
        ops.linear_add_bwd(dy_r.v, yact, N, act, 0.2, w_bwd=wz.t().contiguous(), dx=acc_r.v, accumulate=True)
        close(acc_r.get("dx+="), prev + dpre @ w[:, Kr:], 2e-5, "dx accumulate")
        dw, db = torch.zeros(N, Kz, device="cuda"), torch.zeros(N, device="cuda")
        ops.linear_add_bwd(dy_r.v, yact, N, act, 0.2, x=xz_r.v, k_real=Kz, dw=dw, db=db)
        close(dw.cpu().double(), dpre.t() @ xz, 2e-5, "dw")
        close(db.cpu().double(), dpre.sum(0), 2e-5, "db")


@pytest.mark.parametrize("B,T,D", [(1, 1, 1), (3, 2, 32), (4, 9, 32), (33, 3, 5)])
def test_kl_with_the_constant_first_prior(hip_device, B, T, D):
    from s2p_amd import ops
    g = torch.Generator().manual_seed(B * 100 + T)
    mk = lambda rows: (torch.randn(rows, D, generator=g, dtype=torch.float64).float().double(),
                       (torch.rand(rows, D, generator=g, dtype=torch.float64) + 0.2).float().double())
    (mp, sp), (mq, sq) = mk(B * T), mk(B * (T - 1))
    mp, sp, mq, sq = [t.requires_grad_(True) for t in (mp, sp, mq, sq)]
    qm = torch.cat([torch.zeros(B, 1, D, dtype=torch.float64), mq.view(B, T - 1, D)], 1).reshape(B * T, D)
    qs = torch.cat([torch.ones(B, 1, D, dtype=torch.float64), sq.view(B, T - 1, D)], 1).reshape(B * T, D)
    vr = (sp / qs) ** 2
    want = (0.5 * (vr + ((mp - qm) / qs) ** 2 - 1 - vr.log())).sum() / B
    want.backward()
    loss = torch.full((3,), SENT, device="cuda")
    loss[1] = 0.25                                                           # accumulated into
    dev = [t.detach().float().cuda() for t in (mp, sp, mq, sq)]
    grads = ops.gauss_kl(dev[0], dev[1], dev[2], dev[3], B, T, 1.0 / B, loss[1:2])
    got = loss.cpu().double()
    assert float(got[0]) == float(torch.tensor(SENT)) and float(got[2]) == float(torch.tensor(SENT))
    assert abs(float(got[1]) - 0.25 - float(want)) <= 2e-5 * abs(float(want)) + 1e-6
    for gg, ref, name in zip(grads, (mp, sp, mq, sq), ("dmu_p", "dstd_p", "dmu_q", "dstd_q")):
        if ref.numel():
            close(gg.cpu().double(), ref.grad, 1e-5, name)
    # the non-constant form: q has T steps
    loss2 = torch.zeros(1, device="cuda")
    ops.gauss_kl(dev[0], dev[1], qm.detach().float().cuda(), qs.detach().float().cuda(), B, T, 1.0 / B, loss2, const_first=False,
                 want_grad=False)
    assert abs(float(loss2) - float(want)) <= 2e-5 * abs(float(want)) + 1e-6


@pytest.mark.parametrize("n", (1, 3, 32, 33, 288))
def test_masked_reward_likelihood(hip_device, n):
    from s2p_amd import ops
    g = torch.Generator().manual_seed(n)
    mu = torch.randn(n, 1, generator=g, dtype=torch.float64).float().double().requires_grad_(True)
    sd = (torch.rand(n, 1, generator=g, dtype=torch.float64) + 0.1).float().double().requires_grad_(True)
    r = torch.randn(n, generator=g, dtype=torch.float64).float().double()
    for done in ((torch.rand(n, generator=g) < 0.3).double(), torch.ones(n, dtype=torch.float64)):     # (an all-ones row: loss 0)
        mu.grad = sd.grad = None
        nll = 0.5 * ((r - mu[:, 0]) / (sd[:, 0] + 1e-8)) ** 2 + sd[:, 0].log() + 0.5 * math.log(2 * math.pi)
        want = (nll * (1 - done)).sum() / 4
        want.backward()
        loss = torch.zeros(1, device="cuda")
        mu_r, sd_r = Region(n, 1, pitch=3, off=1, fill=mu.detach()), Region(n, 1, pitch=2, off=0, fill=sd.detach())
        dmu, dsd = ops.gauss_ll(mu_r.v, sd_r.v, r.float().cuda(), done.float().cuda(), 0.25, loss)
        assert abs(float(loss) - float(want)) <= 2e-5 * abs(float(want)) + 1e-7
        close(dmu.cpu().double(), mu.grad[:, 0], 1e-5 if float(mu.grad.abs().max()) > 0 else 0.0, "dmu")
        close(dsd.cpu().double(), sd.grad[:, 0], 1e-5 if float(sd.grad.abs().max()) > 0 else 0.0, "dstd")
        if float(done.min()) == 1.0:
            assert float(loss) == 0.0 and float(dmu.abs().max()) == 0.0 and float(dsd.abs().max()) == 0.0


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
@pytest.mark.parametrize("N,H,W", [(1, 1, 1), (3, 5, 7), (2, 100, 100)])
@pytest.mark.parametrize("u8", (False, True))
def test_image_likelihood_and_its_gradient_layout(hip_device, dtype, N, H, W, u8):
    from s2p_amd import ops
    g = torch.Generator().manual_seed(N * H + W)
    ce = 4 if dtype == torch.float32 else 8
    C, sigma, scale = 3, 0.1 ** 0.5, 0.25
    frames = (torch.rand(N, H, W, C, generator=g) * 255).round().to(torch.uint8)
    x = frames.double() / 255.0                                              # NHWC, [0,1]
    mu = torch.full((N, H, W, ce), SENT, dtype=torch.float32)                # padded channels hold garbage: they must not be read
    mu[..., :C] = torch.rand(N, H, W, C, generator=g)
    mu = mu.to(dtype)
    m64 = mu[..., :C].double()
    want = (0.5 * ((x - m64) / (sigma + 1e-8)) ** 2 + math.log(sigma) + 0.5 * math.log(2 * math.pi)).sum() * scale
    dwant = scale * (m64 - x) / (sigma + 1e-8) ** 2
    target = frames.cuda() if u8 else x.permute(0, 3, 1, 2).float().contiguous().cuda()
    loss = torch.zeros(1, device="cuda")
    dmu = ops.gauss_ll_image(mu.cuda(), target, C, sigma, scale, loss)
    torch.cuda.synchronize()
    assert abs(float(loss) - float(want)) <= 2e-5 * abs(float(want))
    assert dmu.dtype == dtype and dmu.shape == mu.shape and bool((dmu[..., C:] == 0).all())
    close(dmu[..., :C].cpu().double(), dwant, 1e-5 if dtype == torch.float32 else 2.0 ** -8, "dmu")
    loss2 = torch.zeros(1, device="cuda")
    assert ops.gauss_ll_image(mu.cuda(), target, C, sigma, scale, loss2, want_grad=False) is None
    assert abs(float(loss2) - float(want)) <= 2e-5 * abs(float(want))
