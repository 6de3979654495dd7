"""GPU: the spectral-norm kernels (csrc/spectral.hip, s2p_pack_weights_scaled) against float64 -- one power iteration
(training and eval variants), the W / sigma pack and the projection of the gradient (SPEC.md D5s)."""
import ctypes

import pytest
import torch

from s2p_amd import _lib
from s2p_amd.ops import pad_to

pytestmark = pytest.mark.gpu

EPS = 1e-12
# (R, T, C): every production shape (G ResBlk conv 256 x 9*256; D 128 x 16*64, 256 x 16*128, 512 x 16*256) and ragged ones
# whose column count K = T*C is not a multiple of 4 or 64
SHAPES = [(256, 9, 256), (128, 16, 64), (256, 16, 128), (512, 16, 256)] + \
         [(r, t, c) for r in (1, 3, 70) for (t, c) in ((9, 3), (16, 6), (4, 25))]


def _table(items, ctype, dev):
    arr = (ctype * len(items))(*items)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)


def _normalize(x):
    return x / max(float(x.norm()), EPS)


class Jobs:
    """Device tensors + job table of a set of (R, T, C) SN weights."""

    def __init__(self, shapes, dev, seed=0, grad_pad=0):
        g = torch.Generator().manual_seed(seed)
        self.shapes = shapes
        self.w, self.u, self.v, self.sig, self.ws, self.grad = [], [], [], [], [], []
        L = _lib.lib()
        sizes = [r * t * c for r, t, c in shapes]
        # gradients of all jobs inside one flat buffer with `grad_pad` untouched floats around each
        self.flat = torch.randn(sum(sizes) + grad_pad * (len(shapes) + 1), generator=g).to(dev)
        off = grad_pad
        for (r, t, c), n in zip(shapes, sizes):
            k = t * c
            self.w.append((torch.randn(r, t, c, generator=g) / k ** 0.5).to(dev))
            self.u.append(_normalize(torch.randn(r, generator=g)).to(dev))
            self.v.append(_normalize(torch.randn(k, generator=g)).to(dev))
            self.sig.append(torch.zeros(1, device=dev))
            self.ws.append(torch.full((L.s2p_sn_workspace_floats(r, k),), float("nan"), device=dev))
            self.grad.append(self.flat[off:off + n])
            off += n + grad_pad
        self.jobs = [_lib.SnJob(w.data_ptr(), u.data_ptr(), v.data_ptr(), s.data_ptr(), ws.data_ptr(), gr.data_ptr(), r, t * c)
                     for (r, t, c), w, u, v, s, ws, gr in zip(shapes, self.w, self.u, self.v, self.sig, self.ws, self.grad)]
        self.dev_table = _table(self.jobs, _lib.SnJob, dev)
        self.max_R = max(r for r, _, _ in shapes)
        self.max_K = max(t * c for _, t, c in shapes)

    def power_iter(self, training):
        _lib.check(_lib.lib().s2p_sn_power_iter(self.dev_table.data_ptr(), len(self.jobs), self.max_R, self.max_K,
                                                1 if training else 0, _lib.stream()), "s2p_sn_power_iter")
        torch.cuda.synchronize()

    def project(self):
        _lib.check(_lib.lib().s2p_sn_project_grad(self.dev_table.data_ptr(), len(self.jobs), self.max_R, self.max_K,
                                                  _lib.stream()), "s2p_sn_project_grad")
        torch.cuda.synchronize()

    def state(self, i):
        return self.u[i].clone(), self.v[i].clone(), self.sig[i].clone()


def _ref_power_iter(W, u, v, training):
    W, u, v = W.double().cpu().reshape(W.shape[0], -1), u.double().cpu(), v.double().cpu()
    if training:
        v = _normalize(W.t() @ u)
        u = _normalize(W @ v)
    return u, v, float(u @ (W @ v))


def test_power_iteration_matches_float64_training_and_eval(hip_device):
    J = Jobs(SHAPES, hip_device, seed=1)
    before = [J.state(i) for i in range(len(SHAPES))]
    J.power_iter(True)
    for i, (r, t, c) in enumerate(SHAPES):
        u, v, s = _ref_power_iter(J.w[i], before[i][0], before[i][1], True)
        assert (J.u[i].double().cpu() - u).abs().max() <= 1e-5, (r, t, c)
        assert (J.v[i].double().cpu() - v).abs().max() <= 1e-5, (r, t, c)
        assert abs(float(J.sig[i]) - s) <= 1e-5 * abs(s), (r, t, c, float(J.sig[i]), s)
    # eval: sigma from the stored u, v, which stay bitwise as they are
    after = [J.state(i) for i in range(len(SHAPES))]
    J.power_iter(False)
    for i, (r, t, c) in enumerate(SHAPES):
        assert torch.equal(J.u[i], after[i][0]) and torch.equal(J.v[i], after[i][1])
        _, _, s = _ref_power_iter(J.w[i], after[i][0], after[i][1], False)
        assert abs(float(J.sig[i]) - s) <= 1e-5 * abs(s), (r, t, c)


def test_power_iteration_is_deterministic_and_job_independent(hip_device):
    A = Jobs(SHAPES, hip_device, seed=2)
    B = Jobs(SHAPES, hip_device, seed=2)
    A.power_iter(True)
    B.power_iter(True)
    for i in range(len(SHAPES)):
        for x, y in zip(A.state(i), B.state(i)):
            assert torch.equal(x, y)
    # each job alone in its own launch: bitwise what it got in the full table
    for i, shp in enumerate(SHAPES):
        C = Jobs(SHAPES, hip_device, seed=2)                 # the inputs of the iteration above
        one = Jobs([shp], hip_device, seed=0)
        one.w[0].copy_(C.w[i]); one.u[0].copy_(C.u[i]); one.v[0].copy_(C.v[i])
        one.power_iter(True)
        for x, y in zip(one.state(0), A.state(i)):
            assert torch.equal(x, y), shp


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_scaled_pack_is_w_over_sigma_and_null_is_unscaled(hip_device, dtype):
    J = Jobs(SHAPES, hip_device, seed=3)
    J.power_iter(True)
    ce = _lib.chunk_elems(dtype)
    jobs, sig_ptrs, outs = [], [], []
    for i, (r, t, c) in enumerate(SHAPES):
        for scaled in (True, False):
            cp, rp = pad_to(c, ce), pad_to(r, ce)
            fwd = torch.zeros((r, t, cp), dtype=dtype, device=hip_device)
            bwd = torch.zeros((cp, t, rp), dtype=dtype, device=hip_device)
            jobs.append(_lib.PackJob(J.w[i].data_ptr(), fwd.data_ptr(), bwd.data_ptr(), r, t, c, cp, rp, 0, _lib.dtype_id(dtype)))
            sig_ptrs.append(J.sig[i].data_ptr() if scaled else 0)
            outs.append((i, scaled, fwd, bwd))
    max_elems = max(r * t * c for r, t, c in SHAPES)
    jobs_dev, sig_dev = _table(jobs, _lib.PackJob, hip_device), _table(sig_ptrs, ctypes.c_void_p, hip_device)
    _lib.check(_lib.lib().s2p_pack_weights_scaled(jobs_dev.data_ptr(), sig_dev.data_ptr(), len(jobs), max_elems, _lib.stream()),
               "s2p_pack_weights_scaled")
    # the plain pack of the unscaled jobs, for comparison
    plain, plain_out = [], {}
    for (i, scaled, fwd, bwd), j in zip(outs, jobs):
        if not scaled:
            f2, b2 = torch.zeros_like(fwd), torch.zeros_like(bwd)
            plain.append(_lib.PackJob(j.src, f2.data_ptr(), b2.data_ptr(), j.R, j.T, j.C, j.Cpad, j.Rrow, 0, j.dtype))
            plain_out[i] = (f2, b2)
    plain_dev = _table(plain, _lib.PackJob, hip_device)          # (the device tables stay referenced until the launches ran)
    _lib.check(_lib.lib().s2p_pack_weights(plain_dev.data_ptr(), len(plain), max_elems, _lib.stream()), "s2p_pack_weights")
    torch.cuda.synchronize()
    del jobs_dev, sig_dev, plain_dev
    for i, scaled, fwd, bwd in outs:
        r, t, c = SHAPES[i]
        W = J.w[i].cpu()
        ref = (W / J.sig[i].cpu() if scaled else W).to(dtype)          # fp32 division, then the RNE cast
        f, b = fwd.cpu(), bwd.cpu()
        assert torch.equal(f[:, :, :c], ref), (SHAPES[i], scaled)
        assert not f[:, :, c:].float().any()
        assert torch.equal(b[:c, :, :r], ref.permute(2, 1, 0)), (SHAPES[i], scaled)
        if not scaled:
            f2, b2 = plain_out[i]
            assert torch.equal(f, f2.cpu()) and torch.equal(b, b2.cpu())


def test_projection_matches_float64_autograd_and_leaves_the_rest(hip_device):
    J = Jobs(SHAPES, hip_device, seed=4, grad_pad=37)
    J.power_iter(True)
    flat0 = J.flat.clone()
    G0 = [g.clone() for g in J.grad]
    J.project()
    for i, (r, t, c) in enumerate(SHAPES):
        W = J.w[i].double().cpu().reshape(r, -1).requires_grad_(True)
        u, v = J.u[i].double().cpu(), J.v[i].double().cpu()
        sigma = u @ (W @ v)
        (G0[i].double().cpu().reshape(r, -1) * (W / sigma)).sum().backward()
        ref = W.grad
        got = J.grad[i].double().cpu().reshape(r, -1)
        err = float((got - ref).norm() / ref.norm())
        assert err <= 1e-5, ((r, t, c), err)
    mask = torch.ones_like(J.flat, dtype=torch.bool)
    for g in J.grad:
        off = (g.data_ptr() - J.flat.data_ptr()) // 4
        mask[off:off + g.numel()] = False
    assert torch.equal(J.flat[mask], flat0[mask])
