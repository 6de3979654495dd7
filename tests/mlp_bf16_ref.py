"""The bf16 compute mode of the grouped MLP layers (SPEC.md N3l) restated in torch on the CPU, for tests/test_mlp_bf16*.py.

The rule: every tensor is fp32; both operands of every product are rounded to bf16 (round to nearest even) and the products are
summed in fp32; the bias add, ReLU, the mask and db = sum_m dpre (of the UNROUNDED values) are fp32.  Here the rounded operands are
multiplied in fp64 (the reference) or in fp32 (a correct implementation in another summation order).

The per-element bound of the kernel tests: a sum of K_sum products of bf16 operands is exact product by product in fp32 (8 + 8
significand bits), so all error is accumulation: at most (K_sum + 2) additions' worth of unit roundoff 2^-23 (the +2: the bias add
and the store) of the sum of the magnitudes,
    |got - ref| <= (K_sum + 2) 2^-23 (sum |a^ b^| + |bias|),
the worst case of fp32 summation in ANY order with a unit roundoff of 2^-23 -- twice that of round-to-nearest, which also covers a
matrix unit that truncates."""
import itertools

import torch

ROWS, WIDTHS, DEPTHS = (1, 31, 33, 70), (20, 36, 68, 128), (4, 12, 20, 36, 296)
SHAPES = list(itertools.product(ROWS, WIDTHS, DEPTHS))        # (rows, N, K): the tile edges of csrc/ens_tile_bf16.h
GROUPED = ((70, 36), (0, 20), (33, 12))                       # (rows, K) of one launch of three groups, one of them empty
SPLITS = (1, 2, 3)                                            # S of the row-split backward on 70 rows
U = 2.0 ** -23


def round_bf16(t):
    """fp32 -> bf16 (torch's cast rounds to nearest even) -> fp64."""
    return t.float().to(torch.bfloat16).double()


def _round_like(t):
    return t.float().to(torch.bfloat16).to(t.dtype)


def fwd(x, w, bias, dtype=torch.float64):
    """pre [rows][N] of one layer on rounded operands, and the bound's magnitude sum |x^| |w^| + |bias|."""
    xr, wr = round_bf16(x), round_bf16(w)
    return (xr.to(dtype) @ wr.to(dtype).T + bias.to(dtype)).double(), xr.abs() @ wr.abs().T + bias.double().abs()


def wgrad(dpre, x, dtype=torch.float64):
    """dw [N][K] = sum_m dpre^ x^, its magnitude sum, and db [N] = sum_m dpre of the unrounded values."""
    dr, xr = round_bf16(dpre), round_bf16(x)
    return (dr.to(dtype).T @ xr.to(dtype)).double(), dr.abs().T @ xr.abs(), dpre.to(dtype).sum(0).double()


def dgrad(dpre, w, pre_prev=None, dtype=torch.float64):
    """dprev [rows][K] = (sum_n dpre^ w^) [pre_prev > 0] (unmasked without pre_prev), and the magnitude sum of the unmasked sum."""
    dr, wr = round_bf16(dpre), round_bf16(w)
    d = (dr.to(dtype) @ wr.to(dtype)).double()
    if pre_prev is not None:
        d = d * (pre_prev > 0)
    return d, dr.abs() @ wr.abs()


def bound(k_sum, mag):
    return (k_sum + 2) * U * mag


def worst_ratio(got, ref, k_sum, mag):
    """max over elements of |got - ref| / bound; a NaN (or an element of zero bound that differs) counts as outside: inf."""
    got, b = got.detach().cpu().double(), bound(k_sum, mag)
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b)
    ratio = torch.where(torch.isnan(got) | torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return float(ratio.max()) if ratio.numel() else 0.0


class RoundedLinear(torch.autograd.Function):
    """y = x^ w^T + b in the dtype of x; backward dw = dy^T x^, dx = dy^ w^, db = sum dy (unrounded)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return _round_like(x) @ _round_like(w).T + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dr = _round_like(dy)
        return dr @ _round_like(w), dr.T @ _round_like(x), dy.sum(0)


def mlp(layers, x, dtype, wide=lambda n: n > 16):
    """A ReLU MLP (none after the last layer) in `dtype`.  layers: [(w [N][K], b [N])]; a layer of output width n with wide(n) rounds
    its operands as above in forward and backward, the others (the narrow last layers, which keep the fp32 kernels) are plain.
    -> (output, the leaf parameters [(w, b)] whose .grad a backward fills, the leaf input)."""
    x = x.to(dtype).clone().requires_grad_(True)
    leaves, h = [], x
    for li, (w, b) in enumerate(layers):
        w, b = w.to(dtype).clone().requires_grad_(True), b.to(dtype).clone().requires_grad_(True)
        leaves.append((w, b))
        h = RoundedLinear.apply(h, w, b) if wide(w.shape[0]) else h @ w.T + b
        if li < len(layers) - 1:
            h = torch.relu(h)
    return h, leaves, x
