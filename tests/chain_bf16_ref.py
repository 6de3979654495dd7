"""The rounding rule of the bf16-compute latent chains (SPEC.md N3m) restated in torch on the CPU -- TEST INFRASTRUCTURE ONLY.

Per layer: both operands rounded to bf16 (nearest even), the products summed in `dtype` (fp64: the reference; fp32: what a kernel can
do), (acc + add) + bias or acc + bias, LeakyReLU 0.2, the head.  The feature / action columns of the first layers are the hoisted
terms `add`: unrounded products, computed here in `dtype` or GIVEN (the fp32 tensors a kernel was handed).  `gen` permutes each
layer's summation index ("another summation order").  Free-running, a chain feeds on its own samples; teacher-forced (`z_given`), each
of its 2 T MLP evaluations reads the given fp32 z instead, so one evaluation's rounding flips do not travel down the chain."""
import torch
import torch.nn.functional as F

import slac_latent_ref as R

Z1, Z2, Z, FEAT, HID = 32, 256, 288, 256, 256


def bf(x):
    """x rounded to bf16 (nearest even), in x's dtype."""
    return x.float().to(torch.bfloat16).to(x.dtype)


def _dot(x, w, dtype, gen):
    """sum_k bf16(x)[.., k] bf16(w)[n, k] in `dtype`, over a permuted k when `gen` is given."""
    x, w = bf(x.to(dtype)), bf(w.to(dtype))
    if gen is not None:
        perm = torch.randperm(x.shape[-1], generator=gen)
        x, w = x[..., perm].contiguous(), w[:, perm].contiguous()
    return x @ w.t()


def mlp(p, name, cols, x, add, eps, dtype, gen=None):
    """One Gaussian MLP under the rule: x the chain input (fp32 values), cols the chain columns of its first layer, add the hoisted
    term or None, eps the noise -> (mean, std, z) in `dtype`."""
    w = lambda i: p["%s.net.%d.weight" % (name, i)]
    b = lambda i: p["%s.net.%d.bias" % (name, i)].to(dtype)
    acc = _dot(x, w(0)[:, cols], dtype, gen)
    h = F.leaky_relu((acc + add.to(dtype)) + b(0) if add is not None else acc + b(0), 0.2)
    h = F.leaky_relu(_dot(h, w(2), dtype, gen) + b(2), 0.2)
    mean, raw = torch.chunk(_dot(h, w(4), dtype, gen) + b(4), 2, dim=-1)
    std = F.softplus(raw) + 1e-5
    return mean, std, mean + eps.to(dtype) * std


def hoisted_posterior(p, feat, action, dtype):
    """(ra, rb) [T-1, B, 256]: [feat(t) | a(t-1)] on z1_posterior's feature and action columns, a(t-1) on z2_prior's action columns."""
    wa, wb = p["z1_posterior.net.0.weight"].to(dtype), p["z2_prior.net.0.weight"].to(dtype)
    f, a = feat[:, 1:].transpose(0, 1).to(dtype), action.transpose(0, 1).to(dtype)
    return torch.cat([f, a], -1) @ torch.cat([wa[:, :FEAT], wa[:, FEAT + Z2:]], 1).t(), a @ wb[:, Z:].t()


def hoisted_prior(p, action, dtype):
    """(rc, rb) [H, B, 256]: a(h-1) on the action columns of z1_prior and of z2_prior."""
    a = action.transpose(0, 1).to(dtype)
    return a @ p["z1_prior.net.0.weight"].to(dtype)[:, Z2:].t(), a @ p["z2_prior.net.0.weight"].to(dtype)[:, Z:].t()


def _steps(p, heads, z2, adds, noise, first, dtype, gen, z_given):
    """The steps of a chain from z2 (fp32 values or `dtype`): per step the z1 MLP on z2(t-1), the z2 MLP on z1(t) | z2(t-1).  Slot s of
    noise / z_given is `first + s`.  -> lists of mean, std, z1, z2."""
    out = [[], [], [], []]
    for s in range(adds[0].shape[0]):
        t = first + s
        if z_given is not None and t > 0:
            z2 = z_given[:, t - 1, Z1:]
        m, sd, z1 = mlp(p, heads[0], slice(FEAT, FEAT + Z2) if heads[0] == "z1_posterior" else slice(0, Z2), z2, adds[0][s], noise[:, t, :Z1],
                        dtype, gen)
        x1 = z_given[:, t, :Z1] if z_given is not None else z1
        z2n = mlp(p, heads[1], slice(0, Z), torch.cat([x1.to(dtype), z2.to(dtype)], -1), adds[1][s], noise[:, t, Z1:], dtype, gen)[2]
        for o, v in zip(out, (m, sd, z1, z2n)):
            o.append(v)
        z2 = z2n
    return out


def posterior(p, feat, action, noise, dtype, gen=None, ra=None, rb=None, z_given=None):
    """sample_posterior under the rule -> (mean, std [B,T,32], z [B,T,288]) in `dtype`.  ra, rb: the hoisted terms [T-1, B, 256] a
    kernel was given (None: computed in `dtype`); z_given [B,T,288]: teacher forcing."""
    T = feat.shape[1]
    m, sd, z1 = mlp(p, "z1_posterior_init", slice(0, FEAT), feat[:, 0], None, noise[:, 0, :Z1], dtype, gen)
    x1 = z_given[:, 0, :Z1] if z_given is not None else z1
    z2 = mlp(p, "z2_prior_init", slice(0, Z1), x1, None, noise[:, 0, Z1:], dtype, gen)[2]
    out = [[m], [sd], [z1], [z2]]
    if T > 1:
        if ra is None:
            ra, rb = hoisted_posterior(p, feat, action, dtype)
        z2_0 = z_given[:, 0, Z1:] if z_given is not None else z2
        for o, more in zip(out, _steps(p, ("z1_posterior", "z2_prior"), z2_0, (ra, rb), noise, 1, dtype, gen, z_given)):
            o += more
    mean, std, z1, z2 = (torch.stack(o, 1) for o in out)
    return mean, std, torch.cat([z1, z2], -1)


def prior(p, z0, action, noise, dtype, gen=None, rc=None, rb=None, z_given=None):
    """predict under the rule: z0 [B,288], action [B,H,A], noise [B,H,288] -> (mean, std [B,H,32], z [B,H,288]); slot h - 1 is step h.
    z_given [B,H,288]: teacher forcing (step h reads the given z2(h-1), z2(0) from z0, and the given z1(h))."""
    if rc is None:
        rc, rb = hoisted_prior(p, action, dtype)
    zg = None if z_given is None else torch.cat([z0[:, None], z_given], 1)          # slot t = step t
    ns = torch.cat([noise[:, :1] * 0, noise], 1)
    mean, std, z1, z2 = (torch.stack(o, 1) for o in _steps(p, ("z1_prior", "z2_prior"), z0[:, Z1:], (rc, rb), ns, 1, dtype, gen, zg))
    return mean, std, torch.cat([z1, z2], -1)


def evaluations(mean, std, z):
    """The 2 T MLP evaluations of a call as rows: [T, B, 96] = mean | std | z1 of the z1 MLPs and [T, B, 256] = z2 of the z2 MLPs."""
    return torch.cat([mean, std, z[..., :Z1]], -1).transpose(0, 1), z[..., Z1:].transpose(0, 1)


def row_deviation(got, ref):
    """Per (row, MLP evaluation): max |got - ref| relative to the evaluation's maximum |ref| -> a flat fp64 tensor of 2 T B values."""
    out = []
    for g, r in zip(evaluations(*[t.double().cpu() for t in got]), evaluations(*[t.double().cpu() for t in ref])):
        out.append(((g - r).abs().amax(-1) / r.abs().amax((-1, -2), keepdim=True).squeeze(-1)).flatten())
    return torch.cat(out)


def exact_params(a):
    """R.make_params(a) with the heads replaced by data on which every fp32 sum of the chain is exact in any order: weights in {0, 1/4},
    two non-zeros per row in every column segment of every layer (the chain columns, the feature columns and the action columns of a
    first layer each), biases in {1/4, 1/2, 3/4, 1}."""
    g = torch.Generator().manual_seed(4242)
    p = R.make_params(a)
    segs = {"z2_prior_init": [Z1], "z1_prior": [Z2, a], "z2_prior": [Z, a], "z1_posterior_init": [FEAT], "z1_posterior": [FEAT, Z2, a],
            "reward": [2 * Z + a]}
    for name, (din, dout) in R.head_dims(a).items():
        for i, (ws, co) in zip((0, 2, 4), ((segs[name], HID), ([HID], HID), ([HID], 2 * dout))):
            parts = []
            for wd in ws:
                w = torch.zeros(co, wd)
                for n in range(co):
                    w[n, torch.randperm(wd, generator=g)[:2]] = 0.25
                parts.append(w)
            p["%s.net.%d.weight" % (name, i)] = torch.cat(parts, 1)
            p["%s.net.%d.bias" % (name, i)] = torch.randint(1, 5, (co,), generator=g).float() / 4
        assert p[name + ".net.0.weight"].shape[1] == din
    return p


def exact_inputs(B, T, a, seed=0):
    """feat multiples of 2^-8 in [0, 2), actions multiples of 1/4 in [0, 2), eps = 0; row b is the same whatever B is."""
    g = torch.Generator().manual_seed(77 + 1000 * seed + 100 * T + a)
    feat = torch.randint(0, 512, (33, T, FEAT), generator=g).float() / 256
    action = torch.randint(0, 8, (33, max(T - 1, 0), a), generator=g).float() / 4
    return feat[:B], action[:B], torch.zeros(B, T, Z)


def random_inputs(B, T, a, seed=0):
    """The inputs of tests/test_posterior_chain_gpu.py::_inputs, on the CPU."""
    g = torch.Generator().manual_seed(1000 * seed + 100 * T + a)
    feat, action, noise = torch.randn(33, T, FEAT, generator=g), torch.randn(33, T - 1, a, generator=g), torch.randn(33, T, Z, generator=g)
    return feat[:B], action[:B], noise[:B]
