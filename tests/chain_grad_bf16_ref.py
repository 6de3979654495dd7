"""The rounding rule of the bf16-compute posterior chain UNDER GRAD (SPEC.md N3p) restated in torch on the CPU, and the refusal
tables of its three entry points -- TEST INFRASTRUCTURE ONLY.

A layer of the chain is a custom autograd function: FORWARD both operands rounded to bf16 (tests/chain_bf16_ref.py's _dot: the rule of
N3m, unchanged), INPUT GRADIENT both operands rounded -- bf16(g) . bf16(w), g the gradient at the layer's sum, i.e. draw for a last
layer and dh . act'(h) for the others -- WEIGHT GRADIENT on the unrounded g and the unrounded input: the straight-through gradient
with respect to the fp32 masters.  Everything else (the epilogues, LeakyReLU, the head, the hoisted feature / action terms and their
gradients) is ordinary autograd in `dtype`.  `gen` permutes every layer's summation index, forward and backward."""
import torch
import torch.nn.functional as F

import chain_bf16_ref as C
import chain_refusals as CR

Z1, Z2, Z, FEAT, HID = C.Z1, C.Z2, C.Z, C.FEAT, C.HID
CHAIN_HEADS = ("z1_posterior_init", "z2_prior_init", "z1_posterior", "z2_prior")
P = CR.P


class _Layer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, gen):
        ctx.save_for_backward(x, w)
        ctx.gen = gen
        return C._dot(x, w, x.dtype, gen)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gh, wh = C.bf(g), C.bf(w)
        if ctx.gen is not None:
            perm = torch.randperm(g.shape[-1], generator=ctx.gen)
            gh, wh = gh[..., perm].contiguous(), wh[perm].contiguous()
        return gh @ wh, g.reshape(-1, g.shape[-1]).t() @ x.reshape(-1, x.shape[-1]), None


def mlp(p, name, cols, x, add, eps, dtype, gen=None):
    """chain_bf16_ref.mlp with every layer a _Layer: the same values, and gradients under the rule."""
    w = lambda i: p["%s.net.%d.weight" % (name, i)].to(dtype)
    b = lambda i: p["%s.net.%d.bias" % (name, i)].to(dtype)
    acc = _Layer.apply(x.to(dtype), w(0)[:, cols], gen)
    h = F.leaky_relu((acc + add.to(dtype)) + b(0) if add is not None else acc + b(0), 0.2)
    h = F.leaky_relu(_Layer.apply(h, w(2), gen) + b(2), 0.2)
    mean, raw = torch.chunk(_Layer.apply(h, w(4), gen) + b(4), 2, dim=-1)
    std = F.softplus(raw) + 1e-5
    return mean, std, mean + eps.to(dtype) * std


def posterior(p, feat, action, noise, dtype, gen=None):
    """sample_posterior under the rule, free-running -> (mean, std [B,T,32], z [B,T,288]) in `dtype`, differentiable in feat, action
    and every tensor of p that requires grad."""
    T = feat.shape[1]
    m, sd, z1 = mlp(p, "z1_posterior_init", slice(0, FEAT), feat[:, 0], None, noise[:, 0, :Z1], dtype, gen)
    z2 = mlp(p, "z2_prior_init", slice(0, Z1), z1, None, noise[:, 0, Z1:], dtype, gen)[2]
    out = [[m], [sd], [z1], [z2]]
    if T > 1:
        ra, rb = C.hoisted_posterior(p, feat, action, dtype)
        for t in range(1, T):
            m, sd, z1 = mlp(p, "z1_posterior", slice(FEAT, FEAT + Z2), z2, ra[t - 1], noise[:, t, :Z1], dtype, gen)
            z2 = mlp(p, "z2_prior", slice(0, Z), torch.cat([z1, z2], -1), rb[t - 1], noise[:, t, Z1:], dtype, gen)[2]
            for o, v in zip(out, (m, sd, z1, z2)):
                o.append(v)
    mean, std, z1, z2 = (torch.stack(o, 1) for o in out)
    return mean, std, torch.cat([z1, z2], -1)


def param_keys():
    return ["%s.net.%d.%s" % (h, i, k) for h in CHAIN_HEADS for i in (0, 2, 4) for k in ("weight", "bias")]


def loss_weights(B, T, seed):
    """The fixed random weighting of mean, std, z that makes the end-to-end loss."""
    g = torch.Generator().manual_seed(31 + seed)
    return [torch.randn(B, T, c, generator=g) for c in (Z1, Z1, Z)]


def gradients(p, feat, action, noise, weights, dtype, gen=None):
    """The gradients of sum(w . (mean, std, z)) under the rule -> {"dfeat", "daction", the 24 parameter keys: tensor in `dtype`}."""
    q = dict(p)
    keys = param_keys()
    for k in keys:
        q[k] = p[k].detach().clone().requires_grad_(True)
    feat, action = feat.detach().clone().requires_grad_(True), action.detach().clone().requires_grad_(True)
    outs = posterior(q, feat, action, noise, dtype, gen)
    loss = sum((o * w.to(dtype)).sum() for o, w in zip(outs, weights))
    grads = torch.autograd.grad(loss, [feat, action] + [q[k] for k in keys])
    return dict(zip(["dfeat", "daction"] + keys, grads))


def deviation(got, ref):
    """max |got - ref| / max |ref| per gradient -> {name: float}; ref in fp64."""
    return {k: float((got[k].double().cpu() - ref[k].double()).abs().max() / ref[k].double().abs().max()) for k in ref}


# ---- the refusal tables of the three entry points, in the style of tests/chain_refusals.py ----------------------------------------------
FWD, BWD, PACK = "s2p_posterior_chain_fwd_save_bf16", "s2p_posterior_chain_bwd_bf16", "s2p_chain_pack_bf16"
ENTRIES = {
    FWD: CR._chain("feat", "ra", "T", CR.POSTERIOR_HEADS, bf16=True, state=" state"),
    BWD: CR.Entry(" ".join(CR.ENTRIES["s2p_posterior_chain_bwd"].order), dict(CR.ENTRIES["s2p_posterior_chain_bwd"].defaults),
                  CR.POSTERIOR_HEADS[2:], "T", bf16=True, bwd=True),
}


def args(_lib, name, **edit):
    """chain_refusals.args for the two chain entries of N3p (the backward's mlps are ChainMlpBwdBf16)."""
    e = ENTRIES[name]
    a = dict(e.defaults)
    if e.bwd:
        mlps = (_lib.ChainMlpBwdBf16 * 2)(*[_lib.ChainMlpBwdBf16(P, P, P, k, 256) for _, k in e.heads])
    else:
        mlps = (_lib.ChainMlpBf16 * 4)(*[_lib.ChainMlpBf16(P, P, P, P, P, P, k, k) for _, k in e.heads])
    a.update(mlps=mlps, state=_lib.ChainState(*[P] * 13), grads=_lib.ChainGrads(*[P] * 7))
    for k, v in edit.items():
        if k == "mlp":
            setattr(mlps[v[0]], v[1], v[2])
        elif k in ("state", "grads") and isinstance(v, tuple):
            setattr(a[k], v[0], v[1])
        else:
            assert k in a, k
            a[k] = v
    return tuple(a[n] for n in e.order) + (None,)


def cases(name):
    """(the edit, a piece of the message): the fp32 entry's table, with the row multiple of bf16 elements in the mlps' cases."""
    e = ENTRIES[name]
    own = CR._bwd_cases(name, e) if e.bwd else CR._chain_cases(name, e)
    mlp = CR._mlp_cases(e)
    if e.bwd:                                          # _mlp_cases words the backward's row rule for fp32 rows
        mlp = [(c, t.replace("4 floats", "8 bf16 elements")) for c, t in mlp]
    return [(dict(B=-1), "negative size"), ({e.time: -1}, "negative size")] + own + mlp


def check(_lib, name):
    """chain_refusals.check for an entry of ENTRIES -> the number of cases."""
    import ctypes
    L, e = _lib.lib(), ENTRIES[name]
    fn, table = getattr(L, name), cases(name)
    for edit, text in table:
        rc = fn(*args(_lib, name, **edit))
        msg = L.s2p_last_error().decode()
        assert rc < 0 and name + ":" in msg and text in msg, (name, edit, rc, msg)
    sig = _lib.SIGNATURES[name]
    assert len(sig) == len(e.order) + 1, name
    iB, iT = e.order.index("B"), e.order.index(e.time)
    for B, T in ((0, 5), (5, 0)) + (((5, 1),) if e.bwd else ()):
        nothing = [0 if t is ctypes.c_int else None for t in sig]
        nothing[iB], nothing[iT] = B, T
        assert fn(*nothing) == 0, (name, B, T)
    return len(table)


def pack_job(_lib, **edit):
    d = dict(src=P, dst=P, dst_t=P, rows=256, cols=288, src_pitch=296, dst_pitch=288, dst_t_pitch=256)
    d.update(edit)
    return _lib.Bf16PackJob(**d)


PACK_CASES = [(dict(rows=-1), "negative size"), (dict(cols=-1), "negative size"), (dict(src=None), "null pointer"),
              (dict(dst=None, dst_t=None), "null pointer"), (dict(src_pitch=287), "a pitch is below its row"),
              (dict(dst_pitch=280), "a pitch is below its row"), (dict(dst_t_pitch=255), "a pitch is below its row")]
