"""What the eight entry points of the fused latent chains (SPEC.md N3h, N3i, N3j, N3k, N3m, N3n) refuse, as tables -- TEST
INFRASTRUCTURE ONLY.  A refusal happens before any launch, so fake addresses serve and no device is needed: `args` makes the argument
tuple of a valid call with one edit applied, `cases` lists (edit, a piece of the message) for an entry, `check` runs them and the
no-ops.  Every case is refused or is a no-op -- none may reach a launch, the addresses are not memory.  A case breaks ONE condition; the
two "only when T > 1" cases break a second, later one on purpose, so that the call is refused by THAT message instead of launching."""
import ctypes

P = 4096                                               # a non-NULL, 16-byte aligned address
POSTERIOR_HEADS = (("z1_posterior_init", 256), ("z2_prior_init", 32), ("z1_posterior", 256), ("z2_prior", 288))
PRIOR_HEADS = (("z1_prior", 256), ("z2_prior", 288))
VIEWS = dict(eps=P, eps_pitch=288, mean=P, mean_pitch=32, std=P, std_pitch=32, z=P, z_pitch=288)
_VIEW_ORDER = "mean mean_pitch std std_pitch z z_pitch"
_CHAIN = "%s %s_pitch %s rb eps eps_pitch mlps " + _VIEW_ORDER + "%s B %s"
_IMAGINE = "z0 z0_pitch eps eps_pitch mlps wc wc_row wb wb_row A policy act act_pitch " + _VIEW_ORDER + " B H"


class Entry:
    """One entry point: the names of its arguments in order (without the stream), the values of a valid call, the heads of its
    `mlps` (name, the chain columns of the first layer), the name of its time argument, and its kind."""

    def __init__(self, order, defaults, heads, time, bf16=False, bwd=False):
        self.order, self.defaults, self.heads, self.time, self.bf16, self.bwd = order.split(), defaults, heads, time, bf16, bwd


def _chain(src, ra, time, heads, bf16=False, state=""):
    d = dict(VIEWS, B=17, rb=P)
    d.update({src: P, src + "_pitch": 256, ra: P, time: 2})
    return Entry(_CHAIN % (src, src, ra, state, time), d, heads, time, bf16)


def _imagine(bf16):
    return Entry(_IMAGINE, dict(VIEWS, z0=P, z0_pitch=288, wc=P, wc_row=8, wb=P, wb_row=8, A=6, act=P, act_pitch=8, B=17, H=2), PRIOR_HEADS,
                 "H", bf16)


ENTRIES = {
    "s2p_posterior_chain_fwd": _chain("feat", "ra", "T", POSTERIOR_HEADS),
    "s2p_posterior_chain_fwd_save": _chain("feat", "ra", "T", POSTERIOR_HEADS, state=" state"),
    "s2p_posterior_chain_bwd": Entry("eps eps_pitch dmean dmean_pitch dstd dstd_pitch dz dz_pitch mlps state grads B T",
                                     dict(eps=P, eps_pitch=288, dmean=P, dmean_pitch=32, dstd=P, dstd_pitch=32, dz=P, dz_pitch=288, B=17, T=2),
                                     POSTERIOR_HEADS[2:], "T", bwd=True),
    "s2p_prior_chain_fwd": _chain("z2_0", "rc", "H", PRIOR_HEADS),
    "s2p_imagine_chain_fwd": _imagine(False),
    "s2p_posterior_chain_fwd_bf16": _chain("feat", "ra", "T", POSTERIOR_HEADS, bf16=True),
    "s2p_prior_chain_fwd_bf16": _chain("z2_0", "rc", "H", PRIOR_HEADS, bf16=True),
    "s2p_imagine_chain_fwd_bf16": _imagine(True),
}


def args(_lib, name, **edit):
    """The arguments of a valid call of `name` (B 17, T or H 2, A 6, W 256) on fake addresses, with `edit` applied: an argument by its
    name (`mlps`, `policy` / `policy_ptr`, `state`, `grads`: the pointer itself), or `mlp=(index, field, value)`,
    `policy=(field, value)`, `state=(field, value)`, `grads=(field, value)` for a field of the host structs."""
    e = ENTRIES[name]
    a = dict(e.defaults)
    if e.bwd:
        mlps = (_lib.ChainMlpBwd * len(e.heads))(*[_lib.ChainMlpBwd(P, P, P, k, 256) for _, k in e.heads])
    else:
        mlp_t = _lib.ChainMlpBf16 if e.bf16 else _lib.ChainMlp
        mlps = (mlp_t * len(e.heads))(*[mlp_t(P, P, P, P, P, P, k, k) for _, k in e.heads])
    a.update(mlps=mlps, policy=(_lib.PolicyMlpBf16 if e.bf16 else _lib.PolicyMlp)(P, P, P, P, P, P, 288, 256),
             state=_lib.ChainState(*[P] * 13), grads=_lib.ChainGrads(*[P] * 7))
    for k, v in edit.items():
        if k == "mlp":
            setattr(mlps[v[0]], v[1], v[2])
        elif k in ("policy", "state", "grads") and isinstance(v, tuple):
            setattr(a[k], v[0], v[1])
        elif k == "policy_ptr":
            a["policy"] = v
        else:
            assert k in a, k
            a[k] = v
    return tuple(a[n] for n in e.order) + (None,)


def _mlp_cases(e):
    """Per head of the entry's `mlps`: a null operand, a wrong k1, a first-layer row that is too short resp. no whole 16 bytes, and a
    misaligned weight.  The row multiple is 4 floats, in bf16 compute 8 bf16 elements: K + 4 is a row only the fp32 entries take."""
    out = []
    for g, (head, k) in enumerate(e.heads):
        if e.bwd:
            fields, weights, row, least, text = ("w1t", "w2t", "w3t"), ("w1t", "w2t", "w3t"), "w1t_row", 256, "a multiple of 4 floats and at least 256"
        else:
            fields, weights, row, least = ("w1", "b1", "w2", "b2", "w3", "b3"), ("w1", "w2", "w3"), "w1_row", k
            text = "a multiple of %s and at least K" % ("8 bf16 elements" if e.bf16 else "4 floats")
        out += [(dict(mlp=(g, fields[g % len(fields)], None)), head + ": null operand"),
                (dict(mlp=(g, fields[(g + 1 + len(fields) // 2) % len(fields)], None)), head + ": null operand"),
                (dict(mlp=(g, "k1", k // 2)), "%s: the first layer's K is %d, %d is built" % (head, k // 2, k)),
                (dict(mlp=(g, row, least - 8)), "%s: %s must be %s" % (head, row, text)),
                (dict(mlp=(g, row, least + (4 if e.bf16 else 2))), "%s: %s must be %s" % (head, row, text)),
                (dict(mlp=(g, weights[g % 3], P + 8)), head + ": the weights must be 16-byte aligned"),
                (dict(mlp=(g, weights[(g + 1) % 3], P + (2 if e.bf16 else 4))), head + ": the weights must be 16-byte aligned")]
    return out


def _view_cases(names="eps mean std z", rows="(eps 288, mean 32, std 32, z 288)"):
    names = names.split()
    return ([(({n: None}), "null pointer (%s and %s are required)" % (", ".join(names[:-1]), names[-1])) for n in names] +
            [({n + "_pitch": VIEWS.get(n + "_pitch", 288 if n == "dz" else 32) - 1}, "a pitch is below its row " + rows) for n in names])


def _chain_cases(name, e):
    src, ra = e.order[0], e.order[2]
    need = "(feat and mlps are required)" if src == "feat" else "(z2_0, rc, rb and mlps are required)"
    out = [({src: None}, "null pointer " + need), (dict(mlps=None), "null pointer " + need),
           ({src + "_pitch": 255}, "the pitch of %s is below its row of 256" % src),
           ({src + "_pitch": 258}, "%s must be 16-byte aligned, its pitch a multiple of 4 floats" % src),
           ({src: P + 4}, "%s must be 16-byte aligned, its pitch a multiple of 4 floats" % src)]
    if src == "feat":                                  # ra / rb: required when T > 1 only -- at T = 1 the call gets as far as `z`
        out += [(dict(ra=None), "ra and rb are required when T > 1"), (dict(rb=None), "ra and rb are required when T > 1"),
                (dict(T=1, ra=None, rb=None, z=None), "null pointer (eps, mean, std and z are required)")]
    else:
        out += [(dict(rc=None), "null pointer " + need), (dict(rb=None), "null pointer " + need)]
    if "state" in e.order:                             # the chain's buffers are required when T > 1 only, and so are the heads 2 and 3
        out += [(dict(state=None), "null pointer (state is required)"),
                (dict(state=("a0_h1", None)), "state: a buffer is NULL or not 16-byte aligned"),
                (dict(state=("b0_raw", P + 4)), "state: a buffer is NULL or not 16-byte aligned"),
                (dict(state=("h1a", None)), "state: a buffer is NULL or not 16-byte aligned"),
                (dict(state=("xz", P + 8)), "state: a buffer is NULL or not 16-byte aligned"),
                (dict(T=1, ra=None, rb=None, mlp=(3, "w1", None), state=("b0_h2", None)), "state: a buffer is NULL or not 16-byte aligned")]
    return out + _view_cases()


def _bwd_cases(name, e):
    need = "null pointer (eps, dmean, dstd, dz, mlps, state and grads are required)"
    out = [({n: None}, need) for n in ("mlps", "state", "grads")]
    out += [(c, need if "null pointer" in t else t) for c, t in _view_cases("eps dmean dstd dz", "(eps 288, dz 288, dmean 32, dstd 32)")]
    for f in ("h1a", "rawb"):
        out += [(dict(state=(f, None)), "state: a chain buffer is NULL or not 16-byte aligned"),
                (dict(state=(f, P + 4)), "state: a chain buffer is NULL or not 16-byte aligned")]
    for f in ("drawa", "dxz"):
        out += [(dict(grads=(f, None)), "grads: a buffer is NULL or not 16-byte aligned"),
                (dict(grads=(f, P + 8)), "grads: a buffer is NULL or not 16-byte aligned")]
    return out


def _imagine_cases(name, e):
    odd = 288 + (4 if e.bf16 else 2)                   # a row of whole floats that is no whole 16 bytes of this mode's elements
    return [
        (dict(z0=None), "null pointer"), (dict(wc=None), "null pointer"), (dict(wb=None), "null pointer"), (dict(act=None), "null pointer"),
        (dict(mlps=None), "null pointer"), (dict(policy_ptr=None), "null pointer"),
        (dict(eps=None), "null pointer"), (dict(mean=None), "null pointer"), (dict(std=None), "null pointer"), (dict(z=None), "null pointer"),
        (dict(mlp=(0, "w2", None)), "z1_prior: null operand"), (dict(policy=("b2", None)), "policy: null operand"),
        (dict(mlp=(0, "k1", 288)), "z1_prior: the first layer's K is 288, 256 is built"),
        (dict(mlp=(1, "k1", 256)), "z2_prior: the first layer's K is 256, 288 is built"),
        (dict(policy=("width", 192)), "hidden width 192"), (dict(policy=("width", 64)), "hidden width 64"),
        (dict(policy=("width", 1152)), "hidden width 1152"), (dict(A=0), "action width 0"), (dict(A=9), "action width 9"),
        (dict(z0_pitch=287), "a pitch is below its row (z0 288, act A)"), (dict(act_pitch=5), "a pitch is below its row (z0 288, act A)"),
        (dict(eps_pitch=287), "a pitch is below its row"), (dict(mean_pitch=31), "a pitch is below its row"),
        (dict(std_pitch=31), "a pitch is below its row"), (dict(z_pitch=287), "a pitch is below its row"),
        (dict(z0_pitch=290), "z0 must be 16-byte aligned, its pitch a multiple of 4 floats"),
        (dict(z0=P + 4), "z0 must be 16-byte aligned"),
        (dict(wc_row=4), "wc_row and wb_row"), (dict(wb_row=10), "wc_row and wb_row"),
        (dict(wc=P + 8), "wc and wb must be 16-byte aligned"), (dict(wb=P + 4), "wc and wb must be 16-byte aligned"),
        (dict(mlp=(1, "w1_row", 280)), "z2_prior: w1_row"), (dict(mlp=(1, "w1_row", odd)), "z2_prior: w1_row"),
        (dict(mlp=(0, "w3", P + 2)), "z1_prior: the weights must be 16-byte aligned"),
        (dict(policy=("w1_row", 280)), "policy: w1_row"), (dict(policy=("w1_row", odd)), "policy: w1_row"),
        (dict(policy=("w1", P + 2)), "policy: the weights must be 16-byte aligned"),
        (dict(policy=("w3", P + 8)), "policy: the weights must be 16-byte aligned"),
        (dict(policy=("w1_row", odd)), "policy: w1_row must be a multiple of %s and at least K" % ("8 bf16 elements" if e.bf16 else "4 floats")),
        (dict(policy=("w1", None)), "policy: null operand"), (dict(policy=("b3", None)), "policy: null operand"),
    ]


def cases(name):
    """(the edit, a piece of the message) for every refusal of `name` that the tables pin."""
    e = ENTRIES[name]
    own = _bwd_cases if e.bwd else _imagine_cases if "policy" in e.order else _chain_cases
    return [(dict(B=-1), "negative size"), ({e.time: -1}, "negative size")] + own(name, e) + _mlp_cases(e)


def check(_lib, name):
    """Every case of `cases(name)` returns a negative value with its message, and the no-ops -- B = 0, T = 0 and for the backward
    T = 1 -- return 0 looking at no pointer.  -> the number of cases."""
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
