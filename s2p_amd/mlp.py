"""The grouped ReLU-MLP layers of csrc/mlp.hip from the Python side: the layout of a network's layers inside a flat buffer (`Packed`),
a network's view for the grouped launches (`Net`), and ONE pair of table builders for every consumer (the IQL and CQL trainers, the
policy's `act`).  A builder works in two steps.  `fwd_plan` / `bwd_plan` describe the launches -- which layer of which network is a
group of which launch, with the launch's N and activation -- from shapes alone: no device, no pointer.  `fwd_tables` / `bwd_tables` turn a
plan into the ctypes group tables `[(groups, G, N, act)]` that `run` hands to an s2p_mlp_linear_* entry point.  Which entry point
is a separate, later choice: `entry_point` names it from the launch's kind, its N and the compute mode ("fp32", or "bf16": the wide
layers on the bf16 matrix cores, SPEC.md N3l), so a table serves both modes."""
from collections import namedtuple

import torch

from ._lib import ACT_NONE, ACT_RELU, MlpBwdGroup, MlpFwdGroup, check, lib, ptr, stream
from .ops import pad_to


class Packed:
    """The layers of one network inside a flat buffer: W [N][Kpad] (K padded to a multiple of 4 with zeros: torch's nn.Linear
    orientation, so a state_dict copy is a row copy), then b [N] in a range padded to a multiple of 4."""

    def __init__(self, dims, base=0):
        self.dims, self.off, n = dims, [], base
        for cin, cout in dims:
            kp = pad_to(cin, 4)
            self.off.append((n, n + cout * kp, kp))
            n += cout * kp + pad_to(cout, 4)
        self.end = n

    def w(self, flat, li):
        (cin, cout), (ow, ob, kp) = self.dims[li], self.off[li]
        return flat[ow:ob].view(cout, kp)

    def b(self, flat, li):
        return flat[self.off[li][1]:self.off[li][1] + self.dims[li][1]]

    def put(self, flat, li, w, b):
        with torch.no_grad():
            self.w(flat, li)[:, :w.shape[1]] = w.to(flat.device, torch.float32)
            self.b(flat, li).copy_(b.to(flat.device, torch.float32))

    def get(self, flat, li):
        return self.w(flat, li)[:, :self.dims[li][0]].detach().cpu().clone(), self.b(flat, li).detach().cpu().clone()


class Net:
    """One network's view for the grouped launches.  The shape half (`name`, the packed layers, the forward row count and the
    backward one: IQL runs vf forward on 2 B rows and backward on the first B) is all a plan needs; `bind` adds the buffers:
    parameters and gradients, the input, the ReLU outputs it keeps (all the backward needs), their gradients, the output and the
    output's gradient, and where the input's gradient goes."""

    def __init__(self, name, pk, rows, bwd_rows=None):
        self.name, self.pk, self.rows, self.bwd_rows = name, pk, rows, bwd_rows

    def bind(self, flat, grad, x, out, dout=None, dx=None, act=None):
        """`act`: the caller's own buffers for the hidden layers' outputs (a forward-only pass may reuse two)."""
        hid, dev, f = [cout for _, cout in self.pk.dims[:-1]], x.device, torch.float32
        self.flat, self.grad, self.x, self.out, self.dout, self.dx = flat, grad, x, out, dout, dx
        self.act = act if act is not None else [torch.empty(self.rows, h, dtype=f, device=dev) for h in hid]
        self.dact = [torch.empty(self.bwd_rows, h, dtype=f, device=dev) for h in hid] if dout is not None else None
        return self


class Launch(namedtuple("Launch", "li N act nets")):
    """One grouped launch: layer `li` of every network of `nets` (in group order).  `act` is the layer's activation in a forward
    plan and the PREVIOUS layer's, whose derivative the input gradient takes, in a backward plan."""


def _by_width(nets, li, one_width):
    """The networks of a layer partitioned by output width, in order of first appearance: the groups of a launch share N."""
    parts = {}
    for n in nets:
        parts.setdefault(n.pk.dims[li][1], []).append(n)
    if one_width and len(parts) != 1:
        raise ValueError("layer %d: output widths %s in one launch" % (li, sorted(parts)))
    return parts.items()


def _depth(nets):
    depths = {len(n.pk.dims) for n in nets}
    if len(depths) != 1:
        raise ValueError("networks of unequal depth in one table: %s" % sorted(depths))
    return depths.pop() - 1


def fwd_plan(nets, one_width=False):
    """One grouped launch per layer and output width: ReLU after the hidden layers, none after the last."""
    L = _depth(nets)
    return [Launch(li, N, ACT_NONE if li == L else ACT_RELU, part) for li in range(L + 1) for N, part in _by_width(nets, li, one_width)]


def bwd_plan(nets, one_width=False):
    """The backward of `fwd_plan`, last layer first."""
    L = _depth(nets)
    return [Launch(li, N, ACT_RELU if li else ACT_NONE, part) for li in range(L, -1, -1) for N, part in _by_width(nets, li, one_width)]


def _pitch(t):
    return t.shape[1] if t.dim() == 2 else 1


def _fwd_group(n, li):
    x, last = (n.x if li == 0 else n.act[li - 1]), li == len(n.pk.dims) - 1
    y = n.out if last else n.act[li]
    return MlpFwdGroup(ptr(x), ptr(n.pk.w(n.flat, li)), ptr(n.pk.b(n.flat, li)), ptr(y) if last else None, None if last else ptr(y),
                       x.shape[1], _pitch(y), n.rows, n.pk.off[li][2])


def _bwd_group(n, li, with_weights):
    x = n.x if li == 0 else n.act[li - 1]
    d = n.dout if li == len(n.pk.dims) - 1 else n.dact[li]
    prev = n.dact[li - 1] if li else n.dx
    return MlpBwdGroup(ptr(x), ptr(d), ptr(n.pk.w(n.flat, li)), ptr(n.pk.w(n.grad, li)) if with_weights else None,
                       ptr(n.pk.b(n.grad, li)) if with_weights else None, ptr(x) if li else None, ptr(prev), x.shape[1], _pitch(d),
                       prev.shape[1] if prev is not None else 0, n.bwd_rows, n.pk.off[li][2])


def _tables(plan, struct, group):
    return [((struct * len(l.nets))(*[group(n, l.li) for n in l.nets]), len(l.nets), l.N, l.act) for l in plan]


def fwd_tables(plan):
    """A forward plan of bound networks -> [(groups, G, N, act)] for s2p_mlp_linear_fwd.  A table holds bare addresses and owns
    no buffer: the caller keeps the bound `Net`s alive as long as it runs the table."""
    return _tables(plan, MlpFwdGroup, _fwd_group)


def bwd_tables(plan, with_weights=True):
    """A backward plan of bound networks -> [(groups, G, N, act_prev)] for s2p_mlp_linear_bwd / _bwd_split; without weights the
    tables feed s2p_mlp_linear_dgrad (dw / db NULL).  The first layer's input gradient goes to the network's `dx`, if it has one.
    As with `fwd_tables`, the caller keeps the bound `Net`s alive."""
    return _tables(plan, MlpBwdGroup, lambda n, li: _bwd_group(n, li, with_weights))


COMPUTE_MODES = ("fp32", "bf16")
ENTRY = dict(fwd="s2p_mlp_linear_fwd", bwd="s2p_mlp_linear_bwd", dgrad="s2p_mlp_linear_dgrad", bwd_split="s2p_mlp_linear_bwd_split")
_KIND = {name: kind for kind, name in ENTRY.items()}


def check_compute(compute):
    if compute not in COMPUTE_MODES:
        raise ValueError("mlp_compute %r (one of %s)" % (compute, ", ".join(COMPUTE_MODES)))
    return compute


def entry_point(kind, N, compute="fp32"):
    """The entry point of a grouped launch of `kind` (fwd, bwd, dgrad, bwd_split) and output width N under a compute mode: the
    `_bf16` entry (SPEC.md N3l: operands rounded to bf16 as a tile loads them, fp32 sums, every tensor fp32) for the MFMA-tile form
    in mode "bf16", the fp32 entry otherwise -- the narrow layers (N <= 16) have no bf16 form."""
    return ENTRY[kind] + "_bf16" if check_compute(compute) == "bf16" and N > 16 else ENTRY[kind]


def run(table, entry="s2p_mlp_linear_fwd", call=None, compute="fp32"):
    """Every launch of a table through `entry` -- for the four entries of `ENTRY`, through what `entry_point` names under `compute`;
    `call(entry, *args)` instead of the plain checked call where the caller counts."""
    st, kind = stream(), _KIND.get(entry)
    for gs, G, N, a in table:
        name = entry_point(kind, N, compute) if kind else entry
        if call is not None:
            call(name, gs, G, N, a, st)
        else:
            check(getattr(lib(), name)(gs, G, N, a, st), name)


def split_chunks(tiles, rows, max_rows=1024, waves=1024, cap=8):
    """S of s2p_mlp_linear_bwd_split for a launch of `tiles` weight tiles over `rows` rows: enough chunks that the weight waves reach
    the chip's 1 024 SIMDs and that no wave sums more than `max_rows` rows in one chain (the accuracy floor), at most `cap`.  Measured at
    7 936 rows: K 296 is fastest at S = 8, K 1024 at S = 4 with S = 8 within 4 % (the table of DESIGN.md section 6b.5)."""
    return max(1, min(cap, max(-(-waves // max(tiles, 1)), -(-rows // max_rows))))
