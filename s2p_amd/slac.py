"""SLAC encoder / decoder conv stacks on HIP: the first consumer of the generated frames
(`rlkit/torch/slac/network/latent.py:116-171` Encoder, `:55-113` Decoder, image_size 100 branches), trained on every RL
step (`iql_trainer.py:348-350`).  Mirrors the reference call surface -- `Encoder(input_dim, output_dim, image_size)(x
[B,S,C,H,W]) -> [B,S,256]`, `Decoder(input_dim, output_dim, std, image_size)(z [B,S,L]) -> (mean [B,S,3,100,100], std)`
-- as `nn.Module`s whose parameters carry the reference's state_dict keys (`net.<2i>.weight/bias`, reference layouts),
so reference checkpoints load natively and any torch optimizer trains them.

Forward: every layer is one implicit-GEMM launch with bias + LeakyReLU(0.2) fused in the epilogue (conv-transpose layers
run as merged sub-pixel phases); activations stay NHWC in HBM between layers.
Backward: the whole stack is ONE autograd node.  Per layer, in reverse: wgrad (bias gradient fused for the gather
form) straight from the saved NHWC activations, and a dgrad whose epilogue multiplies by the LeakyReLU derivative of
the layer below (EPI_MUL_ACTGRAD), so no separate activation-backward pass runs between layers.
"""
import torch
import torch.nn as nn

from . import ops
from ._lib import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_TANH, EPI_MUL_ACTGRAD, chunk_elems
from .ops import ConvGeom, pad_to
from .slac_buffer import FrameBatch

ENCODER_100 = [("conv", 3, 32, 5, 2, 2, 0), ("conv", 32, 64, 3, 2, 1, 0), ("conv", 64, 128, 3, 2, 1, 0),
               ("conv", 128, 256, 3, 2, 1, 0), ("conv", 256, 256, 3, 2, 1, 0), ("conv", 256, 256, 4, 1, 0, 0)]
DECODER_100 = [("convT", 288, 256, 4, 1, 0, 0), ("convT", 256, 256, 3, 2, 1, 0), ("convT", 256, 128, 3, 2, 1, 0),
               ("convT", 128, 64, 3, 2, 1, 0), ("convT", 64, 32, 3, 2, 1, 1), ("convT", 32, 3, 5, 2, 2, 1)]
SLOPE = 0.2


class _Layer(nn.Module):
    """Parameter holder under the reference's key (`net.<2i>`); weight in the torch layout of the reference layer."""

    def __init__(self, kind, cin, cout, k):
        super().__init__()
        shape = (cout, cin, k, k) if kind == "conv" else (cin, cout, k, k)
        self.weight = nn.Parameter(torch.zeros(shape))
        self.bias = nn.Parameter(torch.zeros(cout))


class _StackFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, stack, *params):
        packed = stack.packed()
        acts, h = [x], x
        for (geom, cin_pad, _), (wf, _, b) in zip(stack.meta, packed):
            h = ops.conv_fwd(geom, h, wf, b, cin_pad, act=ACT_LRELU, slope=SLOPE)
            acts.append(h)
        ctx.stack, ctx.packed = stack, packed
        ctx.acts = acts if torch.is_grad_enabled() or any(ctx.needs_input_grad) else None
        return h

    @staticmethod
    def backward(ctx, dy):
        stack, acts, packed = ctx.stack, ctx.acts, ctx.packed
        dev = dy.device
        need_dx = ctx.needs_input_grad[0]
        d = ops.act_bwd(dy.contiguous(), acts[-1], ACT_LRELU, SLOPE)     # gradient wrt the last pre-activation
        grads = [None] * (2 * len(stack.meta))
        for i in reversed(range(len(stack.meta))):
            geom, cin_pad, (kind, cin, cout, k) = stack.meta[i]
            x_i = acts[i]
            tr = kind == "convT"
            rows, cols = (cin, cout) if tr else (cout, cin)
            dw = torch.zeros((rows, k * k, cols), dtype=torch.float32, device=dev)
            db = torch.zeros(cout, dtype=torch.float32, device=dev)
            if tr:                                                       # scatter form: bias gradient is a plain channel sum
                ops.conv_wgrad(geom, x_i, d, dw, cin_pad, cin, cout, deterministic=True)
                ops.channel_sum(d, cout, db, deterministic=True)
            else:                                                        # (deterministic: no atomics in fp32 either)
                ops.conv_wgrad(geom, x_i, d, dw, cin_pad, cin, cout, db=db, deterministic=True)
            grads[2 * i] = dw.reshape(rows, k, k, cols).permute(0, 3, 1, 2).contiguous()
            grads[2 * i + 1] = db
            if i > 0:                                                    # x_i = lrelu(pre_{i-1}): fold its derivative in
                d = ops.conv_dgrad(geom, d, packed[i][1], tuple(x_i.shape), cin_pad, aux=x_i, epi=EPI_MUL_ACTGRAD,
                                   aux_act=ACT_LRELU, slope=SLOPE)
            elif need_dx:
                d = ops.conv_dgrad(geom, d, packed[i][1], tuple(x_i.shape), cin_pad)
        ctx.acts = None
        return (d if need_dx else None, None) + tuple(grads)


class _Stack(nn.Module):
    def __init__(self, spec, dtype, device):
        super().__init__()
        self.spec, self.dtype = spec, dtype
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("the SLAC conv stacks run on a HIP device only (no CPU fallback)")
        self.net = nn.Module()
        ce = chunk_elems(dtype)
        self.meta = []
        for i, (kind, cin, cout, k, s, pad, op) in enumerate(spec):
            self.net.add_module(str(2 * i), _Layer(kind, cin, cout, k))
            geom = ConvGeom(cin, cout, k, s, pad, transposed=(kind == "convT"), output_padding=op)
            self.meta.append((geom, pad_to(cin, ce), (kind, cin, cout, k)))
        self.to(dev)
        self._pack_key, self._packed = None, None

    @property
    def device(self):
        return self.net._modules["0"].weight.device

    def load_state_dict(self, sd, strict=True):
        """Accepts the reference's state_dict (tensors or numpy arrays); returns self for chaining."""
        sd = {k: torch.as_tensor(v, dtype=torch.float32) for k, v in sd.items()}
        super().load_state_dict(sd, strict=strict)
        return self

    def layer_params(self):
        out = []
        for i in range(len(self.spec)):
            m = self.net._modules[str(2 * i)]
            out += [m.weight, m.bias]
        return out

    def packed(self):
        """Compute-dtype GEMM operands of every layer: w_fwd [Cout][tap][Cin_pad], w_bwd [Cin_pad][tap][Cout_pad], bias.
        Re-packed only when a parameter changed (optimizer step / load)."""
        ps = self.layer_params()
        key = tuple((p.data_ptr(), p._version) for p in ps)
        if key == self._pack_key:
            return self._packed
        ce = chunk_elems(self.dtype)
        out = []
        with torch.no_grad():
            for i, (kind, cin, cout, k, s, pad, op) in enumerate(self.spec):
                w, b = ps[2 * i], ps[2 * i + 1]
                w_std = w if kind == "conv" else w.permute(1, 0, 2, 3)          # [Cout,Cin,kh,kw] view
                cin_pad, cout_pad = pad_to(cin, ce), pad_to(cout, ce)
                wf = torch.zeros((cout, k * k, cin_pad), dtype=torch.float32, device=w.device)
                wf[:, :, :cin] = w_std.permute(0, 2, 3, 1).reshape(cout, k * k, cin)
                wb = torch.zeros((cin_pad, k * k, cout_pad), dtype=torch.float32, device=w.device)
                wb[:cin, :, :cout] = w_std.permute(1, 2, 3, 0).reshape(cin, k * k, cout)
                out.append((wf.to(self.dtype).contiguous(), wb.to(self.dtype).contiguous(), b.detach().float().contiguous()))
        self._pack_key, self._packed = key, out
        return out

    def run(self, x_nhwc):
        return _StackFn.apply(x_nhwc, self, *self.layer_params())


class _ToNchw(torch.autograd.Function):
    """NHWC (padded pitch) -> fp32 NCHW; the backward re-pads with zeros so padded channels carry no gradient."""

    @staticmethod
    def forward(ctx, y, C):
        ctx.dt, ctx.pitch = y.dtype, y.shape[3]
        return ops.nhwc_to_nchw(y, C)

    @staticmethod
    def backward(ctx, g):
        return ops.nchw_to_nhwc(g.contiguous().float(), ctx.dt, ctx.pitch), None


class Encoder(_Stack):
    def __init__(self, input_dim=3, output_dim=256, image_size=100, dtype=torch.float32, device="cuda:0"):
        if image_size != 100 or input_dim != 3 or output_dim != 256:
            raise NotImplementedError("only the image_size=100 configuration used by the shipped run scripts is built")
        super().__init__(ENCODER_100, dtype, device)

    def forward(self, x):
        """x: fp32 [B,S,3,100,100] in [0,1] (or uint8 NHWC frames [B,S,100,100,3], or a FrameBatch) -> fp32 [B,S,256].
        Frames are data: no gradient is produced for x."""
        dev = self.device
        if isinstance(x, FrameBatch):
            B, S = x.shape[:2]
            h = x.nhwc
            if h.dtype == self.dtype and h.shape[3] == chunk_elems(self.dtype) and h.device == dev:
                return self.run(h).reshape(B, S, -1).float()           # the replay buffer's gather wrote the encoder's input
            x = x.u8
        with torch.no_grad():
            if x.dtype == torch.uint8:
                B, S = x.shape[:2]
                frames = x.reshape(B * S, *x.shape[2:]).to(dev).contiguous()
                h = ops.u8_to_nhwc(frames, self.dtype, chunk_elems(self.dtype))      # [-1,1]; SLAC wants [0,1]:
                h = (h.float() + 1.0).mul_(0.5).to(self.dtype)
                h[..., 3:] = 0
            else:
                B, S, C, H, W = x.shape
                h = ops.nchw_to_nhwc(x.reshape(B * S, C, H, W).to(dev, torch.float32).contiguous(), self.dtype,
                                     chunk_elems(self.dtype))
        y = self.run(h)                                            # [B*S,1,1,256]
        return y.reshape(B, S, -1).float()


class Decoder(_Stack):
    def __init__(self, input_dim=288, output_dim=3, std=1.0, image_size=100, dtype=torch.float32, device="cuda:0"):
        if image_size != 100 or input_dim != 288 or output_dim != 3:
            raise NotImplementedError("only the image_size=100 configuration used by the shipped run scripts is built")
        super().__init__(DECODER_100, dtype, device)
        self.std = std

    def forward(self, z):
        """z: fp32 [B,S,288] -> (mean fp32 [B,S,3,100,100], std tensor filled with self.std).  Differentiable in z."""
        B, S, L = z.shape
        h = z.to(self.device).reshape(B * S, 1, 1, L).to(self.dtype).contiguous()
        y = self.run(h)                                            # [B*S,100,100,pitch]
        img = _ToNchw.apply(y, 3).reshape(B, S, 3, y.shape[1], y.shape[2])
        return img, torch.full_like(img, self.std)


# ---- the latent model (SPEC.md N3b; reference latent.py:174-311) ---------------------------------------------------------
Z1, Z2, HID, FEAT = 32, 256, 256, 256
_LOG_STD_MIN = 1e-5


def _f32(shape, dev, zero=False):
    return (torch.zeros if zero else torch.empty)(shape, dtype=torch.float32, device=dev)


class _Lin(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(cout, cin))
        self.bias = nn.Parameter(torch.zeros(cout))
        nn.init.xavier_uniform_(self.weight, gain=1.0)


class Gaussian(nn.Module):
    """Linear -> LeakyReLU(0.2) -> Linear -> LeakyReLU(0.2) -> Linear(2D); mean | raw = chunk, std = softplus(raw) + 1e-5
    (latent.py:29-52).  Parameters under the reference's keys `net.{0,2,4}.{weight,bias}`.  `groups` splits the first layer's
    input columns into separately packed operands (the chain part and the part hoisted out of the chain)."""

    def __init__(self, input_dim, output_dim, hidden_units=(256, 256), groups=None):
        super().__init__()
        if tuple(hidden_units) != (HID, HID):
            raise NotImplementedError("only hidden_units=(256, 256) is built")
        self.input_dim, self.D = input_dim, output_dim
        self.N = 2 * output_dim
        self.Npad = pad_to(self.N, 4)
        self.groups = groups if groups is not None else [[(0, input_dim)]]
        self.net = nn.Module()
        self.net.add_module("0", _Lin(input_dim, HID))
        self.net.add_module("2", _Lin(HID, HID))
        self.net.add_module("4", _Lin(HID, self.N))
        self._pack_key, self._packed = None, None
        self._cols_key, self._cols = None, {}
        self._bf16_key, self._bf16 = None, {}
        self._bf16g_key, self._bf16g = None, None

    def layer_params(self):
        out = []
        for i in (0, 2, 4):
            m = self.net._modules[str(i)]
            out += [m.weight, m.bias]
        return out

    def packed(self):
        """fp32 GEMM operands: per first-layer column group (w [256][Kpad], its transpose [Kpad][256], K); w2 / w3 and their
        transposes, the last layer padded to a multiple of 4 rows.  Re-packed only when a parameter changed."""
        ps = self.layer_params()
        key = tuple((p.data_ptr(), p._version) for p in ps)
        if key == self._pack_key:
            return self._packed
        with torch.no_grad():
            w1, b1, w2, b2, w3, b3 = [p.detach().float() for p in ps]
            g1 = []
            for cols in self.groups:
                w = torch.cat([w1[:, a:b] for a, b in cols], dim=1)
                k = w.shape[1]
                wp = _f32((HID, pad_to(k, 4)), w.device, zero=True)
                wp[:, :k] = w
                g1.append((wp, wp.t().contiguous(), k))
            w3p = _f32((self.Npad, HID), w3.device, zero=True)
            w3p[:self.N] = w3
            b3p = _f32((self.Npad,), w3.device, zero=True)
            b3p[:self.N] = b3
            out = dict(g1=g1, b1=b1.contiguous(), w2=w2.contiguous(), w2t=w2.t().contiguous(), b2=b2.contiguous(), w3=w3p,
                       w3t=w3p.t().contiguous(), b3=b3p)
        self._pack_key, self._packed = key, out
        return out

    def packed_bf16(self, k1=None):
        """The operands of the bf16-compute chains (SPEC.md N3m), beside packed() and under its key rule: w1 [256][k1] = the chain
        operand of the first layer, i.e. the first column group (`k1`: only its leading k1 columns, as a pack of their own -- z1_prior's
        256 z2 columns in the prior chain), w2 [256][256], w3 [2 D][256].  Each is the fp32 parameter `.to(torch.bfloat16)` (round to
        nearest even); the biases are packed()'s fp32 ones.  The other column groups stay in the hoisted fp32 GEMMs."""
        ps = self.layer_params()
        key = tuple((p.data_ptr(), p._version) for p in ps)
        if key != self._bf16_key:
            self._bf16_key, self._bf16 = key, {}
        if k1 not in self._bf16:
            pk = self.packed()
            with torch.no_grad():
                w1, _, w2, _, w3, _ = [p.detach().float() for p in ps]
                w = torch.cat([w1[:, a:b] for a, b in self.groups[0]], dim=1)
                w = w if k1 is None else w[:, :k1]
                if w.shape[1] % 8:
                    raise ValueError("a bf16 chain operand has a multiple of 8 columns, not %d" % w.shape[1])
                bf = lambda t: t.to(torch.bfloat16).contiguous()
                self._bf16[k1] = dict(w1=bf(w), b1=pk["b1"], w2=bf(w2), b2=pk["b2"], w3=bf(w3), b3=pk["b3"])
        return self._bf16[k1]

    def packed_bf16_grad(self):
        """The operands of the bf16-compute chain under grad (SPEC.md N3p), beside packed_bf16() and under its key rule: its w1 (the
        first column group), w2, w3 and their transposes w1t [k1][256], w2t [256][256], w3t [256][2 D] -- the same rounded values --
        made from the fp32 parameters in place by ONE launch (ops.chain_pack_bf16): under training the parameters change every step.
        The biases are packed()'s fp32 ones."""
        ps = self.layer_params()
        key = tuple((p.data_ptr(), p._version) for p in ps)
        if key != self._bf16g_key:
            pk = self.packed()
            with torch.no_grad():
                w1, _, w2, _, w3, _ = [p.detach() for p in ps]
                if any(w.dtype != torch.float32 for w in (w1, w2, w3)):
                    raise ValueError("the bf16 chain packs are made from fp32 parameters")
                k1 = sum(b - a for a, b in self.groups[0])
                if k1 % 8:
                    raise ValueError("a bf16 chain operand has a multiple of 8 columns, not %d" % k1)
                bf = lambda *shape: torch.empty(shape, dtype=torch.bfloat16, device=w1.device)
                out = dict(w1=bf(HID, k1), w1t=bf(k1, HID), b1=pk["b1"], w2=bf(HID, HID), w2t=bf(HID, HID), b2=pk["b2"],
                           w3=bf(self.N, HID), w3t=bf(HID, self.N), b3=pk["b3"])
                jobs, o = [(w2, out["w2"], out["w2t"]), (w3, out["w3"], out["w3t"])], 0
                for a, b in self.groups[0]:
                    jobs.append((w1[:, a:b], out["w1"][:, o:o + b - a], out["w1t"][o:o + b - a]))
                    o += b - a
                ops.chain_pack_bf16(jobs)
            self._bf16g_key, self._bf16g = key, out
        return self._bf16g

    def packed_cols(self, lo, hi):
        """net.0.weight[:, lo:hi] as a GEMM operand of its own, [256][(hi - lo) padded to 4] with a zero pad, beside packed() and
        under its key rule (the prior chain hoists z1_prior's action columns; packed() keeps that head's one [z2 | a] group)."""
        ps = self.layer_params()
        key = tuple((p.data_ptr(), p._version) for p in ps)
        if key != self._cols_key:
            self._cols_key, self._cols = key, {}
        if (lo, hi) not in self._cols:
            with torch.no_grad():
                w1 = ps[0].detach().float()
                wp = _f32((HID, pad_to(hi - lo, 4)), w1.device, zero=True)
                wp[:, :hi - lo] = w1[:, lo:hi]
            self._cols[(lo, hi)] = wp
        return self._cols[(lo, hi)]

    def unpack_dw1(self, dws):
        """Gradients of the packed first-layer groups -> the gradient of net.0.weight (reference column order)."""
        dw = torch.empty_like(self.net._modules["0"].weight)
        for cols, g in zip(self.groups, dws):
            o = 0
            for a, b in cols:
                dw[:, a:b] = g[:, o:o + b - a]
                o += b - a
        return dw


def _mlp_tail_fwd(g, pk, h1, h2, raw):
    """Layers 2 and 3 on a first-layer output h1 (views [M, 256]); raw: [M, Npad]."""
    ops.linear_fwd_into(h1, pk["w2"], pk["b2"], HID, h2, ACT_LRELU, SLOPE)
    ops.linear_fwd_into(h2, pk["w3"], pk["b3"], g.Npad, raw)


def _mlp_tail_dgrad(g, pk, draw, h2, dh2, h1, dh1):
    """dL/dh2 and dL/dh1 from dL/draw: the two launches of the backward that ARE sequential (weight gradients are not)."""
    ops.linear_add_bwd(draw, None, g.Npad, ACT_NONE, w_bwd=pk["w3t"], dx=dh2)
    ops.linear_add_bwd(dh2, h2, HID, ACT_LRELU, SLOPE, w_bwd=pk["w2t"], dx=dh1)


def _mlp_tail_wgrad(g, pk, draw, h2, dh2, h1, dev):
    """Weight / bias gradients of layers 2 and 3 over all rows in one launch each (s2p_linear_bwd's wgrad pass)."""
    dw3, db3 = _f32((g.Npad, HID), dev, True), _f32((g.Npad,), dev, True)
    dw2, db2 = _f32((HID, HID), dev, True), _f32((HID,), dev, True)
    ops.linear_add_bwd(draw, None, g.Npad, ACT_NONE, x=h2, k_real=HID, dw=dw3, db=db3)
    ops.linear_add_bwd(dh2, h2, HID, ACT_LRELU, SLOPE, x=h1, k_real=HID, dw=dw2, db=db2)
    return dw2, db2, dw3[:g.N], db3[:g.N]


def _mlp_fwd(g, pk, x, M, dev):
    h1, h2, raw = _head_state([g], (M,), dev)[0]
    ops.linear_fwd_into(x, pk["g1"][0][0], pk["b1"], HID, h1, ACT_LRELU, SLOPE)
    _mlp_tail_fwd(g, pk, h1, h2, raw)
    return h1, h2, raw


def _mlp_bwd(g, pk, x, h1, h2, draw, dev, need_dx=True):
    """Whole backward of an MLP that is not inside the chain (all rows known): -> (grads of the 6 parameters, dx)."""
    M = x.shape[0]
    dh2, dh1 = _f32((M, HID), dev), _f32((M, HID), dev)
    _mlp_tail_dgrad(g, pk, draw, h2, dh2, h1, dh1)
    dw2, db2, dw3, db3 = _mlp_tail_wgrad(g, pk, draw, h2, dh2, h1, dev)
    w1, w1t, k = pk["g1"][0]
    dw1, db1 = _f32((HID, k), dev, True), _f32((HID,), dev, True)
    dx = _f32((M, w1.shape[1]), dev) if need_dx else None
    ops.linear_add_bwd(dh1, h1, HID, ACT_LRELU, SLOPE, x=x, k_real=k, dw=dw1, db=db1, w_bwd=w1t, dx=dx)
    return [g.unpack_dw1([dw1]), db1, dw2, db2, dw3, db3], dx


def _action_term(action, w):
    """a . w^T of the action columns `w` [256][A padded to 4] of a first layer over all S*B rows, without bias: action [B,S,A] ->
    (the padded input [S,B,Kpad], the term [S*B, 256]), both time-major.  One s2p_linear_fwd."""
    dev = action.device
    B, S, A = action.shape
    k = w.shape[1]
    x = _f32((S, B, k), dev, True)
    x[:, :, :A] = action.transpose(0, 1)
    r = _f32((S * B, HID), dev)
    ops.linear_fwd_into(x.view(S * B, k), w, None, HID, r)
    return x, r


def _chain_step(g1, p1, g2, p2, bufa, bufb, add_a, add_b, noise, mean, std, z, t, xz, xz_next):
    """One step of a latent chain, 8 launches: the z1 head (g1, p1) on xz[:, Z1:] = z2(t-1) plus the row term add_a, then the z2 head
    (g2, p2) on xz = z1(t) | z2(t-1) plus add_b.  Both read the chain columns of their first layer in place (p["g1"][0]).  Results go
    to slot t of mean, std [B,T,32] and z [B,T,288] with the eps of noise [B,T,288], z1(t) to xz[:, :Z1] and z2(t) to the z2 columns
    of the next step's input row xz_next (None: there is no next step).  bufa / bufb: each head's (h1, h2, raw)."""
    (h1a, h2a, rawa), (h1b, h2b, rawb) = bufa, bufb
    ops.linear_fwd_into(xz[:, Z1:], p1["g1"][0][0], p1["b1"], HID, h1a, ACT_LRELU, SLOPE, add=add_a)
    _mlp_tail_fwd(g1, p1, h1a, h2a, rawa)
    ops.gauss_head_fwd(rawa, Z1, eps=noise[:, t, :Z1], mean=mean[:, t], std=std[:, t], z=z[:, t, :Z1], z2=xz[:, :Z1])
    ops.linear_fwd_into(xz, p2["g1"][0][0], p2["b1"], HID, h1b, ACT_LRELU, SLOPE, add=add_b)
    _mlp_tail_fwd(g2, p2, h1b, h2b, rawb)
    ops.gauss_head_fwd(rawb, Z2, eps=noise[:, t, Z1:], z=z[:, t, Z1:], z2=xz_next[:, Z1:] if xz_next is not None else None)


class _GaussFn(torch.autograd.Function):
    """A Gaussian head on rows that are all known up front (z1_prior, reward): x [M, Kpad] -> mean, std [M, D]."""

    @staticmethod
    def forward(ctx, x, g, *params):
        dev, M = x.device, x.shape[0]
        pk = g.packed()
        h1, h2, raw = _mlp_fwd(g, pk, x, M, dev)
        mean, std = _f32((M, g.D), dev), _f32((M, g.D), dev)
        ops.gauss_head_fwd(raw, g.D, mean=mean, std=std)
        ctx.g, ctx.pk = g, pk
        ctx.saved = (x, h1, h2, raw) if torch.is_grad_enabled() or any(ctx.needs_input_grad) else None
        return mean, std

    @staticmethod
    def backward(ctx, dmean, dstd):
        g, pk = ctx.g, ctx.pk
        x, h1, h2, raw = ctx.saved
        dev = x.device
        draw = _f32(raw.shape, dev, True)
        ops.gauss_head_bwd(raw, g.D, draw, dmean=dmean.contiguous(), dstd=dstd.contiguous())
        grads, dx = _mlp_bwd(g, pk, x, h1, h2, draw, dev, need_dx=ctx.needs_input_grad[0])
        ctx.saved = None
        return (dx, None) + tuple(grads)


def _head_state(gs, lead, dev):
    """The posterior chain's backward state of the Gaussian heads `gs`, uninitialised: per head (h1, h2, raw) on rows of the leading
    shape `lead` -- (B,) for the two t = 0 heads, (Tn, B) for the two chain heads -- in the order `ops.chain_state` and
    `_PosteriorFn.backward` read them, whichever forward form fills them."""
    return [(_f32(lead + (HID,), dev), _f32(lead + (HID,), dev), _f32(lead + (g.Npad,), dev)) for g in gs]


def _chain_mlps(packs):
    return [ops.chain_mlp(p) for p in packs]


def _chain_mlps_bf16(heads):
    return [ops.chain_mlp_bf16(g.packed_bf16()) for g in heads]


def _chain_grad_compute(model):
    """`model.chain_grad_compute`, read where a fused chain under grad is about to run: "fp32" or "bf16" (SPEC.md N3p)."""
    mode = getattr(model, "chain_grad_compute", "fp32")
    if mode not in ("fp32", "bf16"):
        raise ValueError("chain_grad_compute is 'fp32' or 'bf16', not %r" % (mode,))
    return mode


class _PosteriorFn(torch.autograd.Function):
    """The reparameterised posterior chain (latent.py:250-281) as ONE autograd node over HIP launches.
    feat [B,T,256], action [B,T-1,A], noise [B,T,288] (keep: the caller's grad mode; activations are saved only then) -> z1_mean [B,T,32], z1_std [B,T,32], z [B,T,288] (z1 | z2).
    Per time step the chain is 8 launches forward (2 x (3 layers + head)) and 8 backward (2 x (head + 3 dgrads)): the
    feature / action columns of the two first layers are one batched GEMM before the chain, every weight gradient and the
    feature / action gradients are batched launches after it.  `model.chain_form(keep)` names what the forward does with the chain
    itself: "layers" runs those 8 launches per step; "fused" / "fused_bf16" (`model.fused_chain`, no backward state kept) run it as
    one launch (SPEC.md N3h, bitwise the same; N3m, bf16 operands); "fused_save" (`model.fused_chain_grad`, state kept) as one launch
    that also stores that state, with the 8 S sequential launches of the backward as one (SPEC.md N3k), bitwise the same again.
    With "fused_save", `model.chain_grad_compute == "bf16"` (SPEC.md N3p) gives those two launches bf16 operands: mixed precision, not
    the same numbers; the state, every weight gradient and the t = 0 backward stay the fp32 launches on unrounded tensors."""

    @staticmethod
    def forward(ctx, feat, action, noise, model, keep, *params):
        dev = feat.device
        B, T, _ = feat.shape
        S = T - 1
        form = model.chain_form(keep)
        ctx.fused = form == "fused_save"                               # the backward follows what the forward did
        ctx.bf16_packs = None                                          # SPEC.md N3p: the packs the forward multiplied with
        if ctx.fused and _chain_grad_compute(model) == "bf16":
            ctx.bf16_packs = [g.packed_bf16_grad() for g in model._chain_heads()]
        gs = gi1, gi2, g1, g2 = model._chain_heads()
        packs = pi1, pi2, p1, p2 = tuple(g.packed() for g in gs)
        z = _f32((B, T, Z1 + Z2), dev)
        mean, std = _f32((B, T, Z1), dev), _f32((B, T, Z1), dev)
        xz = a0 = b0 = chain = xa = xb = ra = rb = None
        state = form in ("layers", "fused_save")                       # the forms that fill backward state: its one allocation
        Tn = max(S, 1) if keep else 1                                  # time slots of that state: one when it is not kept
        if state:
            xz = _f32((Tn, B, Z1 + Z2), dev)                           # [slot(t)] = z1(t) | z2(t-1): the chain's input rows
        if form == "fused_save":
            a0, b0 = _head_state(gs[:2], (B,), dev)
        elif form == "layers":                                         # t = 0: q(z1(0) | feat(0)), q(z2(0) | z1(0))
            a0 = _mlp_fwd(gi1, pi1, feat[:, 0], B, dev)
            ops.gauss_head_fwd(a0[2], Z1, eps=noise[:, 0, :Z1], mean=mean[:, 0], std=std[:, 0], z=z[:, 0, :Z1])
            b0 = _mlp_fwd(gi2, pi2, z[:, 0, :Z1], B, dev)
            ops.gauss_head_fwd(b0[2], Z2, eps=noise[:, 0, Z1:], z=z[:, 0, Z1:], z2=xz[0][:, Z1:] if S > 0 else None)
        if S > 0:
            xa, xb, ra, rb = _PosteriorFn._hoisted(feat, action, p1, p2)
            if state:
                chain = sum(_head_state(gs[2:], (Tn, B), dev), ())     # h1a, h2a, rawa, h1b, h2b, rawb
        if form == "fused":                                            # the whole chain, t = 0 included, as ONE launch (SPEC.md N3h)
            ops.posterior_chain_fwd(feat[:, 0], ra, rb, noise, _chain_mlps(packs), mean, std, z)
        elif form == "fused_bf16":                                     # SPEC.md N3m: the same launch count, bf16 operands
            ops.posterior_chain_fwd_bf16(feat[:, 0], ra, rb, noise, _chain_mlps_bf16(gs), mean, std, z)
        elif form == "fused_save" and ctx.bf16_packs:                  # SPEC.md N3p: the same launch count, bf16 operands
            ops.posterior_chain_fwd_save_bf16(feat[:, 0], ra, rb, noise, [ops.chain_mlp_bf16(p) for p in ctx.bf16_packs], mean, std, z,
                                              ops.chain_state(a0, b0, chain + (xz,) if chain else None))
        elif form == "fused_save":                                     # one launch that also fills the state (SPEC.md N3k)
            ops.posterior_chain_fwd_save(feat[:, 0], ra, rb, noise, _chain_mlps(packs), mean, std, z,
                                         ops.chain_state(a0, b0, chain + (xz,) if chain else None))
        else:
            slot = (lambda t: t - 1) if keep else (lambda t: 0)
            for t in range(1, T):
                s, r = slot(t), slice((t - 1) * B, t * B)
                # q(z1(t) | feat(t), z2(t-1), a(t-1)), q(z2(t) | z1(t), z2(t-1), a(t-1))
                _chain_step(g1, p1, g2, p2, tuple(c[s] for c in chain[:3]), tuple(c[s] for c in chain[3:]), ra[r], rb[r], noise, mean, std, z, t,
                            xz[s], xz[slot(t + 1)] if t < S else None)
        sv = (xa, xb) + chain if keep and S > 0 else None             # every form leaves the same behind: operands, state, its bytes
        ctx.model, ctx.packs, ctx.A = model, packs, action.shape[2]
        ctx.saved = (feat, noise, z, xz, a0, b0, sv) if keep else None
        model.chain_state_bytes = sum(t.numel() * 4 for t in (xz,) + a0 + b0 + (sv or ())) if keep else 0
        return mean, std, z

    @staticmethod
    def _hoisted(feat, action, p1, p2):
        """What does not depend on the chain: feat(t) | a(t-1) -> the row term of z1_posterior's first layer, a(t-1) -> z2_posterior's.
        Returns the two inputs [S,B,Kpad] and the two terms [S*B, 256] (time-major)."""
        dev = feat.device
        B, T, _ = feat.shape
        S, A = T - 1, action.shape[2]
        ka = p1["g1"][1][0].shape[1]
        xa = _f32((S, B, ka), dev, True)
        xa[:, :, :FEAT] = feat[:, 1:].transpose(0, 1)
        xa[:, :, FEAT:FEAT + A] = action.transpose(0, 1)
        ra = _f32((S * B, HID), dev)
        ops.linear_fwd_into(xa.view(S * B, ka), p1["g1"][1][0], None, HID, ra)
        xb, rb = _action_term(action, p2["g1"][1][0])
        return xa, xb, ra, rb

    @staticmethod
    def backward(ctx, dmean, dstd, dz):
        model, A = ctx.model, ctx.A
        pi1, pi2, p1, p2 = ctx.packs
        gi1, gi2, g1, g2 = model._chain_heads()
        feat, noise, z, xz, a0, b0, sv = ctx.saved
        dev = feat.device
        B, T, _ = feat.shape
        S = T - 1
        dmean = dmean.contiguous() if dmean is not None else _f32((B, T, Z1), dev, True)
        dstd = dstd.contiguous() if dstd is not None else _f32((B, T, Z1), dev, True)
        dz = dz.contiguous() if dz is not None else _f32((B, T, Z1 + Z2), dev, True)
        g_chain, dfeat, daction = [None] * 12, _f32((B, T, FEAT), dev), None
        dxz = None
        if S > 0:
            xa, xb, h1a, h2a, rawa, h1b, h2b, rawb = sv
            dxz = _f32((S, B, Z1 + Z2), dev)                           # gradient at z1(t) | z2(t-1), slot t - 1
            drawa, dh2a, dh1a = _f32((S, B, g1.Npad), dev), _f32((S, B, HID), dev), _f32((S, B, HID), dev)
            drawb, dh2b, dh1b = _f32((S, B, g2.Npad), dev), _f32((S, B, HID), dev), _f32((S, B, HID), dev)
            steps = range(S, 0, -1)
            if ctx.fused and ctx.bf16_packs:                           # the loop below as ONE launch in bf16 compute (SPEC.md N3p)
                ops.posterior_chain_bwd_bf16(noise, dmean, dstd, dz, [ops.chain_mlp_bwd_bf16(p) for p in ctx.bf16_packs[2:]],
                                             ops.chain_state(a0, b0, sv[2:] + (xz,)), (drawa, dh2a, dh1a, drawb, dh2b, dh1b, dxz))
                steps = ()
            elif ctx.fused:                                            # the loop below as ONE launch (s2p_posterior_chain_bwd)
                ops.posterior_chain_bwd(noise, dmean, dstd, dz, [ops.chain_mlp_bwd(p1), ops.chain_mlp_bwd(p2)],
                                        ops.chain_state(a0, b0, sv[2:] + (xz,)), (drawa, dh2a, dh1a, drawb, dh2b, dh1b, dxz))
                steps = ()
            for t in steps:
                s = t - 1
                ops.gauss_head_bwd(rawb[s], Z2, drawb[s], eps=noise[:, t, Z1:], dz=dz[:, t, Z1:], dz2=dxz[t][:, Z1:] if t < S else None)
                _mlp_tail_dgrad(g2, p2, drawb[s], h2b[s], dh2b[s], h1b[s], dh1b[s])
                ops.linear_add_bwd(dh1b[s], h1b[s], HID, ACT_LRELU, SLOPE, w_bwd=p2["g1"][0][1], dx=dxz[s])
                ops.gauss_head_bwd(rawa[s], Z1, drawa[s], eps=noise[:, t, :Z1], dmean=dmean[:, t], dstd=dstd[:, t], dz=dz[:, t, :Z1],
                                   dz2=dxz[s][:, :Z1])
                _mlp_tail_dgrad(g1, p1, drawa[s], h2a[s], dh2a[s], h1a[s], dh1a[s])
                ops.linear_add_bwd(dh1a[s], h1a[s], HID, ACT_LRELU, SLOPE, w_bwd=p1["g1"][0][1], dx=dxz[s][:, Z1:], accumulate=True)
        # t = 0
        drb0 = _f32(b0[2].shape, dev)
        ops.gauss_head_bwd(b0[2], Z2, drb0, eps=noise[:, 0, Z1:], dz=dz[:, 0, Z1:], dz2=dxz[0][:, Z1:] if S > 0 else None)
        g_i2, dz10 = _mlp_bwd(gi2, pi2, z[:, 0, :Z1], b0[0], b0[1], drb0, dev)
        dra0 = _f32(a0[2].shape, dev)
        ops.gauss_head_bwd(a0[2], Z1, dra0, eps=noise[:, 0, :Z1], dmean=dmean[:, 0], dstd=dstd[:, 0], dz=dz[:, 0, :Z1], dz2=dz10)
        g_i1, dfeat0 = _mlp_bwd(gi1, pi1, feat[:, 0], a0[0], a0[1], dra0, dev)
        dfeat[:, 0] = dfeat0
        if S > 0:
            # after the chain: every weight gradient of the two chain MLPs, and the feature / action gradients, over all S*B rows
            M = S * B
            f2 = lambda t: t.view(M, t.shape[-1])
            for j, (g, p, dr, h2, dh2, h1, dh1, xrow, xchain) in enumerate((
                    (g1, p1, drawa, h2a, dh2a, h1a, dh1a, xa, f2(xz)[:, Z1:]), (g2, p2, drawb, h2b, dh2b, h1b, dh1b, xb, f2(xz)))):
                dw2, db2, dw3, db3 = _mlp_tail_wgrad(g, p, f2(dr), f2(h2), f2(dh2), f2(h1), dev)
                (wz, wzt, kz), (wr, wrt, kr) = p["g1"]
                dwz, dwr, db1 = _f32((HID, kz), dev, True), _f32((HID, kr), dev, True), _f32((HID,), dev, True)
                ops.linear_add_bwd(f2(dh1), f2(h1), HID, ACT_LRELU, SLOPE, x=xchain, k_real=kz, dw=dwz, db=db1)
                dxr = _f32((M, wr.shape[1]), dev)
                ops.linear_add_bwd(f2(dh1), f2(h1), HID, ACT_LRELU, SLOPE, x=f2(xrow), k_real=kr, dw=dwr, w_bwd=wrt, dx=dxr)
                g_chain[6 * j:6 * j + 6] = [g.unpack_dw1([dwz, dwr]), db1, dw2, db2, dw3, db3]
                dxr = dxr.view(S, B, -1).transpose(0, 1)
                if j == 0:
                    dfeat[:, 1:] = dxr[:, :, :FEAT]
                    daction = dxr[:, :, FEAT:FEAT + A].contiguous()
                else:
                    daction = daction + dxr[:, :, :A]
        else:
            g_chain = [torch.zeros_like(q) for q in g1.layer_params() + g2.layer_params()]
        ctx.saved = None
        need = ctx.needs_input_grad
        return (dfeat if need[0] else None, daction if need[1] else None, None, None, None) + tuple(g_i1) + tuple(g_i2) + tuple(g_chain)


class _KlFn(torch.autograd.Function):
    """loss_kld = KL(posterior || prior).mean(0).sum() with the N(0, I) prior of t = 0 built in; value and gradients in one launch."""

    @staticmethod
    def forward(ctx, mu_p, std_p, mu_q, std_q, B, T):
        loss = _f32((1,), mu_p.device, True)
        keep = torch.is_grad_enabled() or any(ctx.needs_input_grad)
        ctx.shapes = (mu_p.shape, mu_q.shape)
        ctx.g = ops.gauss_kl(mu_p.reshape(B * T, -1), std_p.reshape(B * T, -1), mu_q, std_q, B, T, 1.0 / B, loss, want_grad=keep)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, go):
        go = go.reshape(1).float().contiguous()
        g, ctx.g = ctx.g, None
        sp, sq = ctx.shapes
        return tuple(ops.scale_(t, go).reshape(s) for t, s in zip(g, (sp, sp, sq, sq))) + (None, None)


class _RewardLlFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mu, std, reward, done, B):
        loss = _f32((1,), mu.device, True)
        keep = torch.is_grad_enabled() or any(ctx.needs_input_grad)
        ctx.g = ops.gauss_ll(mu, std, reward, done, 1.0 / B, loss, want_grad=keep)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, go):
        go = go.reshape(1).float().contiguous()
        (dmu, dstd), ctx.g = ctx.g, None
        return ops.scale_(dmu, go).reshape(-1, 1), ops.scale_(dstd, go).reshape(-1, 1), None, None, None


class _ImageLlFn(torch.autograd.Function):
    """loss_image on the decoder's NHWC output; the gradient is produced in that layout and dtype in the same pass."""

    @staticmethod
    def forward(ctx, y, target, sigma, B):
        loss = _f32((1,), y.device, True)
        keep = torch.is_grad_enabled() or any(ctx.needs_input_grad)
        ctx.g = ops.gauss_ll_image(y, target, 3, sigma, 1.0 / B, loss, want_grad=keep)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, go):
        g, ctx.g = ctx.g, None
        return ops.scale_(g, go.reshape(1).float().contiguous()), None, None, None


def create_feature_actions(feature_, action_):
    """fa(t) = (feat(1:t), a(1:t-1)) and fa(t+1), flattened per sample (slac/utils.py:7-18)."""
    N = feature_.size(0)
    f, n_f = feature_[:, :-1].reshape(N, -1), feature_[:, 1:].reshape(N, -1)
    a, n_a = action_[:, :-1].reshape(N, -1), action_[:, 1:].reshape(N, -1)
    return torch.cat([f, a], dim=-1), torch.cat([n_f, n_a], dim=-1)


class LatentModel(nn.Module):
    """SLAC's stochastic latent variable model (latent.py:174-311) on HIP: the call surface, state_dict keys and parameter
    aliasing (`z2_posterior_init` is `z2_prior_init`, `z2_posterior` is `z2_prior`) of the reference, so its `latent.pth`
    loads with strict=True and torch.optim.Adam(model.parameters()) trains it.  The Gaussian heads are fp32; `dtype` is
    the compute dtype of the two conv stacks.  `noise` ([B,S+1,288], the eps of z1(t) | z2(t)) makes a call reproducible."""

    def __init__(self, state_shape=(3, 100, 100), action_shape=(6,), feature_dim=256, z1_dim=32, z2_dim=256,
                 hidden_units=(256, 256), image_size=100, dtype=torch.float32, device="cuda:0"):
        super().__init__()
        if (image_size, feature_dim, z1_dim, z2_dim, tuple(hidden_units)) != (100, FEAT, Z1, Z2, (HID, HID)) or \
                tuple(state_shape) != (3, 100, 100):
            raise NotImplementedError("only image_size=100, feature_dim=256, z1_dim=32, z2_dim=256, hidden_units=(256, 256) is built")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("the SLAC latent model runs on a HIP device only (no CPU fallback)")
        A = self.action_dim = int(action_shape[0])
        self.z2_prior_init = Gaussian(Z1, Z2)                                              # p(z2(0) | z1(0))
        self.z1_prior = Gaussian(Z2 + A, Z1)                                               # p(z1(t+1) | z2(t), a(t))
        self.z2_prior = Gaussian(Z1 + Z2 + A, Z2, groups=[[(0, Z1 + Z2)], [(Z1 + Z2, Z1 + Z2 + A)]])
        self.z1_posterior_init = Gaussian(FEAT, Z1)                                        # q(z1(0) | feat(0))
        self.z2_posterior_init = self.z2_prior_init
        self.z1_posterior = Gaussian(FEAT + Z2 + A, Z1, groups=[[(FEAT, FEAT + Z2)], [(0, FEAT), (FEAT + Z2, FEAT + Z2 + A)]])
        self.z2_posterior = self.z2_prior
        self.reward = Gaussian(2 * (Z1 + Z2) + A, 1)                                       # p(r(t) | z(t), a(t), z(t+1))
        self.encoder = Encoder(state_shape[0], feature_dim, image_size, dtype=dtype, device=dev)
        self.decoder = Decoder(Z1 + Z2, state_shape[0], std=float(0.1 ** 0.5), image_size=image_size, dtype=dtype, device=dev)
        for st in (self.encoder, self.decoder):                                            # initialize_weight of the reference
            for i, p in enumerate(st.layer_params()):
                if i % 2 == 0:
                    nn.init.xavier_uniform_(p, gain=1.0)
        self.to(dev)
        self.chain_state_bytes = 0              # bytes the last sample_posterior kept for its backward (0 under no_grad)
        self.fused_chain = False                # True: a no-grad sample_posterior, predict and imagine run their chain as ONE launch (SPEC.md N3h-N3j)
        self.fused_chain_grad = False           # True: a grad-mode sample_posterior runs its chain as ONE launch forward, ONE backward (SPEC.md N3k)
        self.chain_compute = "fp32"             # "bf16": the fused no-grad chains of sample_posterior and predict multiply in bf16 (SPEC.md N3m; imagine: its `compute` keyword)
        self.chain_grad_compute = "fp32"        # "bf16": with fused_chain_grad, the chain's forward and backward launches multiply in bf16 (SPEC.md N3p)

    @property
    def device(self):
        return self.encoder.device

    def chain_form(self, keep):
        """How a posterior or prior chain that is about to run does its steps, from the three switches.  keep (backward state is
        wanted): "fused_save" with `fused_chain_grad`, else "layers".  Without: "layers" unless `fused_chain`; then "fused", or
        "fused_bf16" when the launch multiplies in bf16 (SPEC.md N3m).  `chain_compute` is read, and an unknown value is a ValueError,
        only there: with grad, on the per-layer path and in `imagine` the attribute changes nothing."""
        if keep:
            return "fused_save" if self.fused_chain_grad else "layers"
        if not self.fused_chain:
            return "layers"
        if self.chain_compute not in ("fp32", "bf16"):
            raise ValueError("chain_compute is 'fp32' or 'bf16', not %r" % (self.chain_compute,))
        return "fused_bf16" if self.chain_compute == "bf16" else "fused"

    def _chain_heads(self):
        return self.z1_posterior_init, self.z2_prior_init, self.z1_posterior, self.z2_prior

    def _chain_params(self):
        return sum((g.layer_params() for g in self._chain_heads()), [])

    def _posterior(self, features_, actions_, noise):
        dev = self.device
        features_ = features_.to(dev, torch.float32).contiguous()
        actions_ = actions_.to(dev, torch.float32).contiguous()
        B, T, _ = features_.shape
        if actions_.shape[:2] != (B, T - 1) or actions_.shape[2] != self.action_dim or features_.shape[2] != FEAT:
            raise ValueError("features_ [B,S+1,256] and actions_ [B,S,A] are needed")
        if noise is None:
            noise = torch.randn((B, T, Z1 + Z2), dtype=torch.float32, device=dev)
        noise = noise.to(dev, torch.float32).contiguous()
        if noise.shape != (B, T, Z1 + Z2):
            raise ValueError("noise is [B,S+1,z1_dim+z2_dim]")
        return _PosteriorFn.apply(features_, actions_, noise, self, torch.is_grad_enabled(), *self._chain_params())

    def sample_posterior(self, features_, actions_, noise=None):
        mean, std, z = self._posterior(features_, actions_, noise)
        return mean, std, z[..., :Z1], z[..., Z1:]

    def _prior(self, actions_, z2_post_):
        B, S, A = actions_.shape
        x = _f32((B, S, pad_to(Z2 + A, 4)), self.device, True)
        x = torch.cat([z2_post_[:, :S], actions_, x[..., Z2 + A:]], dim=-1).reshape(B * S, -1)
        return _GaussFn.apply(x, self.z1_prior, *self.z1_prior.layer_params())          # [B*S, 32] each

    def sample_prior(self, actions_, z2_post_):
        actions_ = actions_.to(self.device, torch.float32)
        B, S, _ = actions_.shape
        mean, std = self._prior(actions_, z2_post_)
        m0, s0 = _f32((B, 1, Z1), self.device, True), torch.ones((B, 1, Z1), dtype=torch.float32, device=self.device)
        return torch.cat([m0, mean.reshape(B, S, Z1)], dim=1), torch.cat([s0, std.reshape(B, S, Z1)], dim=1)

    def _rollout_start(self, z0, H, noise, sample):
        """What `predict` and `imagine` share before they diverge: z0 [B,288] and the noise [B,H,288] (None: drawn on the device;
        sample False: zeros) on the device, the outputs (mean, std [B,H,32], z [B,H,288]), and -- None for an empty batch -- the two
        heads z1_prior / z2_prior, their packs, their action columns wc / wb [256][pad4(A)], and xz [B,288] = z0."""
        dev, A = self.device, self.action_dim
        z0 = z0.to(dev, torch.float32)
        if z0.dim() != 2 or z0.shape[1] != Z1 + Z2 or H < 0:
            raise ValueError("z0 [B,z1_dim+z2_dim] and a horizon >= 0 are needed")
        B = z0.shape[0]
        if not sample:
            noise = _f32((B, H, Z1 + Z2), dev, True)
        elif noise is None:
            noise = torch.randn((B, H, Z1 + Z2), dtype=torch.float32, device=dev)
        noise = noise.to(dev, torch.float32).contiguous()
        if noise.shape != (B, H, Z1 + Z2):
            raise ValueError("noise is [B,H,z1_dim+z2_dim]")
        out = _f32((B, H, Z1), dev), _f32((B, H, Z1), dev), _f32((B, H, Z1 + Z2), dev)
        if B == 0 or H == 0:
            return noise, out, None
        g1, g2 = self.z1_prior, self.z2_prior
        p1, p2 = g1.packed(), g2.packed()
        # xz = z1(h) | z2(h-1), the input row of both first layers: the per-layer path writes it, the fused one reads z(0) from it
        xz = _f32((B, Z1 + Z2), dev).copy_(z0)
        return noise, out, (g1, g2, p1, p2, g1.packed_cols(Z2, Z2 + A), p2["g1"][1][0], xz)

    @torch.no_grad()
    def predict(self, z0, actions_, noise=None, sample=True):
        """Open-loop rollout of the generative model (SPEC.md N3i): z0 [B,288] = z1(0) | z2(0), actions_ [B,H,A] = a(0..H-1), noise
        [B,H,288] = the eps of z1(h) | z2(h) (None: drawn on the device; sample False: zeros, the mean rollout) ->
        (z1_mean [B,H,32], z1_std [B,H,32], z [B,H,288]) of the steps h = 1..H in the slots h - 1.  z1_prior and z2_prior are fed
        their own samples; z1(0) is not read.  Always without grad.  Both first layers are (chain columns + hoisted action term) +
        bias, so H = 1 equals sample_prior within rounding, not bitwise.  With `fused_chain` the H steps are one launch
        (s2p_prior_chain_fwd), else 8 per step; the two are bitwise equal.  `chain_compute == "bf16"` gives the fused launch bf16
        operands (SPEC.md N3m): mixed precision, not the same numbers."""
        actions_ = actions_.to(self.device, torch.float32).contiguous()
        if actions_.dim() != 3 or actions_.shape[:1] != z0.shape[:1] or actions_.shape[2] != self.action_dim:
            raise ValueError("z0 [B,z1_dim+z2_dim] and actions_ [B,H,A] are needed")
        B, H, A = actions_.shape
        noise, (mean, std, z), st = self._rollout_start(z0, H, noise, sample)
        if st is None:
            return mean, std, z
        g1, g2, p1, p2, wc, wb, xz = st
        rc, rb = _action_term(actions_, wc)[1], _action_term(actions_, wb)[1]
        form = self.chain_form(False)
        if form == "fused_bf16":
            ops.prior_chain_fwd_bf16(xz[:, Z1:], rc, rb, noise, [ops.chain_mlp_bf16(g1.packed_bf16(k1=Z2)),
                                                                 ops.chain_mlp_bf16(g2.packed_bf16())], mean, std, z)
            return mean, std, z
        if form == "fused":
            ops.prior_chain_fwd(xz[:, Z1:], rc, rb, noise, [ops.chain_mlp(p1, k1=Z2), ops.chain_mlp(p2)], mean, std, z)
            return mean, std, z
        h1, h2 = _f32((B, HID), self.device), _f32((B, HID), self.device)
        bufa, bufb = (h1, h2, _f32((B, g1.Npad), self.device)), (h1, h2, _f32((B, g2.Npad), self.device))
        for s in range(H):
            r = slice(s * B, (s + 1) * B)
            _chain_step(g1, p1, g2, p2, bufa, bufb, rc[r], rb[r], noise, mean, std, z, s, xz, xz)
        return mean, std, z

    @torch.no_grad()
    def imagine(self, policy, z0, horizon, noise=None, sample=True, compute="fp32"):
        """Closed-loop rollout (SPEC.md N3j): the deterministic policy tanh(mean) reads z(h) and the generative model steps on its
        action.  policy: a `TanhGaussianPolicy` with obs_dim 288 and two hidden layers; z0 [B,288] = z1(0) | z2(0) (z1(0) IS read);
        noise [B,H,288] as in `predict` -> (actions [B,H,A], z1_mean [B,H,32], z1_std [B,H,32], z [B,H,288]); slot h holds a(h) and
        z(h+1).  Always without grad.  With `fused_chain` the H steps are one launch (s2p_imagine_chain_fwd; ValueError for a policy
        outside its built shapes), else 13 per step; the two are bitwise equal, and `predict(z0, actions, noise)` returns bitwise
        this z1_mean, z1_std and z.  `compute`: "fp32" is all of the above whatever `chain_compute` says; "bf16" (SPEC.md N3n) runs the
        one launch with bf16 operands (s2p_imagine_chain_fwd_bf16): mixed precision, not the same numbers, and `predict` with
        `fused_chain` and `chain_compute == "bf16"` returns bitwise ITS z1_mean, z1_std and z.  The mode exists only in the fused
        kernel: without `fused_chain` it is a ValueError, as is any other value."""
        if compute not in ("fp32", "bf16"):
            raise ValueError("compute is 'fp32' or 'bf16', not %r" % (compute,))
        if compute == "bf16" and not self.fused_chain:
            raise ValueError("compute='bf16' needs fused_chain: the bf16 compute mode exists only in the fused imagination kernel")
        dev, A, H = self.device, self.action_dim, int(horizon)
        hs = getattr(policy, "hidden_sizes", None)
        if getattr(policy, "obs_dim", None) != Z1 + Z2 or getattr(policy, "action_dim", None) != A or hs is None or len(hs) != 2:
            raise ValueError("a TanhGaussianPolicy with obs_dim %d, action_dim %d and two hidden layers is needed" % (Z1 + Z2, A))
        if policy.device is None or policy.device.type != dev.type:
            raise ValueError("the policy and the latent model share a HIP device")
        noise, (mean, std, z), st = self._rollout_start(z0, H, noise, sample)
        B = z.shape[0]
        act = _f32((B, H, pad_to(A, 4)), dev, True)
        if st is None:
            return act[..., :A], mean, std, z
        g1, g2, p1, p2, wc, wb, xz = st
        if compute == "bf16":
            ops.imagine_chain_fwd_bf16(xz, noise, [ops.chain_mlp_bf16(g1.packed_bf16(k1=Z2)), ops.chain_mlp_bf16(g2.packed_bf16())], wc, wb,
                                       A, ops.policy_mlp_bf16(policy), act, mean, std, z)
            return act[..., :A], mean, std, z
        if self.fused_chain:
            ops.imagine_chain_fwd(xz, noise, [ops.chain_mlp(p1, k1=Z2), ops.chain_mlp(p2)], wc, wb, A, ops.policy_mlp(policy), act,
                                  mean, std, z)
            return act[..., :A], mean, std, z
        pk, fl = policy.packed, policy.flat
        pw, pb = [pk.w(fl, li) for li in range(3)], [pk.b(fl, li) for li in range(3)]
        q1, q2 = _f32((B, hs[0]), dev), _f32((B, hs[1]), dev)
        rc, rb = _f32((B, HID), dev), _f32((B, HID), dev)
        h1, h2 = _f32((B, HID), dev), _f32((B, HID), dev)
        bufa, bufb = (h1, h2, _f32((B, g1.Npad), dev)), (h1, h2, _f32((B, g2.Npad), dev))
        for s in range(H):
            a = act[:, s]                                                                # [B, pad4(A)] view, pitch H * pad4(A)
            ops.linear_fwd_into(xz, pw[0], pb[0], hs[0], q1, ACT_RELU)
            ops.linear_fwd_into(q1, pw[1], pb[1], hs[1], q2, ACT_RELU)
            ops.linear_fwd_into(q2, pw[2], pb[2], A, a, ACT_TANH)
            ops.linear_fwd_into(a, wc, None, HID, rc)
            ops.linear_fwd_into(a, wb, None, HID, rb)
            _chain_step(g1, p1, g2, p2, bufa, bufb, rc, rb, noise, mean, std, z, s, xz, xz)
        return act[..., :A], mean, std, z

    @staticmethod
    def feature_action_frames(obs_dim, action_dim):
        """S of a `feature_action` policy input: obs_dim = S 256 + (S - 1) A -> S = (obs_dim + A) / (256 + A); None where no integer
        S >= 2 fits."""
        S, rem = divmod(int(obs_dim) + int(action_dim), FEAT + int(action_dim))
        return S if rem == 0 and S >= 2 else None

    @torch.no_grad()
    def imagine_feature_action(self, policy, z0, window, horizon, noise=None, sample=True, quantize=True, final_obs=False,
                               keep_frames=False):
        """Closed-loop rollout of a `feature_action` policy (SPEC.md N3o): the policy reads the window of the last S encoder features
        and S - 1 actions, so every step decodes z(h+1), turns the decoded frame into the frame an environment would hand out
        (s2p_decoded_to_frames), encodes it and shifts it into the window.  policy: a `TanhGaussianPolicy` with two hidden layers and
        obs_dim = S 256 + (S - 1) A, S >= 2; window [B,obs_dim]: the policy-input row at the start, `SlacAlgorithm.preprocess`'s layout
        [f_0 .. f_{S-1} | a_0 .. a_{S-2}]; z0, noise, sample as in `imagine`.  Step h: a(h) = policy.act(window(h)); the prior step of
        the per-layer `imagine` path gives z(h+1); unless h = H - 1 and not `final_obs`, decoder -> hand-off -> encoder -> push give
        window(h+1).  `quantize`: the encoder sees the uint8 frame / 255 (what it was trained on; bitwise the replay buffer's gather of
        that frame); False: the decoded frame clamped to [0,1].  -> (actions [B,H,A], z1_mean, z1_std [B,H,32], z [B,H,288] as `imagine`
        returns them, obs [B,H (+1 with final_obs),obs_dim] the rows the policy read (the last one of `final_obs`: window(H)),
        frames_u8 [B,H-1 (+1 with final_obs),100,100,3] with `keep_frames`, else None: slot h is the frame behind window(h+1)).
        Always without grad; `fused_chain` and `chain_compute` are not read; the conv stacks run in the model's dtype."""
        dev, A, H = self.device, self.action_dim, int(horizon)
        hs = getattr(policy, "hidden_sizes", None)
        P = getattr(policy, "obs_dim", None)
        S = self.feature_action_frames(P, A) if P is not None else None
        if S is None or getattr(policy, "action_dim", None) != A or hs is None or len(hs) != 2:
            raise ValueError("a TanhGaussianPolicy with obs_dim S * %d + (S - 1) * %d for an integer S >= 2, action_dim %d and two hidden "
                             "layers is needed" % (FEAT, A, A))
        if policy.device is None or policy.device.type != dev.type:
            raise ValueError("the policy and the latent model share a HIP device")
        noise, (mean, std, z), st = self._rollout_start(z0, H, noise, sample)
        B = z.shape[0]
        window = torch.as_tensor(window).to(dev, torch.float32)
        if window.dim() != 2 or window.shape[1] != P or window.shape[0] != B:
            raise ValueError("window [B,%d], one policy-input row per row of z0, is needed" % P)
        if B > 65535:
            raise ValueError("at most 65535 rows (s2p_feature_action_push)")
        n_obs = H + 1 if final_obs else H
        n_fr = max(n_obs - 1, 0)
        act = _f32((B, H, pad_to(A, 4)), dev, True)
        obs = _f32((B, n_obs, P), dev)
        frames = torch.empty((n_fr, B, 100, 100, 3), dtype=torch.uint8, device=dev) if keep_frames else None
        if st is None:
            if n_obs and B:
                obs[:, 0] = window
            return act[..., :A], mean, std, z, obs, frames.transpose(0, 1) if keep_frames else None
        g1, g2, p1, p2, wc, wb, xz = st
        dt = self.decoder.dtype
        win = [_f32((B, pad_to(P, 4)), dev, True) for _ in range(2)]
        win[0][:, :P] = window
        rc, rb = _f32((B, HID), dev), _f32((B, HID), dev)
        h1, h2 = _f32((B, HID), dev), _f32((B, HID), dev)
        bufa, bufb = (h1, h2, _f32((B, g1.Npad), dev)), (h1, h2, _f32((B, g2.Npad), dev))
        zin = torch.empty((B, 1, 1, Z1 + Z2), dtype=dt, device=dev)
        xin = torch.empty((B, 100, 100, chunk_elems(dt)), dtype=dt, device=dev)
        for s in range(H):
            cur, nxt = win[s % 2], win[1 - s % 2]
            obs[:, s] = cur[:, :P]
            a = act[:, s]                                                                # [B, pad4(A)] view, pitch H * pad4(A)
            a[:, :A] = policy.act(cur[:, :P])
            ops.linear_fwd_into(a, wc, None, HID, rc)
            ops.linear_fwd_into(a, wb, None, HID, rb)
            _chain_step(g1, p1, g2, p2, bufa, bufb, rc, rb, noise, mean, std, z, s, xz, xz)
            if s == H - 1 and not final_obs:
                break
            zin.view(B, Z1 + Z2).copy_(z[:, s])
            y = self.decoder.run(zin)                                                    # [B,100,100,pitch]
            ops.decoded_to_frames(y, 3, quantize, x=xin, u8_out=frames[s] if keep_frames else None)
            f = self.encoder.run(xin).reshape(B, -1).float()
            ops.feature_action_push(cur, nxt, S, FEAT, A, f, a)
        if final_obs:
            obs[:, H] = win[H % 2][:, :P]
        return act[..., :A], mean, std, z, obs, frames.transpose(0, 1) if keep_frames else None

    def predict_reward(self, z0, z, actions_):
        """Reward head on [z(h-1) | a(h-1) | z(h)], h = 1..H, with z(0) = z0 [B,288], z [B,H,288] (predict's), actions_ [B,H,A] ->
        (mean [B,H], std [B,H])."""
        dev = self.device
        z0, z = z0.to(dev, torch.float32), z.to(dev, torch.float32)
        actions_ = actions_.to(dev, torch.float32)
        B, H, A = actions_.shape
        if z0.shape != (B, Z1 + Z2) or z.shape != (B, H, Z1 + Z2) or A != self.action_dim:
            raise ValueError("z0 [B,z1_dim+z2_dim], z [B,H,z1_dim+z2_dim] and actions_ [B,H,A] are needed")
        k = 2 * (Z1 + Z2) + A
        pad = _f32((B, H, pad_to(k, 4) - k), dev, True)
        x = torch.cat([torch.cat([z0[:, None], z[:, :-1]], dim=1), actions_, z, pad], dim=-1).reshape(B * H, -1)
        mean, std = _GaussFn.apply(x, self.reward, *self.reward.layer_params())
        return mean.reshape(B, H), std.reshape(B, H)

    def calculate_loss(self, state_, action_, reward_, done_, noise=None):
        dev = self.device
        B, T = state_.shape[:2]
        S = T - 1
        action_ = action_.to(dev, torch.float32).contiguous()
        reward_ = reward_.to(dev, torch.float32).reshape(B * S).contiguous()
        done_ = done_.to(dev, torch.float32).reshape(B * S).contiguous()
        feature_ = self.encoder(state_)
        if isinstance(state_, FrameBatch):
            state_ = state_.u8                                         # the image loss reads uint8 NHWC targets
        z1_mean_post_, z1_std_post_, z_ = self._posterior(feature_, action_, noise)
        z1_mean_pri_, z1_std_pri_ = self._prior(action_, z_[..., Z1:])
        loss_kld = _KlFn.apply(z1_mean_post_, z1_std_post_, z1_mean_pri_, z1_std_pri_, B, T)
        # image term: straight on the decoder's NHWC output, target at full precision
        y = self.decoder.run(z_.reshape(B * T, 1, 1, Z1 + Z2).to(self.decoder.dtype).contiguous())
        if state_.dtype == torch.uint8:
            target = state_.reshape(B * T, *state_.shape[2:]).to(dev).contiguous()
        else:
            target = state_.reshape(B * T, *state_.shape[2:]).to(dev, torch.float32).contiguous()
        loss_image = _ImageLlFn.apply(y, target, self.decoder.std, B)
        # reward term
        pad = _f32((B, S, pad_to(2 * (Z1 + Z2) + self.action_dim, 4) - 2 * (Z1 + Z2) - self.action_dim), dev, True)
        x = torch.cat([z_[:, :-1], action_, z_[:, 1:], pad], dim=-1).reshape(B * S, -1)
        r_mean, r_std = _GaussFn.apply(x, self.reward, *self.reward.layer_params())
        loss_reward = _RewardLlFn.apply(r_mean, r_std, reward_, done_, B)
        return loss_kld, loss_image, loss_reward

    def save_model(self, save_dir):
        """encoder.pth and latent.pth with the reference's keys (slac/algo.py:145-150)."""
        import os
        os.makedirs(save_dir, exist_ok=True)
        torch.save(self.encoder.state_dict(), os.path.join(save_dir, "encoder.pth"))
        torch.save(self.state_dict(), os.path.join(save_dir, "latent.pth"))
