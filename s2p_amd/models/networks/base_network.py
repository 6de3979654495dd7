"""BaseNetwork: SPADE-lineage network base class (plugin contract of `--netG/--netD`):
`modify_commandline_options(parser, is_train)` static hook, `cls(opt)` constructor, `init_weights(init_type,
init_variance)`, `print_network()`.  Adds the MI355X flat parameter store hooks, and the optional spectral normalization
(SPEC.md D5s) of chosen conv weights with torch.nn.utils.spectral_norm's checkpoint names."""
import math

import torch
import torch.nn as nn

from ...params import ParamStore

SN_EPS = 1e-12


def sn_buffers(conv):
    """Give the conv module torch.nn.utils.spectral_norm's buffers: `weight_u` [Cout] and `weight_v` [kh*kw*Cin], both
    normalize(randn) as torch initialises them.  v is kept in the flat master's column order (tap, channel); checkpoints
    carry it in torch's (channel, tap) order (BaseNetwork.export_state_dict)."""
    w = conv.weight
    u, v = torch.randn(w.shape[0]), torch.randn(w.numel() // w.shape[0])
    conv.register_buffer("weight_u", u / u.norm().clamp_min(SN_EPS))
    conv.register_buffer("weight_v", v / v.norm().clamp_min(SN_EPS))


class BaseNetwork(nn.Module):
    def __init__(self):
        super().__init__()
        self.store = ParamStore()
        self.compute_dtype = torch.float32
        self.finalized = False
        self.sn_option = None          # the option value that turns spectral norm on for this network (error messages)

    @staticmethod
    def modify_commandline_options(parser, is_train):
        return parser

    def print_network(self):
        n = sum(p.numel() for p in self.parameters())
        print("Network [%s] was created. Total number of parameters: %.1f million."
              % (type(self).__name__, n / 1e6))

    def init_weights(self, init_type="xavier", gain=0.02):
        """SPADE convention: xavier-normal(gain) on conv / linear weights, zero biases."""
        with torch.no_grad():
            for name, p in self.named_parameters():
                if name.endswith(".bias"):
                    p.zero_()
                    continue
                if p.dim() < 2:
                    continue
                tmp = torch.empty(p.shape, dtype=torch.float32)
                if init_type == "normal":
                    nn.init.normal_(tmp, 0.0, gain)
                elif init_type == "xavier":
                    nn.init.xavier_normal_(tmp, gain=gain)
                elif init_type == "xavier_uniform":
                    nn.init.xavier_uniform_(tmp, gain=1.0)
                elif init_type == "kaiming":
                    nn.init.kaiming_normal_(tmp, a=0, mode="fan_in")
                elif init_type == "orthogonal":
                    nn.init.orthogonal_(tmp, gain=gain)
                elif init_type == "none":
                    continue
                else:
                    raise NotImplementedError("initialization method [%s] is not implemented" % init_type)
                p.copy_(tmp)
        if self.finalized:
            self.store.repack()

    # ---- MI355X hooks --------------------------------------------------------------------------------
    def finalize(self, device, compute_dtype):
        """Move the parameters into the flat HBM store on `device` and build the packed compute-dtype operands.
        Must be called once, after construction / weight loading, before forward."""
        if device.type != "cuda":
            raise RuntimeError("the S2P hot path runs on a HIP device only (no CPU fallback); got device %s" % device)
        self.compute_dtype = compute_dtype
        self._declare_packs(compute_dtype)
        self.store.finalize(device)
        self.store.param_names = {id(p): n for n, p in self.named_parameters()}     # part of the checkpointed layout signature
        self.finalized = True
        return self

    def _declare_packs(self, compute_dtype):
        raise NotImplementedError

    def load_state_dict(self, state_dict, strict=True):
        out = super().load_state_dict(self._sn_from_torch(state_dict), strict=strict)
        if self.finalized:
            self.store.repack()
        return out

    def export_state_dict(self):
        """state_dict with plain contiguous CPU tensors (torch-layout), independent of the flat store.  A spectrally normalized
        layer is saved under torch.nn.utils.spectral_norm's names (`weight_orig`, `weight_u`, `weight_v`, v in torch's column
        order), so a torch module wrapped in spectral_norm loads the file as it is."""
        sd = {k: v.detach().cpu().contiguous().clone() for k, v in self.state_dict().items()}
        for name, m in self.sn_layers():
            w = sd.pop(name + ".weight")
            cout, cin, kh, kw = w.shape
            sd[name + ".weight_orig"] = w
            sd[name + ".weight_v"] = sd[name + ".weight_v"].view(kh, kw, cin).permute(2, 0, 1).reshape(-1).clone()
        return sd

    # ---- spectral normalization (SPEC.md D5s) -------------------------------------------------------------------
    def sn_layers(self):
        """(qualified name, module) of every spectrally normalized conv, in declaration order."""
        return [(n, m) for n, m in self.named_modules() if "weight_u" in m._buffers]

    def sn_forward(self):
        """Called once per forward of the network: in training mode one power iteration, in eval mode sigma from the stored
        u, v when the weights changed since the last refresh (after a load or an optimizer step).  No-op without SN layers."""
        st = self.store
        if st.sn and (self.training or st.sn_stale):
            st.sn_refresh(self.training)

    def _sn_from_torch(self, sd):
        """torch.nn.utils.spectral_norm names -> this module's (`weight_orig` -> `weight`, v back to the master's order); a
        checkpoint whose spectral-norm layers do not match this network's options is refused."""
        layers = self.sn_layers()
        orig = sorted(k[:-len(".weight_orig")] for k in sd if k.endswith(".weight_orig"))
        what = type(self).__name__
        if not layers:
            if orig:
                raise RuntimeError("the state dict holds spectrally normalized layers (%s.weight_orig, ...) but this %s was built "
                                   "without spectral norm: pass %s" % (orig[0], what, self.sn_option))
            return sd
        sd = dict(sd)
        for name, m in layers:
            if name + ".weight_orig" not in sd:
                raise RuntimeError("the state dict has no %s.weight_orig: it was written without spectral norm, but this %s was "
                                   "built with %s; load it without that option" % (name, what, self.sn_option))
            w = sd.pop(name + ".weight_orig")
            sd[name + ".weight"] = w
            if name + ".weight_v" in sd:
                cout, cin, kh, kw = w.shape
                sd[name + ".weight_v"] = sd[name + ".weight_v"].reshape(cin, kh, kw).permute(1, 2, 0).reshape(-1)
        return sd

    def _require_ready(self):
        if not self.finalized:
            raise RuntimeError(f"{type(self).__name__}: call .finalize(device, dtype) before forward "
                               "(the HIP path has no CPU fallback)")
