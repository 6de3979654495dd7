"""IQL on SLAC latents (SPEC.md N3d; reference `rlkit/torch/sac/iql_trainer.py:209-435`, networks of
`examples/iql/custom_networks.py` and `rlkit/torch/sac/policies/gaussian_policy.py:76-154`): the consumer loop the replay buffer and
the latent model feed.  `Qfunction` / `Vfunction` / `TanhGaussianPolicy` carry the reference's constructor arguments, its init and
its `state_dict` keys; `CriticSLAC` owns qf1 | qf2 | vf in ONE flat fp32 buffer (beside flat gradient and Adam-moment buffers of
the same layout) and target_qf1 | target_qf2 in a second one of the layout of qf1 | qf2, so an optimizer step is one
s2p_adam_step_dev launch and the Polyak update one s2p_soft_update launch.  A train step runs the six networks as groups of one
grouped launch per layer (csrc/iql.hip); DESIGN.md section 6b.4 counts the launches.  No CPU fallback."""
import ctypes
import math
from collections import OrderedDict

import torch

from ._lib import ACT_NONE, ACT_RELU, MlpBwdGroup, MlpFwdGroup, check, lib, ptr, stream
from .ops import pad_to

LOG_SIG_MAX, LOG_SIG_MIN = 2.0, -20.0


def fanin_init(w):
    """rlkit's `fanin_init` (pytorch_util.py:139-148): the bound comes from size[0], which is the OUT width of an nn.Linear weight."""
    bound = 1.0 / math.sqrt(w.shape[0])
    return w.uniform_(-bound, bound)


class Mlp:
    """A ReLU MLP's shape, init and `state_dict` (rlkit/torch/networks/mlp.py:14-71), held on the CPU until a `CriticSLAC` or a
    policy moves it into its flat device buffer."""
    heads = ("last_fc",)

    def __init__(self, hidden_sizes, output_size, input_size, init_w=3e-3, b_init_value=0.0):
        self.hidden_sizes, self.output_size, self.input_size = [int(h) for h in hidden_sizes], int(output_size), int(input_size)
        if not self.hidden_sizes or any(h % 4 or h <= 16 for h in self.hidden_sizes):
            raise ValueError("hidden_sizes: at least one layer, widths multiples of 4 above 16 (the MFMA tile path)")
        sd, n_in = OrderedDict(), self.input_size
        for i, h in enumerate(self.hidden_sizes):
            sd["fc%d.weight" % i] = fanin_init(torch.empty(h, n_in))
            sd["fc%d.bias" % i] = torch.full((h,), float(b_init_value))
            n_in = h
        sd["last_fc.weight"] = torch.empty(self.output_size, n_in).uniform_(-init_w, init_w)
        sd["last_fc.bias"] = torch.zeros(self.output_size)
        self._sd = sd

    def dims(self):
        """[(in, out)] of the packed layers: the hidden ones, then ALL heads as one layer."""
        ins = [self.input_size] + self.hidden_sizes
        return list(zip(ins, self.hidden_sizes + [self.output_size * len(self.heads)]))

    def names(self):
        return ["fc%d" % i for i in range(len(self.hidden_sizes))] + list(self.heads)

    def state_dict(self):
        return OrderedDict((k, v.clone()) for k, v in self._sd.items())


class Qfunction(Mlp):
    """Q(cat(z, action)) (custom_networks.py:21-34, without an encoder)."""


class Vfunction(Mlp):
    """V(z) (custom_networks.py:36-50, without an encoder)."""


class _Packed:
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


def _load(net, packed, flat, sd, prefix=""):
    """A reference-layout state_dict -> the packed layers; several heads (`last_fc`, `last_fc_log_std`) are rows of ONE layer."""
    names, nh = net.names(), len(net.heads)
    for li, name in enumerate(names[:len(names) - nh]):
        w, b = torch.as_tensor(sd[prefix + name + ".weight"]), torch.as_tensor(sd[prefix + name + ".bias"])
        if tuple(w.shape) != (net.dims()[li][1], net.dims()[li][0]) or tuple(b.shape) != (w.shape[0],):
            raise RuntimeError("size mismatch for %s%s" % (prefix, name))
        packed.put(flat, li, w, b)
    w = torch.cat([torch.as_tensor(sd[prefix + h + ".weight"]) for h in net.heads])
    b = torch.cat([torch.as_tensor(sd[prefix + h + ".bias"]) for h in net.heads])
    li = len(names) - nh
    if tuple(w.shape) != (net.dims()[li][1], net.dims()[li][0]):
        raise RuntimeError("size mismatch for %s%s" % (prefix, net.heads[0]))
    packed.put(flat, li, w, b)


def _export(net, packed, flat, prefix=""):
    out, names, nh = OrderedDict(), net.names(), len(net.heads)
    for li, name in enumerate(names[:len(names) - nh]):
        out[prefix + name + ".weight"], out[prefix + name + ".bias"] = packed.get(flat, li)
    w, b = packed.get(flat, len(names) - nh)
    for i, h in enumerate(net.heads):
        n = net.output_size
        out[prefix + h + ".weight"], out[prefix + h + ".bias"] = w[i * n:(i + 1) * n].clone(), b[i * n:(i + 1) * n].clone()
    return out


def _strict(sd, keys, strict):
    if strict and list(sorted(sd.keys())) != sorted(keys):
        raise RuntimeError("state_dict keys differ: missing %s, unexpected %s" % (sorted(set(keys) - set(sd)), sorted(set(sd) - set(keys))))


def _device(device):
    if device is None:                  # a shape / init / state_dict holder on the CPU: nothing of it can run
        return None
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("the IQL networks (HIP) need a HIP device: there is no CPU fallback")
    return device


class CriticSLAC:
    """qf1, qf2, target_qf1, target_qf2 and vf (custom_networks.py:100-120), `state_dict` keys `qf1.fc0.weight` ... in that order."""
    NETS = ("qf1", "qf2", "target_qf1", "target_qf2", "vf")

    def __init__(self, qf1, qf2, target_qf1, target_qf2, vf=None, device="cuda:0"):
        self.device = _device(device)
        self.nets = OrderedDict(zip(self.NETS, (qf1, qf2, target_qf1, target_qf2, vf)))
        if vf is None or any(n.dims() != qf1.dims() for n in (qf2, target_qf1, target_qf2)) or vf.hidden_sizes != qf1.hidden_sizes:
            raise ValueError("CriticSLAC: four Q networks of one shape and a vf of the same hidden sizes")
        self.packed = {"qf1": _Packed(qf1.dims())}
        self.packed["qf2"] = _Packed(qf2.dims(), self.packed["qf1"].end)
        self.packed["vf"] = _Packed(vf.dims(), self.packed["qf2"].end)
        self.packed["target_qf1"], self.packed["target_qf2"] = self.packed["qf1"], self.packed["qf2"]
        self.n_target, self.n = self.packed["qf2"].end, self.packed["vf"].end
        if self.device is None:
            return
        self.flat = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        self.target_flat = torch.zeros(self.n_target, dtype=torch.float32, device=self.device)
        self.grad = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        sd = OrderedDict()
        for name, net in self.nets.items():
            sd.update((name + "." + k, v) for k, v in net.state_dict().items())
        self.load_state_dict(sd)

    def flat_of(self, name):
        return self.target_flat if name.startswith("target") else self.flat

    def keys(self):
        return [name + "." + layer + "." + p for name, net in self.nets.items() for layer in net.names() for p in ("weight", "bias")]

    def load_state_dict(self, sd, strict=True):
        _strict(sd, self.keys(), strict)
        for name, net in self.nets.items():
            _load(net, self.packed[name], self.flat_of(name), sd, name + ".")
        return self

    def state_dict(self):
        out = OrderedDict()
        if self.device is None:
            for name, net in self.nets.items():
                out.update((name + "." + k, v) for k, v in net.state_dict().items())
            return out
        for name, net in self.nets.items():
            out.update(_export(net, self.packed[name], self.flat_of(name), name + "."))
        return out

    def grads(self):
        """Reference name -> gradient of the last step's critic loss (qf1, qf2, vf: the targets have none)."""
        out = OrderedDict()
        for name in ("qf1", "qf2", "vf"):
            out.update(_export(self.nets[name], self.packed[name], self.grad, name + "."))
        return out


class TanhGaussianPolicy(Mlp):
    """gaussian_policy.py:76-154 with `std=None`: the MLP trunk, then `last_fc` (mean) and `last_fc_log_std`, kept as the rows
    [0, A) and [A, 2A) of ONE packed last layer so both heads are one launch."""
    heads = ("last_fc", "last_fc_log_std")

    def __init__(self, hidden_sizes, obs_dim, action_dim, std=None, init_w=1e-3, device="cuda:0", **kwargs):
        if std is not None:
            raise NotImplementedError("a fixed std")
        super().__init__(hidden_sizes, output_size=action_dim, input_size=obs_dim, init_w=init_w, **kwargs)
        self.obs_dim, self.action_dim, self.device = int(obs_dim), int(action_dim), _device(device)
        if 2 * self.action_dim > 16:
            raise ValueError("action_dim <= 8 (the narrow last-layer kernel)")
        h = self.hidden_sizes[-1]
        self._sd["last_fc_log_std.weight"] = torch.empty(self.action_dim, h).uniform_(-init_w, init_w)
        self._sd["last_fc_log_std.bias"] = torch.empty(self.action_dim).uniform_(-init_w, init_w)
        self.packed = _Packed(self.dims())
        self.n = self.packed.end
        if self.device is None:
            return
        self.flat = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        self.grad = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        sd, self._sd = self._sd, None
        self.load_state_dict(sd)
        self._eval = {}

    def keys(self):
        return [layer + "." + p for layer in self.names() for p in ("weight", "bias")]

    def load_state_dict(self, sd, strict=True):
        _strict(sd, self.keys(), strict)
        _load(self, self.packed, self.flat, sd)
        return self

    def state_dict(self):
        return Mlp.state_dict(self) if self.device is None else _export(self, self.packed, self.flat)

    def grads(self):
        return _export(self, self.packed, self.grad)

    @torch.no_grad()
    def act(self, policy_input):
        """tanh(mean): the reference's `MakeDeterministic`.  Forward only: each layer's output overwrites one of two scratch
        buffers, no activation is kept."""
        x = policy_input.to(self.device, torch.float32)
        B, dims = x.shape[0], self.dims()
        if B not in self._eval:
            xp = torch.zeros(B, self.packed.off[0][2], dtype=torch.float32, device=self.device)
            hs = [torch.empty(B, max(self.hidden_sizes), dtype=torch.float32, device=self.device) for _ in range(2)]
            self._eval = {B: (xp, hs, torch.empty(B, 2 * self.action_dim, dtype=torch.float32, device=self.device))}
        xp, hs, raw = self._eval[B]
        xp[:, :self.obs_dim] = x
        h, hp = xp, xp.shape[1]
        for li, (cin, cout) in enumerate(dims):
            last = li == len(dims) - 1
            y = raw if last else hs[li % 2]
            g = MlpFwdGroup(ptr(h), ptr(self.packed.w(self.flat, li)), ptr(self.packed.b(self.flat, li)), ptr(y) if last else None,
                            None if last else ptr(y), hp, y.shape[1], B, self.packed.off[li][2])
            check(lib().s2p_mlp_linear_fwd(ctypes.byref(g), 1, cout, ACT_NONE if last else ACT_RELU, stream()), "s2p_mlp_linear_fwd")
            h, hp = y, y.shape[1]
        return torch.tanh(raw[:, :self.action_dim])


class _Adam:
    """torch.optim.Adam without weight decay over one flat buffer: one s2p_adam_step_dev launch."""

    def __init__(self, flat, grad, lr, betas=(0.9, 0.999), eps=1e-8):
        self.flat, self.grad, self.lr, self.betas, self.eps = flat, grad, float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.m, self.v = torch.zeros_like(flat), torch.zeros_like(flat)
        self.t = torch.zeros(1, dtype=torch.int32, device=flat.device)

    def step(self):
        check(lib().s2p_adam_step_dev(ptr(self.flat), ptr(self.grad), ptr(self.m), ptr(self.v), self.flat.numel(), self.lr,
                                      self.betas[0], self.betas[1], self.eps, ptr(self.t), 1.0, stream()), "s2p_adam_step_dev")

    def state_dict(self, tensors, all_names):
        """torch.optim.Adam's format; `tensors(flat)` -> name -> tensor in the reference layout, `all_names` the optimizer's
        parameter order (the critic's includes the targets, which never get a state)."""
        t = int(self.t.item())
        state = {}
        if t:
            m, v = tensors(self.m), tensors(self.v)
            for i, k in enumerate(all_names):
                if k in m:
                    state[i] = {"step": torch.tensor(float(t)), "exp_avg": m[k], "exp_avg_sq": v[k]}
        group = dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=0, amsgrad=False, params=list(range(len(all_names))))
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd, put, all_names):
        steps = {int(s["step"]) for s in sd["state"].values()}
        if len(steps) > 1:
            raise ValueError("one step count per optimizer")
        self.m.zero_(); self.v.zero_()
        self.t.fill_(steps.pop() if steps else 0)
        put(self.m, {all_names[int(i)]: s["exp_avg"] for i, s in sd["state"].items()})
        put(self.v, {all_names[int(i)]: s["exp_avg_sq"] for i, s in sd["state"].items()})
        g = sd["param_groups"][0]
        self.lr, self.betas, self.eps = float(g["lr"]), (float(g["betas"][0]), float(g["betas"][1])), float(g["eps"])


def target_update_due(n_train_steps, target_update_period):
    """iql_trainer.py:361: the Polyak update runs on the steps, counted from 0, that the period divides."""
    return n_train_steps % target_update_period == 0


class IQLTrainer:
    """`IQLTrainer` of the reference in its SLAC configuration (`image_rl`, `slac_representation`, the integrated critic
    optimizer), the arguments it uses under their reference names.  Not built: see SPEC.md N3d."""

    def __init__(self, env, policy, qf1=None, qf2=None, vf=None, quantile=0.5, target_qf1=None, target_qf2=None, discount=0.99,
                 reward_scale=1.0, policy_lr=1e-3, qf_lr=1e-3, policy_weight_decay=0, q_weight_decay=0, policy_update_period=1,
                 q_update_period=1, clip_score=None, soft_target_tau=1e-2, target_update_period=1, beta=1.0, critic=None,
                 slac_algo=None, freeze_slac=False, slac_update_period=1, slac_policy_input_type="feature_action"):
        if policy_weight_decay or q_weight_decay or policy_update_period != 1 or q_update_period != 1:
            raise NotImplementedError("weight decay and update periods other than 1")
        if slac_policy_input_type not in ("feature_action", "latent_z"):
            raise ValueError("slac_policy_input_type %r" % (slac_policy_input_type,))
        self.env, self.policy = env, policy
        self.critic = critic if critic is not None else CriticSLAC(qf1, qf2, target_qf1, target_qf2, vf, device=policy.device)
        if self.critic.nets["vf"].hidden_sizes != policy.hidden_sizes or self.critic.device != policy.device:
            raise ValueError("the policy and the critic share the hidden sizes (one grouped launch per layer) and the device")
        self.qf1, self.qf2, self.target_qf1, self.target_qf2, self.vf = (self.critic.nets[n] for n in CriticSLAC.NETS)
        self.device = policy.device
        self.quantile, self.discount, self.reward_scale, self.beta = float(quantile), float(discount), float(reward_scale), float(beta)
        self.clip_score = clip_score
        self.soft_target_tau, self.target_update_period = float(soft_target_tau), int(target_update_period)
        self.slac_algo, self.freeze_slac, self.slac_update_period = slac_algo, bool(freeze_slac), int(slac_update_period)
        self.slac_policy_input_type = slac_policy_input_type
        self.critic_optimizer = _Adam(self.critic.flat, self.critic.grad, qf_lr)
        self.policy_optimizer = _Adam(policy.flat, policy.grad, policy_lr)
        self.eval_statistics = OrderedDict()
        self._n_train_steps_total = 0
        self._need_to_update_eval_statistics = True
        self._buf = {}
        self.obs_dim, self.action_dim = self.vf.input_size, policy.action_dim
        if self.qf1.input_size != self.obs_dim + self.action_dim or self.qf1.output_size != 1 or self.vf.output_size != 1:
            raise ValueError("qf: (Z + A) -> 1, vf: Z -> 1")

    # ---- the grouped launches of a step: buffers and group tables per batch size, built once ---------------------------------
    def _tables(self, B):
        if B in self._buf:
            return self._buf[B]
        cr, po, dev, f = self.critic, self.policy, self.device, torch.float32
        Z, A, hid = self.obs_dim, self.action_dim, self.vf.hidden_sizes
        nets = [(n, cr.packed[n], cr.flat_of(n), cr.grad, B) for n in ("qf1", "qf2", "target_qf1", "target_qf2")]
        nets += [("vf", cr.packed["vf"], cr.flat, cr.grad, 2 * B), ("policy", po.packed, po.flat, po.grad, B)]
        t = dict(xq=torch.zeros(B, pad_to(Z + A, 4), dtype=f, device=dev), xv=torch.zeros(2 * B, pad_to(Z, 4), dtype=f, device=dev),
                 xp=torch.zeros(B, po.packed.off[0][2], dtype=f, device=dev),
                 q=torch.empty(4, B, dtype=f, device=dev), v=torch.empty(2 * B, dtype=f, device=dev),
                 raw=torch.empty(B, 2 * A, dtype=f, device=dev), dq=torch.empty(2, B, dtype=f, device=dev),
                 dv=torch.empty(B, dtype=f, device=dev), draw=torch.empty(B, 2 * A, dtype=f, device=dev),
                 weights=torch.empty(B, dtype=f, device=dev), adv=torch.empty(B, dtype=f, device=dev),
                 q_target=torch.empty(B, dtype=f, device=dev), losses=torch.zeros(4, dtype=f, device=dev),
                 reward=torch.empty(B, dtype=f, device=dev), terminal=torch.empty(B, dtype=f, device=dev),
                 action=torch.empty(B, A, dtype=f, device=dev))
        xin = {"vf": t["xv"], "policy": t["xp"]}
        act = {n: [torch.empty(rows, h, dtype=f, device=dev) for h in hid] for n, _, _, _, rows in nets}
        dact = {n: [torch.empty(B, h, dtype=f, device=dev) for h in hid] for n in ("qf1", "qf2", "vf", "policy")}
        t["act"], t["dact"] = act, dact
        out = {"qf1": t["q"][0], "qf2": t["q"][1], "target_qf1": t["q"][2], "target_qf2": t["q"][3], "vf": t["v"], "policy": t["raw"]}
        dout = {"qf1": t["dq"][0], "qf2": t["dq"][1], "vf": t["dv"], "policy": t["draw"]}
        L = len(hid)

        def width(li, sel):                     # the groups of a launch share N
            ws = {x[1].dims[li][1] for x in nets if x[0] in sel}
            assert len(ws) == 1
            return ws.pop()

        def fwd(li, sel):
            gs = []
            for n, pk, flat, _, rows in (x for x in nets if x[0] in sel):
                x = xin.get(n, t["xq"]) if li == 0 else act[n][li - 1]
                last = li == L
                y = out[n] if last else act[n][li]
                yp = (y.shape[1] if y.dim() == 2 else 1)
                gs.append(MlpFwdGroup(ptr(x), ptr(pk.w(flat, li)), ptr(pk.b(flat, li)), ptr(y) if last else None,
                                      None if last else ptr(y), x.shape[1], yp, rows, pk.off[li][2]))
            return (MlpFwdGroup * len(gs))(*gs), len(gs), width(li, sel)

        def bwd(li, sel):
            gs = []
            for n, pk, flat, grad, _ in (x for x in nets if x[0] in sel):
                x = xin.get(n, t["xq"]) if li == 0 else act[n][li - 1]
                d = dout[n] if li == L else dact[n][li]
                dp = d.shape[1] if d.dim() == 2 else 1
                prev = dact[n][li - 1] if li else None
                gs.append(MlpBwdGroup(ptr(x), ptr(d), ptr(pk.w(flat, li)), ptr(pk.w(grad, li)), ptr(pk.b(grad, li)),
                                      ptr(x) if li else None, ptr(prev), x.shape[1], dp, prev.shape[1] if li else 0, B, pk.off[li][2]))
            return (MlpBwdGroup * len(gs))(*gs), len(gs), width(li, sel)

        every, critics, trained = [n[0] for n in nets], [n[0] for n in nets[:5]], ["qf1", "qf2", "vf", "policy"]
        t["fwd"] = [fwd(li, every) for li in range(L)] + [fwd(L, critics), fwd(L, ["policy"])]
        t["fwd_act"] = [ACT_RELU] * L + [ACT_NONE, ACT_NONE]
        t["bwd"] = [bwd(L, ["qf1", "qf2", "vf"]), bwd(L, ["policy"])] + [bwd(li, trained) for li in range(L - 1, -1, -1)]
        self._buf = {B: t}                      # (one batch size is kept: a new one replaces the tables and their buffers)
        return t

    def _forward_backward(self, z, next_z, action, policy_input, rewards, terminals):
        """Every launch of a step up to the gradients; returns the tables (losses = [qf1, qf2, vf, policy])."""
        B, Z, A, dev, f = z.shape[0], self.obs_dim, self.action_dim, self.device, torch.float32
        t, L = self._tables(B), lib()
        t["xq"][:, :Z] = z.to(dev, f)
        t["xq"][:, Z:Z + A] = action.to(dev, f)
        t["xv"][:B, :Z] = t["xq"][:, :Z]
        t["xv"][B:, :Z] = next_z.to(dev, f)
        t["xp"][:, :self.policy.obs_dim] = policy_input.to(dev, f)
        t["action"].copy_(action.to(dev, f))
        t["reward"].copy_(rewards.to(dev, f).reshape(B))
        t["terminal"].copy_(terminals.to(dev, f).reshape(B))
        st = stream()
        for (gs, G, N), a in zip(t["fwd"], t["fwd_act"]):
            check(L.s2p_mlp_linear_fwd(gs, G, N, a, st), "s2p_mlp_linear_fwd")
        clip = float("inf") if self.clip_score is None else float(self.clip_score)
        q, v = t["q"], t["v"]
        check(L.s2p_iql_critic_head(ptr(q[0]), ptr(q[1]), ptr(q[2]), ptr(q[3]), ptr(v[:B]), ptr(v[B:]), ptr(t["reward"]),
                                    ptr(t["terminal"]), B, self.reward_scale, self.discount, self.quantile, self.beta, clip,
                                    ptr(t["losses"]), ptr(t["dq"][0]), ptr(t["dq"][1]), ptr(t["dv"]), ptr(t["weights"]), ptr(t["adv"]),
                                    ptr(t["q_target"]), st), "s2p_iql_critic_head")
        check(L.s2p_tanh_gauss_policy_head(ptr(t["raw"]), 2 * A, ptr(t["action"]), A, ptr(t["weights"]), B, A, ptr(t["losses"][3:]),
                                           ptr(t["draw"]), 2 * A, None, st), "s2p_tanh_gauss_policy_head")
        for i, (gs, G, N) in enumerate(t["bwd"]):
            check(L.s2p_mlp_linear_bwd(gs, G, N, ACT_RELU if i < len(t["bwd"]) - 1 else ACT_NONE, st), "s2p_mlp_linear_bwd")
        return t

    @torch.no_grad()
    def train_from_latents(self, z, next_z, action, policy_input, rewards, terminals, _latent=False):
        """One IQL step on given latents: z, next_z [B, Z], action [B, A], policy_input [B, P], rewards / terminals [B] or [B, 1]."""
        t = self._forward_backward(z, next_z, action, policy_input, rewards, terminals)
        self.critic_optimizer.step()
        self.policy_optimizer.step()
        if _latent and not self.freeze_slac and self._n_train_steps_total % self.slac_update_period == 0:
            with torch.enable_grad():
                self._latent_losses = self.slac_algo.update_latent(writer=None)
        if target_update_due(self._n_train_steps_total, self.target_update_period):
            check(lib().s2p_soft_update(ptr(self.critic.target_flat), ptr(self.critic.flat), self.critic.n_target,
                                        self.soft_target_tau, stream()), "s2p_soft_update")
        if self._need_to_update_eval_statistics:
            self._need_to_update_eval_statistics = False
            losses = t["losses"].cpu()
            for i, k in enumerate(("QF1 Loss", "QF2 Loss", "VF Loss", "Policy Loss")):
                self.eval_statistics[k] = float(losses[i])
            if _latent and not self.freeze_slac and hasattr(self, "_latent_losses"):
                for k, val in zip(("SLAC Loss kld", "SLAC Loss image", "SLAC Loss reward"), self._latent_losses):
                    self.eval_statistics[k] = float(val)
        self._n_train_steps_total += 1
        return t["losses"]

    def train_from_torch(self, batch):
        """One step on a `random_batch` dict of `slac_buffer.ReplayBuffer` (iql_trainer.py:209-435, the SLAC branch)."""
        z, next_z, action, feature_action, _ = self.slac_algo.prepare_batch(batch["observations"], batch["actions"])
        policy_input = feature_action if self.slac_policy_input_type == "feature_action" else z
        return self.train_from_latents(z, next_z, action, policy_input, batch["rewards"], batch["terminals"], _latent=True)

    def end_epoch(self, epoch):
        self._need_to_update_eval_statistics = True

    def get_diagnostics(self):
        return OrderedDict(self.eval_statistics)

    # ---- snapshots --------------------------------------------------------------------------------------------------------------
    def _critic_tensors(self, flat):
        out = OrderedDict()
        for n in ("qf1", "qf2", "vf"):
            out.update(_export(self.critic.nets[n], self.critic.packed[n], flat, n + "."))
        return out

    def _critic_put(self, flat, named):
        for n in ("qf1", "qf2", "vf"):
            sub = {k: v for k, v in named.items() if k.startswith(n + ".")}
            if sub:
                _load(self.critic.nets[n], self.critic.packed[n], flat, sub, n + ".")

    def state_dict(self):
        po = self.policy
        return dict(critic=self.critic.state_dict(), policy=po.state_dict(),
                    critic_optimizer=self.critic_optimizer.state_dict(self._critic_tensors, self.critic.keys()),
                    policy_optimizer=self.policy_optimizer.state_dict(lambda fl: _export(po, po.packed, fl), po.keys()),
                    n_train_steps_total=self._n_train_steps_total)

    def load_state_dict(self, sd):
        po = self.policy
        self.critic.load_state_dict(sd["critic"])
        po.load_state_dict(sd["policy"])
        self.critic_optimizer.load_state_dict(sd["critic_optimizer"], self._critic_put, self.critic.keys())
        self.policy_optimizer.load_state_dict(sd["policy_optimizer"], lambda fl, named: named and _load(po, po.packed, fl, named),
                                              po.keys())
        self._n_train_steps_total = int(sd.get("n_train_steps_total", 0))
        return self

    def get_snapshot(self):
        """iql_trainer.py:467-483, as state_dicts (the reference pickles the modules)."""
        snap = self.state_dict()
        if self.slac_algo is not None:
            snap["slac_algo_latent"] = self.slac_algo.latent.state_dict()
            snap["slac_algo_latent_optimizer"] = self.slac_algo.optim_latent.state_dict()
        return snap

