"""The networks, the optimizer and the trainer base of the offline RL trainers on SLAC latents (`s2p_amd/iql.py`, `s2p_amd/cql.py`;
SPEC.md N3d, N3e; networks of the reference's `examples/iql/custom_networks.py` and
`rlkit/torch/sac/policies/gaussian_policy.py:76-154`).  `Qfunction` / `Vfunction` / `TanhGaussianPolicy` carry the reference's
constructor arguments, its init and its `state_dict` keys; `CriticSLAC` owns qf1 | qf2 | vf in ONE flat fp32 buffer (beside flat
gradient and Adam-moment buffers of the same layout) and target_qf1 | target_qf2 in a second one of the layout of qf1 | qf2, so an
optimizer step is one s2p_adam_step_dev launch and the Polyak update one s2p_soft_update launch.  `LatentTrainer` is what the two
trainers share around their steps: the critic and the optimizers, snapshots, the epoch statistics and the latent model's update.
No CPU fallback."""
import math
from collections import OrderedDict

import torch

from ._lib import check, lib, ptr, stream
from .mlp import Net, Packed, check_compute, fwd_plan, fwd_tables, run

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
        self.packed = {"qf1": Packed(qf1.dims())}
        self.packed["qf2"] = Packed(qf2.dims(), self.packed["qf1"].end)
        self.packed["vf"] = Packed(vf.dims(), self.packed["qf2"].end)
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

    @torch.no_grad()
    def q_min(self, z, a):
        """min(qf1, qf2)([z | a]) -> [B], forward only: both networks are the two groups of one s2p_mlp_linear_fwd launch per layer."""
        z, a = z.to(self.device, torch.float32), a.to(self.device, torch.float32)
        qf1 = self.nets["qf1"]
        if z.dim() != 2 or a.dim() != 2 or z.shape[0] != a.shape[0] or z.shape[1] + a.shape[1] != qf1.input_size:
            raise ValueError("z [B,Z] and a [B,A] with Z + A = %d are needed" % qf1.input_size)
        B, f = z.shape[0], torch.float32
        if B == 0:
            return torch.zeros(0, dtype=f, device=self.device)
        if getattr(self, "_qmin", (None,))[0] != B:
            xp = torch.zeros(B, self.packed["qf1"].off[0][2], dtype=f, device=self.device)
            nets = []
            for name in ("qf1", "qf2"):
                hs = [torch.empty(B, h, dtype=f, device=self.device) for h in qf1.hidden_sizes]
                nets.append(Net(name, self.packed[name], B).bind(self.flat, None, xp, torch.empty(B, 1, dtype=f, device=self.device), act=hs))
            self._qmin = (B, nets, fwd_tables(fwd_plan(nets)))      # the table holds bare addresses: the entry keeps the buffers alive
        _, nets, table = self._qmin
        xp = nets[0].x
        xp[:, :z.shape[1]] = z
        xp[:, z.shape[1]:qf1.input_size] = a
        run(table)
        return torch.minimum(nets[0].out[:, 0], nets[1].out[:, 0])

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
        self.packed = Packed(self.dims())
        self.n = self.packed.end
        self._bf16_key, self._bf16 = None, None
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

    def packed_bf16(self):
        """The weight operands of the bf16-compute imagination chain (SPEC.md N3n), beside `packed` and under the key rule of
        `Gaussian.packed_bf16`: w[li] = the packed fp32 layer [N][Kpad] `.to(torch.bfloat16)` (round to nearest even; the last one
        holds the `last_fc` rows first), b[li] = the fp32 bias in place.  Re-made only when `flat` changed: its (data_ptr, _version),
        which `load_state_dict` and the trainers' optimizer step move."""
        key = (self.flat.data_ptr(), self.flat._version)
        if key != self._bf16_key:
            n = len(self.packed.dims)
            with torch.no_grad():
                w = [self.packed.w(self.flat, li).to(torch.bfloat16).contiguous() for li in range(n)]
            self._bf16_key, self._bf16 = key, dict(w=w, b=[self.packed.b(self.flat, li) for li in range(n)])
        return self._bf16

    @torch.no_grad()
    def act(self, policy_input):
        """tanh(mean): the reference's `MakeDeterministic`.  Forward only: each layer's output overwrites one of two scratch
        buffers, no activation is kept."""
        x = policy_input.to(self.device, torch.float32)
        B, f = x.shape[0], torch.float32
        if B not in self._eval:
            xp = torch.zeros(B, self.packed.off[0][2], dtype=f, device=self.device)
            hs = [torch.empty(B, max(self.hidden_sizes), dtype=f, device=self.device) for _ in range(2)]
            raw = torch.empty(B, 2 * self.action_dim, dtype=f, device=self.device)
            net = Net("policy", self.packed, B).bind(self.flat, None, xp, raw, act=[hs[li % 2] for li in range(len(self.hidden_sizes))])
            # the table holds bare addresses: the entry keeps `net`, and with it every buffer, alive beside it.  `flat` is only
            # ever written in place (load_state_dict, the optimizer), so its address in the table stays good
            self._eval = {B: (net, fwd_tables(fwd_plan([net])))}
        net, table = self._eval[B]
        xp, raw = net.x, net.out
        xp[:, :self.obs_dim] = x
        run(table)
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
        torch.autograd.graph.increment_version(self.flat)   # the launch wrote `flat` behind torch's back: packs keyed on _version follow

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


class LatentTrainer:
    """What `IQLTrainer` and `CQLTrainer` share: the critic beside the policy on one HIP device, an Adam per flat buffer, the
    `state_dict` halves of both, and the SLAC side of `train_from_torch`.  `TRAINED` names the critic networks the critic loss
    trains: they alone have gradients and optimizer state.  `mlp_compute`: "fp32", or "bf16" for every wide grouped launch of the
    step on the bf16 matrix cores (SPEC.md N3l; weights, gradients, Adam and the snapshots stay fp32).  `launches` counts the last
    step's library calls by entry-point name."""
    TRAINED = ()

    def __init__(self, env, policy, critic, qf1, qf2, target_qf1, target_qf2, vf, qf_lr, policy_lr, slac_algo, freeze_slac,
                 slac_update_period, slac_policy_input_type, share_hidden=False, mlp_compute="fp32"):
        self.mlp_compute = check_compute(mlp_compute)
        if slac_policy_input_type not in ("feature_action", "latent_z"):
            raise ValueError("slac_policy_input_type %r" % (slac_policy_input_type,))
        self.env, self.policy = env, policy
        self.critic = critic if critic is not None else CriticSLAC(qf1, qf2, target_qf1, target_qf2, vf, device=policy.device)
        if share_hidden and self.critic.nets["vf"].hidden_sizes != policy.hidden_sizes:
            raise ValueError("the policy and the critic share the hidden sizes (one grouped launch per layer)")
        if self.critic.device != policy.device or policy.device is None:
            raise ValueError("the policy and the critic share a HIP device")
        self.qf1, self.qf2, self.target_qf1, self.target_qf2, self.vf = (self.critic.nets[n] for n in CriticSLAC.NETS)
        self.device = policy.device
        self.slac_algo, self.freeze_slac, self.slac_update_period = slac_algo, bool(freeze_slac), int(slac_update_period)
        self.slac_policy_input_type = slac_policy_input_type
        self.critic_optimizer = _Adam(self.critic.flat, self.critic.grad, qf_lr)
        self.policy_optimizer = _Adam(policy.flat, policy.grad, policy_lr)
        self.eval_statistics = OrderedDict()
        self._n_train_steps_total = 0
        self._need_to_update_eval_statistics = True
        self._buf = {}
        self.launches = OrderedDict()           # the last step's library calls (and, in CQL, torch copies), by name

    # ---- counted launches -------------------------------------------------------------------------------------------------------
    def _call(self, name, *args):
        self.launches[name] = self.launches.get(name, 0) + 1
        check(getattr(lib(), name)(*args), name)

    def _adam(self, opt):
        self.launches["s2p_adam_step_dev"] = self.launches.get("s2p_adam_step_dev", 0) + 1
        opt.step()

    def _run(self, table, entry="s2p_mlp_linear_fwd"):
        run(table, entry, self._call, self.mlp_compute)

    # ---- the SLAC side of a step ------------------------------------------------------------------------------------------------
    def _policy_inputs(self, z, next_z, feature_action, next_feature_action):
        return (feature_action, next_feature_action) if self.slac_policy_input_type == "feature_action" else (z, next_z)

    def _update_latent(self, _latent):
        if _latent and not self.freeze_slac and self._n_train_steps_total % self.slac_update_period == 0:
            with torch.enable_grad():
                self._latent_losses = self.slac_algo.update_latent(writer=None)

    def _latent_statistics(self, _latent):
        if _latent and not self.freeze_slac and hasattr(self, "_latent_losses"):
            for k, val in zip(("SLAC Loss kld", "SLAC Loss image", "SLAC Loss reward"), self._latent_losses):
                self.eval_statistics[k] = float(val)

    def end_epoch(self, epoch):
        self._need_to_update_eval_statistics = True

    def get_diagnostics(self):
        return OrderedDict(self.eval_statistics)

    # ---- snapshots --------------------------------------------------------------------------------------------------------------
    def _critic_tensors(self, flat):
        out = OrderedDict()
        for n in self.TRAINED:
            out.update(_export(self.critic.nets[n], self.critic.packed[n], flat, n + "."))
        return out

    def _critic_put(self, flat, named):
        for n in self.TRAINED:
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
        """The reference's `get_snapshot` (iql_trainer.py:467-483, cql_trainer.py:722-740), as state_dicts (it pickles the modules)."""
        snap = self.state_dict()
        if self.slac_algo is not None:
            snap["slac_algo_latent"] = self.slac_algo.latent.state_dict()
            snap["slac_algo_latent_optimizer"] = self.slac_algo.optim_latent.state_dict()
        return snap
