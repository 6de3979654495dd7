"""IQL on SLAC latents (SPEC.md N3d; reference `rlkit/torch/sac/iql_trainer.py:209-435`): the consumer loop the replay buffer and
the latent model feed, on the networks, flat buffers, optimizer and trainer base of `s2p_amd/offline_rl.py`.  A train step runs the
six networks as groups of one grouped launch per layer (`s2p_amd/mlp.py`, csrc/mlp.hip), then the fused critic and policy heads
(csrc/iql.hip); DESIGN.md section 6b.4 counts the launches.  No CPU fallback."""
from collections import OrderedDict

import torch

from ._lib import ptr, stream
from .mlp import Net, bwd_plan, bwd_tables, fwd_plan, fwd_tables
from .offline_rl import CriticSLAC, LatentTrainer, Qfunction, TanhGaussianPolicy, Vfunction  # noqa: F401  (re-exported)
from .ops import pad_to


def target_update_due(n_train_steps, target_update_period):
    """iql_trainer.py:361: the Polyak update runs on the steps, counted from 0, that the period divides."""
    return n_train_steps % target_update_period == 0


def step_plan(critic, policy, B):
    """The six networks' views of a step at batch size B and its launches, from shapes alone: (nets, forward plan, backward plan).
    vf runs forward on [z; next_z] and backward on its first B rows; the targets have no backward."""
    rows = {"vf": 2 * B}
    nets = OrderedDict((n, Net(n, critic.packed[n], rows.get(n, B), None if n.startswith("target") else B)) for n in CriticSLAC.NETS)
    nets["policy"] = Net("policy", policy.packed, B, B)
    return nets, fwd_plan(list(nets.values())), bwd_plan([n for n in nets.values() if n.bwd_rows])


class IQLTrainer(LatentTrainer):
    """`IQLTrainer` of the reference in its SLAC configuration (`image_rl`, `slac_representation`, the integrated critic
    optimizer), the arguments it uses under their reference names.  Not built: see SPEC.md N3d."""
    TRAINED = ("qf1", "qf2", "vf")

    def __init__(self, env, policy, qf1=None, qf2=None, vf=None, quantile=0.5, target_qf1=None, target_qf2=None, discount=0.99,
                 reward_scale=1.0, policy_lr=1e-3, qf_lr=1e-3, policy_weight_decay=0, q_weight_decay=0, policy_update_period=1,
                 q_update_period=1, clip_score=None, soft_target_tau=1e-2, target_update_period=1, beta=1.0, critic=None,
                 slac_algo=None, freeze_slac=False, slac_update_period=1, slac_policy_input_type="feature_action", mlp_compute="fp32"):
        if policy_weight_decay or q_weight_decay or policy_update_period != 1 or q_update_period != 1:
            raise NotImplementedError("weight decay and update periods other than 1")
        super().__init__(env, policy, critic, qf1, qf2, target_qf1, target_qf2, vf, qf_lr, policy_lr, slac_algo, freeze_slac,
                         slac_update_period, slac_policy_input_type, share_hidden=True, mlp_compute=mlp_compute)
        self.quantile, self.discount, self.reward_scale, self.beta = float(quantile), float(discount), float(reward_scale), float(beta)
        self.clip_score = clip_score
        self.soft_target_tau, self.target_update_period = float(soft_target_tau), int(target_update_period)
        self.obs_dim, self.action_dim = self.vf.input_size, policy.action_dim
        if self.qf1.input_size != self.obs_dim + self.action_dim or self.qf1.output_size != 1 or self.vf.output_size != 1:
            raise ValueError("qf: (Z + A) -> 1, vf: Z -> 1")

    # ---- the grouped launches of a step: buffers and group tables per batch size, built once ---------------------------------
    def _tables(self, B):
        if B in self._buf:
            return self._buf[B]
        cr, po, dev, f = self.critic, self.policy, self.device, torch.float32
        Z, A = self.obs_dim, self.action_dim
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
        out = {"qf1": t["q"][0], "qf2": t["q"][1], "target_qf1": t["q"][2], "target_qf2": t["q"][3], "vf": t["v"], "policy": t["raw"]}
        dout = {"qf1": t["dq"][0], "qf2": t["dq"][1], "vf": t["dv"], "policy": t["draw"]}
        nets, fwd, bwd = step_plan(cr, po, B)
        for name, n in nets.items():
            own = po if name == "policy" else cr
            n.bind(po.flat if name == "policy" else cr.flat_of(name), own.grad, xin.get(name, t["xq"]), out[name], dout.get(name))
        t["nets"], t["fwd"], t["bwd"] = nets, fwd_tables(fwd), bwd_tables(bwd)
        self._buf = {B: t}                      # (one batch size is kept: a new one replaces the tables and their buffers)
        return t

    def _forward_backward(self, z, next_z, action, policy_input, rewards, terminals):
        """Every launch of a step up to the gradients; returns the tables (losses = [qf1, qf2, vf, policy])."""
        B, Z, A, dev, f = z.shape[0], self.obs_dim, self.action_dim, self.device, torch.float32
        t = self._tables(B)
        t["xq"][:, :Z] = z.to(dev, f)
        t["xq"][:, Z:Z + A] = action.to(dev, f)
        t["xv"][:B, :Z] = t["xq"][:, :Z]
        t["xv"][B:, :Z] = next_z.to(dev, f)
        t["xp"][:, :self.policy.obs_dim] = policy_input.to(dev, f)
        t["action"].copy_(action.to(dev, f))
        t["reward"].copy_(rewards.to(dev, f).reshape(B))
        t["terminal"].copy_(terminals.to(dev, f).reshape(B))
        st = stream()
        self.launches = OrderedDict()
        self._run(t["fwd"])
        clip = float("inf") if self.clip_score is None else float(self.clip_score)
        q, v = t["q"], t["v"]
        self._call("s2p_iql_critic_head", ptr(q[0]), ptr(q[1]), ptr(q[2]), ptr(q[3]), ptr(v[:B]), ptr(v[B:]), ptr(t["reward"]),
                   ptr(t["terminal"]), B, self.reward_scale, self.discount, self.quantile, self.beta, clip, ptr(t["losses"]),
                   ptr(t["dq"][0]), ptr(t["dq"][1]), ptr(t["dv"]), ptr(t["weights"]), ptr(t["adv"]), ptr(t["q_target"]), st)
        self._call("s2p_tanh_gauss_policy_head", ptr(t["raw"]), 2 * A, ptr(t["action"]), A, ptr(t["weights"]), B, A, ptr(t["losses"][3:]),
                   ptr(t["draw"]), 2 * A, None, st)
        self._run(t["bwd"], "s2p_mlp_linear_bwd")
        return t

    @torch.no_grad()
    def train_from_latents(self, z, next_z, action, policy_input, rewards, terminals, _latent=False):
        """One IQL step on given latents: z, next_z [B, Z], action [B, A], policy_input [B, P], rewards / terminals [B] or [B, 1]."""
        t = self._forward_backward(z, next_z, action, policy_input, rewards, terminals)
        self._adam(self.critic_optimizer)
        self._adam(self.policy_optimizer)
        self._update_latent(_latent)
        if target_update_due(self._n_train_steps_total, self.target_update_period):
            self._call("s2p_soft_update", ptr(self.critic.target_flat), ptr(self.critic.flat), self.critic.n_target,
                       self.soft_target_tau, stream())
        if self._need_to_update_eval_statistics:
            self._need_to_update_eval_statistics = False
            losses = t["losses"].cpu()
            for i, k in enumerate(("QF1 Loss", "QF2 Loss", "VF Loss", "Policy Loss")):
                self.eval_statistics[k] = float(losses[i])
            self._latent_statistics(_latent)
        self._n_train_steps_total += 1
        return t["losses"]

    def train_from_torch(self, batch):
        """One step on a `random_batch` dict of `slac_buffer.ReplayBuffer` (iql_trainer.py:209-435, the SLAC branch)."""
        z, next_z, action, feature_action, next_feature_action = self.slac_algo.prepare_batch(batch["observations"], batch["actions"])
        policy_input, _ = self._policy_inputs(z, next_z, feature_action, next_feature_action)
        return self.train_from_latents(z, next_z, action, policy_input, batch["rewards"], batch["terminals"], _latent=True)
