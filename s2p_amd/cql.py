"""CQL on SLAC latents (SPEC.md N3e; reference `rlkit/torch/sac/cql_trainer.py:234-418, 576-585` in its SLAC configuration): the
second consumer of the replay buffer and the latent model, on the networks, flat buffers, optimizer and trainer base of
`s2p_amd/offline_rl.py` and the grouped layers of `s2p_amd/mlp.py`.  A step has two phases.  The policy phase runs the policy on B
rows, draws the reparameterised action into the action columns of a Q-input buffer, runs qf1 | qf2 on it, and differentiates the SAC
loss THROUGH the critics to the action (s2p_mlp_linear_dgrad: the critics' gradient buffer is not touched).  The critic phase runs
the UPDATED policy once on [policy_input; policy_next_input], fills the B (1 + 3 num_random) rows of the Q-input buffer with three
s2p_tanh_gauss_rsample calls (the policy trunk runs on B rows, not on B num_random repeated ones), runs qf1 | qf2 on them and the
targets on B rows as ONE grouped launch per layer, and the fused CQL head.  DESIGN.md section 6b.5 counts the launches.  No CPU
fallback, no host synchronisation inside a step."""
from collections import OrderedDict

import torch

from ._lib import lib, ptr, stream
from .mlp import Net, bwd_plan, bwd_tables, entry_point, fwd_plan, fwd_tables, split_chunks
from .offline_rl import CriticSLAC, LatentTrainer, Qfunction, TanhGaussianPolicy, Vfunction  # noqa: F401  (re-exported)
from .ops import pad_to

NOISE = ("eps0", "eps1", "uniform", "eps2", "eps3")


def step_plan(critic, policy, B, R):
    """The networks' views of a step at batch size B with R sampled actions per row, and its launches, from shapes alone:
    (nets, plans).  The policy on B rows (trained) and on 2 B rows (forward only), qf1 | qf2 under the policy's action on B rows
    (differentiated to the action, no weight gradient), qf1 | qf2 on the B (1 + 3 R) rows of the critic loss, the targets on B."""
    M, q_names = B * (1 + 3 * R), ("qf1", "qf2")
    nets = dict(pol=[Net("policy", policy.packed, B, B)], pol2=[Net("policy", policy.packed, 2 * B)],
                qpol=[Net(n, critic.packed[n], B, B) for n in q_names], qcrit=[Net(n, critic.packed[n], M, M) for n in q_names],
                qtgt=[Net("target_" + n, critic.packed[n], B) for n in q_names])
    plans = dict(policy_fwd=fwd_plan(nets["pol"], True), policy_bwd=bwd_plan(nets["pol"], True), policy2_fwd=fwd_plan(nets["pol2"], True),
                 qpol_fwd=fwd_plan(nets["qpol"], True), qpol_dgrad=bwd_plan(nets["qpol"], True),
                 critic_fwd=fwd_plan(nets["qcrit"] + nets["qtgt"], True), critic_bwd=bwd_plan(nets["qcrit"], True))
    return nets, plans


class CQLTrainer(LatentTrainer):
    """`CQLTrainer` of the reference in its SLAC configuration (`image_rl`, `slac_representation`, two Q networks,
    `min_q_version = 3`), the arguments it uses under their reference names.  Not built: see SPEC.md N3e."""
    TRAINED = ("qf1", "qf2")                    # (vf takes part in no loss: no gradient, no optimizer state, as in the reference)

    def __init__(self, env, policy, qf1=None, qf2=None, target_qf1=None, target_qf2=None, discount=0.99, reward_scale=1.0,
                 policy_lr=1e-3, qf_lr=1e-3, soft_target_tau=1e-2, use_automatic_entropy_tuning=True, target_entropy=None,
                 policy_eval_start=0, num_qs=2, min_q_version=3, temp=1.0, min_q_weight=1.0, max_q_backup=False,
                 deterministic_backup=True, num_random=10, with_lagrange=False, lagrange_thresh=0.0, image_rl=True, critic=None,
                 vf=None, curl_learning=False, slac_representation=True, slac_algo=None, freeze_slac=False, slac_update_period=1,
                 slac_policy_input_type="feature_action", policy_weight_decay=0, q_weight_decay=0, generator=None, mlp_compute="fp32"):
        for flag, what in ((with_lagrange, "with_lagrange"), (max_q_backup, "max_q_backup"), (num_qs != 2, "num_qs != 2"),
                           (min_q_version != 3, "min_q_version != 3"), (curl_learning, "the CURL branch"),
                           (not (image_rl and slac_representation), "the state-RL branch (image_rl and slac_representation only)"),
                           (policy_weight_decay or q_weight_decay, "weight decay")):
            if flag:
                raise NotImplementedError(what)
        if int(num_random) < 1 or not temp > 0:
            raise ValueError("num_random >= 1 and temp > 0")
        super().__init__(env, policy, critic, qf1, qf2, target_qf1, target_qf2, vf, qf_lr, policy_lr, slac_algo, freeze_slac,
                         slac_update_period, slac_policy_input_type, mlp_compute=mlp_compute)
        self.obs_dim, self.action_dim = self.qf1.input_size - policy.action_dim, policy.action_dim
        if self.qf1.output_size != 1 or self.obs_dim <= 0:
            raise ValueError("qf: (Z + A) -> 1")
        self.discount, self.reward_scale, self.soft_target_tau = float(discount), float(reward_scale), float(soft_target_tau)
        self.use_automatic_entropy_tuning = bool(use_automatic_entropy_tuning)
        if not target_entropy:                  # (the reference's test: None and 0 both fall back)
            shape = env.action_space.shape if env is not None else (self.action_dim,)
            target_entropy = -float(torch.Size(shape).numel())
        self.target_entropy = float(target_entropy)
        self.policy_eval_start, self.num_random = int(policy_eval_start), int(num_random)
        self.temp, self.min_q_weight, self.deterministic_backup = float(temp), float(min_q_weight), bool(deterministic_backup)
        self.generator, self.policy_lr = generator, float(policy_lr)
        # log_alpha with its Adam moments, and its step counter: read and written by s2p_sac_policy_head alone
        self.log_alpha_state = torch.zeros(3, dtype=torch.float32, device=self.device)
        self.log_alpha_step = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.alpha = torch.ones(1, dtype=torch.float32, device=self.device)
        self._current_epoch = self._num_q_update_steps = self._num_policy_update_steps = 0

    @property
    def log_alpha(self):
        return self.log_alpha_state[:1]

    # ---- buffers and group tables per batch size, built once ----------------------------------------------------------------------
    def _tables(self, B):
        if B in self._buf:
            return self._buf[B]
        cr, po, dev, f = self.critic, self.policy, self.device, torch.float32
        Z, A, R = self.obs_dim, self.action_dim, self.num_random
        M, Kq = B * (1 + 3 * R), pad_to(Z + A, 4)

        def z(*shape):
            return torch.zeros(*shape, dtype=f, device=dev)

        t = dict(M=M, xq=z(M, Kq), xpq=z(B, Kq), xt=z(B, Kq), xp=z(2 * B, po.packed.off[0][2]), raw=z(2 * B, 2 * A), draw=z(B, 2 * A),
                 q_all=z(2, M), dq_all=z(2, M), tq=z(2, B), qn=z(2, B), dqn=z(2, B), dxpq=z(2, B, Kq), logp0=z(B), dlogp=z(B),
                 new_log_pi=z(B), logp_samp=z(B, 2 * R), sac=z(4), losses=z(4), std=z(2), bc=z(1), q_target=z(B), ones=torch.ones(B, dtype=f, device=dev),
                 action=z(B, A), reward=z(B), terminal=z(B), eps0=z(B, A), eps1=z(B, A), uniform=z(B * R, A), eps2=z(B * R, A), eps3=z(B * R, A))
        nets, plans = step_plan(cr, po, B, R)
        nets["pol"][0].bind(po.flat, po.grad, t["xp"], t["raw"], t["draw"])
        nets["pol2"][0].bind(po.flat, po.grad, t["xp"], t["raw"])
        for i, n in enumerate(nets["qpol"]):
            n.bind(cr.flat, cr.grad, t["xpq"], t["qn"][i], t["dqn"][i], t["dxpq"][i])
        for i, n in enumerate(nets["qcrit"]):
            n.bind(cr.flat, cr.grad, t["xq"], t["q_all"][i], t["dq_all"][i])
        for i, n in enumerate(nets["qtgt"]):
            n.bind(cr.target_flat, None, t["xt"], t["tq"][i])
        t["nets"] = nets
        for k, plan in plans.items():
            t[k] = fwd_tables(plan) if k.endswith("fwd") else bwd_tables(plan, with_weights=k != "qpol_dgrad")
        # the critics' wide layers run on B (1 + 3 R) rows: their weight gradient is split by rows (the N = 1 last layer is not)
        t["critic_split"], need = [], 0
        for gs, G, N, a in t["critic_bwd"]:
            S = 0
            if N > 16:
                tiles = sum(-(-N // 32) * -(-g.K // 64) for g in gs)
                S = split_chunks(tiles, M)
                need = max(need, lib().s2p_mlp_linear_bwd_split_workspace(gs, G, N, S))
            t["critic_split"].append(S)
        t["split_ws"] = torch.empty(max(need // 4, 1), dtype=f, device=dev)
        self._buf = {B: t}                      # (one batch size is kept: a new one replaces the tables and their buffers)
        return t

    def _copy(self, dst, src):
        self.launches["torch copy"] = self.launches.get("torch copy", 0) + 1
        dst.copy_(src)

    def _noise(self, t, noise):
        B, A, R, dev = t["action"].shape[0], self.action_dim, self.num_random, self.device
        if noise is None:                       # in place, one kernel per tensor
            for k in NOISE:
                self.launches["torch random"] = self.launches.get("torch random", 0) + 1
                if k == "uniform":
                    t[k].uniform_(-1.0, 1.0, generator=self.generator)
                else:
                    t[k].normal_(generator=self.generator)
            return
        for k in NOISE:
            want = (B if k in ("eps0", "eps1") else B * R, A)
            if tuple(noise[k].shape) != want:
                raise ValueError("noise[%r]: shape %s, expected %s" % (k, tuple(noise[k].shape), want))
            self._copy(t[k], noise[k].to(dev, torch.float32))

    def _rsample(self, raw, eps, M, rep, action, action_pitch, group, logp, logp_group):
        A = self.action_dim
        self._call("s2p_tanh_gauss_rsample", ptr(raw), 2 * A, ptr(eps), A, M, A, rep, ptr(action), action_pitch, group, ptr(logp),
                   logp_group, None, 0, stream())

    @torch.no_grad()
    def train_from_latents(self, z, next_z, action, policy_input, policy_next_input, rewards, terminals, noise=None, _latent=False):
        """One CQL step on given latents: z, next_z [B, Z], action [B, A], policy_input, policy_next_input [B, P], rewards /
        terminals [B] or [B, 1]; noise: None (drawn on the device) or a dict of eps0, eps1 [B, A] and uniform, eps2, eps3
        [B num_random, A] (row b num_random + r belongs to batch row b).  -> the device tensor [qf1, qf2, min_qf1, min_qf2]."""
        B, Z, A, R, dev, f = z.shape[0], self.obs_dim, self.action_dim, self.num_random, self.device, torch.float32
        self.launches = OrderedDict()
        t, st = self._tables(B), stream()
        M, Kq, P = t["M"], t["xq"].shape[1], self.policy.obs_dim
        self._current_epoch += 1
        bc = self._current_epoch < self.policy_eval_start
        z, next_z, action = z.to(dev, f), next_z.to(dev, f), action.to(dev, f)
        samp = t["xq"][B:].view(B, 3 * R, Kq)
        self._copy(t["xq"][:B, :Z], z)
        self._copy(t["xq"][:B, Z:Z + A], action)
        self._copy(samp[:, :, :Z], z[:, None, :])             # z staged into the 3 R sampled rows of every batch row
        self._copy(t["xpq"][:, :Z], z)
        self._copy(t["xt"][:, :Z], next_z)
        self._copy(t["xp"][:B, :P], policy_input.to(dev, f))
        self._copy(t["xp"][B:, :P], policy_next_input.to(dev, f))
        self._copy(t["action"], action)
        self._copy(t["reward"], rewards.to(dev, f).reshape(B))
        self._copy(t["terminal"], terminals.to(dev, f).reshape(B))
        self._noise(t, noise)
        self._copy(samp[:, :R, Z:Z + A], t["uniform"].view(B, R, A))
        tune = 1 if self.use_automatic_entropy_tuning else 0

        # ---- policy phase ----
        self._run(t["policy_fwd"])
        self._rsample(t["raw"], t["eps0"], B, 1, t["xpq"][:, Z:], Kq, 1, t["logp0"], 1)
        self._run(t["qpol_fwd"])                               # (in the cloning branch only the 'Policy Loss' statistic reads it)
        self._call("s2p_sac_policy_head", ptr(t["logp0"]), ptr(t["qn"][0]), ptr(t["qn"][1]), B, tune, self.target_entropy, self.policy_lr,
                   0.9, 0.999, 1e-8, ptr(self.log_alpha_state), ptr(self.log_alpha_step), ptr(self.alpha), ptr(t["sac"]), ptr(t["dlogp"]),
                   None if bc else ptr(t["dqn"][0]), None if bc else ptr(t["dqn"][1]), st)
        if bc:
            self._call("s2p_tanh_gauss_policy_head", ptr(t["raw"]), 2 * A, ptr(t["action"]), A, ptr(t["ones"]), B, A, ptr(t["bc"]),
                       ptr(t["draw"]), 2 * A, None, st)
            self._call("s2p_tanh_gauss_rsample_bwd", ptr(t["raw"]), 2 * A, ptr(t["eps0"]), A, ptr(t["dlogp"]), None, None, 0, B, A,
                       ptr(t["draw"]), 2 * A, 1, st)
        else:
            self._run(t["qpol_dgrad"], "s2p_mlp_linear_dgrad")
            self._call("s2p_tanh_gauss_rsample_bwd", ptr(t["raw"]), 2 * A, ptr(t["eps0"]), A, ptr(t["dlogp"]), ptr(t["dxpq"][0][:, Z:]),
                       ptr(t["dxpq"][1][:, Z:]), Kq, B, A, ptr(t["draw"]), 2 * A, 0, st)
        self._run(t["policy_bwd"], "s2p_mlp_linear_bwd")
        self._adam(self.policy_optimizer)
        self._num_policy_update_steps += 1

        # ---- critic phase: every policy pass from the updated policy, forward only ----
        self._run(t["policy2_fwd"])
        raw, raw_next = t["raw"][:B], t["raw"][B:]
        self._rsample(raw_next, t["eps1"], B, 1, t["xt"][:, Z:], Kq, 1, t["new_log_pi"], 1)
        self._rsample(raw_next, t["eps3"], B, R, t["xq"][B + R:, Z:], Kq, 3 * R, t["logp_samp"], 2 * R)
        self._rsample(raw, t["eps2"], B, R, t["xq"][B + 2 * R:, Z:], Kq, 3 * R, t["logp_samp"][:, R:], 2 * R)
        self._run(t["critic_fwd"])
        self._call("s2p_cql_critic_head", ptr(t["q_all"]), M, ptr(t["q_all"][0][B:]), M, ptr(t["logp_samp"]), ptr(t["tq"]),
                   ptr(t["new_log_pi"]), ptr(self.alpha), ptr(t["reward"]), ptr(t["terminal"]), B, R, A, self.reward_scale, self.discount,
                   self.temp, self.min_q_weight, 1 if self.deterministic_backup else 0, ptr(t["losses"]), ptr(t["dq_all"]), M,
                   ptr(t["dq_all"][0][B:]), M, ptr(t["q_target"]), ptr(t["std"]), st)
        for (gs, G, N, a), S in zip(t["critic_bwd"], t["critic_split"]):
            if S:
                self._call(entry_point("bwd_split", N, self.mlp_compute), gs, G, N, a, S, ptr(t["split_ws"]), t["split_ws"].numel() * 4, st)
            else:
                self._call(entry_point("bwd", N, self.mlp_compute), gs, G, N, a, st)
        self._adam(self.critic_optimizer)
        self._num_q_update_steps += 1
        self._update_latent(_latent)
        self._call("s2p_soft_update", ptr(self.critic.target_flat), ptr(self.critic.flat), self.critic.n_target, self.soft_target_tau, st)
        self._bc = bc
        if self._need_to_update_eval_statistics:
            self._need_to_update_eval_statistics = False
            self.eval_statistics.update(self.last_statistics())
            self.eval_statistics["Num Q Updates"] = self._num_q_update_steps
            self.eval_statistics["Num Policy Updates"] = self._num_policy_update_steps
            self._latent_statistics(_latent)
        self._n_train_steps_total += 1
        return t["losses"]

    def last_statistics(self):
        """The last step's figures under the reference's key names (one device-to-host copy each of three small tensors);
        `policy_loss` is the loss the policy step optimised, which the reference does not print."""
        t = next(iter(self._buf.values()))
        losses, sac, std = t["losses"].cpu(), t["sac"].cpu(), t["std"].cpu()
        out = OrderedDict()
        out["QF1 Loss"], out["min QF1 Loss"], out["QF2 Loss"], out["min QF2 Loss"] = (float(losses[i]) for i in (0, 2, 1, 3))
        out["Std QF1 values"], out["Std QF2 values"] = float(std[0]), float(std[1])
        out["Policy Loss"] = float(sac[3])
        out["policy_loss"] = float(sac[2]) + float(t["bc"].cpu()[0]) if self._bc else float(sac[1])
        if self.use_automatic_entropy_tuning:
            out["Alpha"], out["Alpha Loss"] = float(self.alpha.cpu()[0]), float(sac[0])
        return out

    def train_from_torch(self, batch):
        """One step on a `random_batch` dict of `slac_buffer.ReplayBuffer` (cql_trainer.py:234-418, the SLAC branch)."""
        z, next_z, action, feature_action, next_feature_action = self.slac_algo.prepare_batch(batch["observations"], batch["actions"])
        policy_input, policy_next_input = self._policy_inputs(z, next_z, feature_action, next_feature_action)
        return self.train_from_latents(z, next_z, action, policy_input, policy_next_input, batch["rewards"], batch["terminals"], _latent=True)

    # ---- snapshots: the base's, and log_alpha with its optimizer and the epoch counter on top -------------------------------------
    def state_dict(self):
        la, step = self.log_alpha_state.cpu(), int(self.log_alpha_step.item())
        group = dict(lr=self.policy_lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, params=[0])
        state = {0: {"step": torch.tensor(float(step)), "exp_avg": la[1:2].clone(), "exp_avg_sq": la[2:3].clone()}} if step else {}
        return dict(super().state_dict(), log_alpha=la[:1].clone(), alpha_optimizer={"state": state, "param_groups": [group]},
                    current_epoch=self._current_epoch)

    def load_state_dict(self, sd):
        super().load_state_dict(sd)
        s = sd["alpha_optimizer"]["state"].get(0)
        la = torch.zeros(3)
        la[0] = torch.as_tensor(sd["log_alpha"]).reshape(-1)[0]
        if s is not None:
            la[1], la[2] = torch.as_tensor(s["exp_avg"]).reshape(-1)[0], torch.as_tensor(s["exp_avg_sq"]).reshape(-1)[0]
        self.log_alpha_state.copy_(la)
        self.log_alpha_step.fill_(int(s["step"]) if s is not None else 0)
        self.alpha.copy_(torch.exp(la[:1]) if self.use_automatic_entropy_tuning else torch.ones(1))
        self._current_epoch = int(sd.get("current_epoch", self._n_train_steps_total))
        return self
