"""Plain-torch restatement of SPEC.md N3e (the CQL step of `rlkit/torch/sac/cql_trainer.py:234-418, 576-585` in its SLAC
configuration) on the reference-layout state_dicts of tests/iql_ref.py (`critic` with `qf1.fc0.weight` ... `vf.last_fc.bias`, `policy`
with `fc0` ... `last_fc_log_std`).  The noise is an argument: a dict of eps0 [B,A] (the policy-loss sample), eps1 [B,A] (the backup's
next action), uniform [B R,A] in (-1, 1), eps2 [B R,A] (samples at policy_input), eps3 [B R,A] (samples at policy_next_input); row
b R + r belongs to batch row b, as in `_get_policy_actions`.  tests/test_cql.py asserts that it reproduces the fixture of the REAL
trainer to 1e-9 in fp64; the GPU tests use it for the shapes the fixture does not hold."""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

import iql_ref as R

CFG = dict(discount=0.99, reward_scale=1.0, policy_lr=1e-4, qf_lr=3e-4, soft_target_tau=0.005, temp=1.0, min_q_weight=5.0,
           num_random=4, deterministic_backup=False, use_automatic_entropy_tuning=True, target_entropy=None, policy_eval_start=2)
HEADS = ("last_fc", "last_fc_log_std")
NOISE = ("eps0", "eps1", "uniform", "eps2", "eps3")
STATS = ("QF1 Loss", "QF2 Loss", "min QF1 Loss", "min QF2 Loss", "Std QF1 values", "Std QF2 values", "Policy Loss", "Alpha",
         "Alpha Loss", "policy_loss")           # the last one: the loss the policy step optimises (the reference never prints it)


def sample(policy, x, eps, rep=1):
    """rsample + log_prob from the pre-tanh value (distributions.py:339-386, gaussian_policy.py:113-146): -> action, logp [rows],
    mean, raw log std.  `rep` repeats every row of x (the reference repeats the input and runs the policy on B R rows)."""
    mean, raw_ls = R.mlp_forward(policy, "", x, HEADS)
    mean_r, ls = mean.repeat_interleave(rep, 0), torch.clamp(raw_ls, -20.0, 2.0).repeat_interleave(rep, 0)
    std = torch.exp(ls)
    u = mean_r + std * eps
    normal = (-0.5 * ((u - mean_r) / std) ** 2 - ls - 0.5 * math.log(2 * math.pi)).sum(1)
    log2 = float(torch.tensor(math.log(2.0), dtype=torch.float32))      # an fp32 tensor in the reference at any precision
    return torch.tanh(u), normal - 2.0 * (log2 - u - F.softplus(-2.0 * u)).sum(1), mean, raw_ls


def q_of(critic, name, z, action):
    return R.mlp_forward(critic, name + ".", torch.cat([z, action], 1))[0][:, 0]


def make_noise(B, A, num_random, seed):
    g = torch.Generator().manual_seed(seed)
    n = {k: torch.randn(B if k in ("eps0", "eps1") else B * num_random, A, generator=g) for k in NOISE}
    n["uniform"] = torch.rand(B * num_random, A, generator=g) * 2 - 1
    return n


def make_batch(B, Z, A, P, seed, terminals=False, scale=1.0):
    b = R.make_batch(B, Z, A, P, seed, terminals=terminals, scale=scale, extreme_rows=None)
    b["policy_next_input"] = torch.randn(B, P, generator=torch.Generator().manual_seed(seed + 7919)) * scale
    return b


class Stepper:
    """The step's state across calls: the parameters (copies of the given state_dicts, on their device), `log_alpha`, and the three
    torch.optim.Adam objects.  `step(batch, noise)` runs one step and returns its STATS and gradients."""

    def __init__(self, critic, policy, dtype, cfg=CFG, log_alpha=0.0):
        self.cfg, self.dtype, self.epoch = cfg, dtype, 0
        self.critic = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(k.startswith(("qf1.", "qf2.")))) for k, v in critic.items())
        self.policy = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in policy.items())
        dev = next(iter(self.policy.values())).device
        qparams = [v for v in self.critic.values() if v.requires_grad]       # vf takes part in no loss: no gradient, no Adam state
        self.la = torch.full((1,), float(log_alpha), dtype=dtype, device=dev, requires_grad=True)
        self.ones = torch.ones(1, dtype=dtype, device=dev)
        self.opt_c = torch.optim.Adam(qparams, lr=cfg["qf_lr"], betas=(0.9, 0.999))
        self.opt_p = torch.optim.Adam(list(self.policy.values()), lr=cfg["policy_lr"])
        self.opt_a = torch.optim.Adam([self.la], lr=cfg["policy_lr"])
        self.pairs = [(self.critic["target_" + k], v) for k, v in self.critic.items() if k.startswith(("qf1.", "qf2."))]

    def step(self, batch, noise):
        cfg, dtype, critic, policy, la = self.cfg, self.dtype, self.critic, self.policy, self.la
        opt_c, opt_p, opt_a = self.opt_c, self.opt_p, self.opt_a
        Rn, temp, w = cfg["num_random"], cfg["temp"], cfg["min_q_weight"]
        self.epoch += 1
        b = {k: v.to(dtype) for k, v in batch.items()}
        n = {k: v.to(dtype) for k, v in noise.items()}
        z, nz, a, r, t = b["z"], b["next_z"], b["action"], b["rewards"].reshape(-1), b["terminals"].reshape(-1)
        A, epoch, out = a.shape[1], self.epoch, {}
        target_entropy = cfg["target_entropy"] if cfg["target_entropy"] else -float(A)
        # 1-4: the policy and alpha
        new_a, log_pi, mean, raw_ls = sample(policy, b["policy_input"], n["eps0"])
        if cfg["use_automatic_entropy_tuning"]:
            alpha_loss = -(la * (log_pi + target_entropy).detach()).mean()
            opt_a.zero_grad()
            alpha_loss.backward()
            opt_a.step()
            alpha = la.detach().exp()
            out["Alpha"], out["Alpha Loss"] = alpha[0].clone(), alpha_loss.detach().clone()
        else:
            alpha = self.ones
        q_new = torch.min(q_of(critic, "qf1", z, new_a), q_of(critic, "qf2", z, new_a))
        if epoch < cfg["policy_eval_start"]:
            policy_loss = (alpha * log_pi - R.tanh_normal_log_prob(mean, raw_ls, a)[0]).mean()
        else:
            policy_loss = (alpha * log_pi - q_new).mean()
        out["policy_loss"], out["Policy Loss"] = policy_loss.detach().clone(), (log_pi - q_new).mean().detach()
        pg = torch.autograd.grad(policy_loss, list(policy.values()))        # (the critic's share of this backward is discarded)
        opt_p.zero_grad()
        for p, g in zip(policy.values(), pg):
            p.grad = g
        opt_p.step()
        out.update(("grad.policy." + k, g.detach().clone()) for k, g in zip(policy, pg))
        # 5-9: the critic loss, every policy pass from the UPDATED policy and without a gradient
        q_pred = [q_of(critic, nm, z, a) for nm in ("qf1", "qf2")]
        with torch.no_grad():
            next_a, new_log_pi, _, _ = sample(policy, b["policy_next_input"], n["eps1"])
            target_q = torch.min(q_of(critic, "target_qf1", nz, next_a), q_of(critic, "target_qf2", nz, next_a))
            if not cfg["deterministic_backup"]:
                target_q = target_q - alpha * new_log_pi
            q_target = cfg["reward_scale"] * r + (1.0 - t) * cfg["discount"] * target_q
            curr_a, curr_lp, _, _ = sample(policy, b["policy_input"], n["eps2"], Rn)
            nxt_a, nxt_lp, _, _ = sample(policy, b["policy_next_input"], n["eps3"], Rn)
        zr = z.repeat_interleave(Rn, 0)
        density = math.log(0.5 ** A)
        critic_loss = 0.0
        for i, nm in enumerate(("qf1", "qf2")):
            q_rand, q_next, q_curr = (q_of(critic, nm, zr, x).view(-1, Rn) for x in (n["uniform"], nxt_a, curr_a))
            std = torch.std(torch.cat([q_rand, q_pred[i][:, None], q_next, q_curr], 1), dim=1)
            cat = torch.cat([q_rand - density, q_next - nxt_lp.view(-1, Rn), q_curr - curr_lp.view(-1, Rn)], 1)
            min_qf = torch.logsumexp(cat / temp, dim=1).mean() * w * temp - q_pred[i].mean() * w
            qf = ((q_pred[i] - q_target) ** 2).mean() + min_qf
            critic_loss = critic_loss + qf
            out["QF%d Loss" % (i + 1)], out["min QF%d Loss" % (i + 1)] = qf.detach().clone(), min_qf.detach().clone()
            out["Std QF%d values" % (i + 1)] = std.mean().detach()
        opt_c.zero_grad()
        critic_loss.backward()
        opt_c.step()
        out.update(("grad." + k, v.grad.detach().clone()) for k, v in critic.items() if v.requires_grad)
        out["q_target"] = q_target
        # 12: the Polyak update, every step
        with torch.no_grad():
            tau = cfg["soft_target_tau"]
            for tgt, v in self.pairs:
                tgt.copy_(tgt * (1.0 - tau) + v * tau)
        return out

    def final(self):
        return (OrderedDict((k, v.detach().clone()) for k, v in self.critic.items()),
                OrderedDict((k, v.detach().clone()) for k, v in self.policy.items()), self.la.detach().clone())


def train(critic, policy, batches, noises, dtype, cfg=CFG, log_alpha=0.0):
    """One step per (batch, noise) from the given state_dicts (not modified).  -> (per_step: a dict per step of STATS and
    `grad.<critic key>` / `grad.policy.<key>`;  final: (critic state_dict, policy state_dict, log_alpha) after the last step)."""
    st = Stepper(critic, policy, dtype, cfg, log_alpha)
    return [st.step(b, n) for b, n in zip(batches, noises)], st.final()
