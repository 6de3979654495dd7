"""Plain-torch restatement of SPEC.md N3d (the IQL step of `rlkit/torch/sac/iql_trainer.py:209-435` in its SLAC configuration) on
reference-layout state_dicts: `critic` with keys `qf1.fc0.weight` ... `vf.last_fc.bias`, `policy` with `fc0` ... `last_fc_log_std`.
tests/test_iql.py asserts that it reproduces the fixture of the REAL trainer to 1e-9 in fp64; the GPU tests use it for the shapes
the fixture does not hold (its fp32 run gives the ref32_err there)."""
import math
from collections import OrderedDict

import torch

CFG = dict(discount=0.99, reward_scale=1.0, policy_lr=1e-4, qf_lr=3e-4, soft_target_tau=0.005, beta=0.1, quantile=0.7, clip_score=100.0,
           target_update_period=2)
NETS = ("qf1", "qf2", "target_qf1", "target_qf2", "vf")


def rel_max(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def n_hidden(sd, prefix=""):
    return sum(1 for k in sd if k.startswith(prefix + "fc") and k.endswith(".weight"))


def mlp_names(nh, heads=("last_fc",)):
    return ["fc%d" % i for i in range(nh)] + list(heads)


def critic_keys(nh):
    return [n + "." + layer + "." + p for n in NETS for layer in mlp_names(nh) for p in ("weight", "bias")]


def policy_keys(nh):
    return [layer + "." + p for layer in mlp_names(nh, ("last_fc", "last_fc_log_std")) for p in ("weight", "bias")]


def init_params(Z, A, H, P, n_layers=2, seed=0, last_scale=1.0):
    """The init of SPEC.md N3d: hidden weights uniform +-1/sqrt(OUT width), hidden biases 0, last layers uniform +-3e-3 with bias 0,
    both policy heads +-1e-3 (the log-std head's bias included); the four Q networks independent.  last_scale multiplies the last
    layers' weights (tests: the +-3e-3 init makes vf and the advantages degenerate)."""
    g = torch.Generator().manual_seed(seed)

    def u(shape, bound):
        return (torch.rand(shape, generator=g) * 2 - 1) * bound

    def mlp(n_in, n_out, init_w, heads=("last_fc",)):
        sd = OrderedDict()
        for i in range(n_layers):
            sd["fc%d.weight" % i], sd["fc%d.bias" % i] = u((H, n_in), 1 / math.sqrt(H)), torch.zeros(H)
            n_in = H
        for h in heads:
            sd[h + ".weight"] = u((n_out, H), init_w) * last_scale
            sd[h + ".bias"] = torch.zeros(n_out) if h == "last_fc" else u((n_out,), init_w)
        return sd

    critic = OrderedDict()
    for n in NETS:
        critic.update((n + "." + k, v) for k, v in mlp(Z if n == "vf" else Z + A, 1, 3e-3).items())
    return critic, mlp(P, A, 1e-3, ("last_fc", "last_fc_log_std"))


def mlp_forward(sd, prefix, x, heads=("last_fc",)):
    h = x
    for i in range(n_hidden(sd, prefix)):
        h = torch.relu(h @ sd["%sfc%d.weight" % (prefix, i)].t() + sd["%sfc%d.bias" % (prefix, i)])
    return [h @ sd[prefix + k + ".weight"].t() + sd[prefix + k + ".bias"] for k in heads]


def softplus(x):
    return torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))


def tanh_normal_log_prob(mean, log_std_raw, action):
    """distributions.py:339-354 with gaussian_policy.py:119-123; returns (logp [B], clamped log std)."""
    ls = torch.clamp(log_std_raw, -20.0, 2.0)
    v = torch.clamp(action, -0.999999, 0.999999)
    u = torch.log(1 + v) / 2 - torch.log(1 - v) / 2
    normal = (-0.5 * ((u - mean) / torch.exp(ls)) ** 2 - ls - 0.5 * math.log(2 * math.pi)).sum(1)
    log2 = float(torch.tensor(math.log(2.0), dtype=torch.float32))      # the reference's constant is an fp32 tensor at any precision
    return normal - 2.0 * (log2 - u - softplus(-2.0 * u)).sum(1), ls


def losses(critic, policy, batch, cfg=CFG):
    """-> dict(qf1_loss, qf2_loss, vf_loss, policy_loss, weights, adv, q_target, vf_err, raw_log_std); differentiable in the
    parameters.  batch: z, next_z, action, policy_input, rewards [B], terminals [B]."""
    z, nz, a, r, t = batch["z"], batch["next_z"], batch["action"], batch["rewards"].reshape(-1), batch["terminals"].reshape(-1)
    za = torch.cat([z, a], 1)
    q1, q2 = (mlp_forward(critic, n + ".", za)[0][:, 0] for n in ("qf1", "qf2"))
    with torch.no_grad():
        tq1, tq2 = (mlp_forward(critic, n + ".", za)[0][:, 0] for n in ("target_qf1", "target_qf2"))
        v_next = mlp_forward(critic, "vf.", nz)[0][:, 0]
    v = mlp_forward(critic, "vf.", z)[0][:, 0]
    q_target = (cfg["reward_scale"] * r + (1.0 - t) * cfg["discount"] * v_next).detach()
    q_pred = torch.min(tq1, tq2)
    vf_err = v - q_pred
    sign = (vf_err > 0).float()           # (fp32 in the reference at any precision: quantile and 1 - quantile are fp32-rounded)
    w = (1 - sign) * cfg["quantile"] + sign * (1 - cfg["quantile"])
    mean, raw_ls = mlp_forward(policy, "", batch["policy_input"], ("last_fc", "last_fc_log_std"))
    logp, _ = tanh_normal_log_prob(mean, raw_ls, a)
    adv = (q_pred - v).detach()
    exp_adv = torch.exp(adv / cfg["beta"])
    if cfg["clip_score"] is not None:
        exp_adv = torch.clamp(exp_adv, max=cfg["clip_score"])
    return dict(qf1_loss=((q1 - q_target) ** 2).mean(), qf2_loss=((q2 - q_target) ** 2).mean(), vf_loss=(w * vf_err ** 2).mean(),
                policy_loss=(-logp * exp_adv).mean(), weights=exp_adv, adv=adv, q_target=q_target, vf_err=vf_err.detach(),
                raw_log_std=raw_ls.detach(), exp_adv_unclipped=torch.exp(adv / cfg["beta"]))


def train(critic, policy, batches, dtype, cfg=CFG):
    """Runs one step per batch from the given state_dicts (not modified).  -> (step0: dict of the four losses, weights and
    `grad.<critic key>` / `grad.policy.<key>`;  final: (critic state_dict, policy state_dict) after the last step;  grads64: per step
    a dict of every trained parameter's gradient)."""
    critic = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(not k.startswith("target"))) for k, v in critic.items())
    policy = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in policy.items())
    trained = [v for k, v in critic.items() if not k.startswith("target")]
    opt_c = torch.optim.Adam(trained, lr=cfg["qf_lr"])
    opt_p = torch.optim.Adam(list(policy.values()), lr=cfg["policy_lr"], betas=(0.9, 0.999))
    step0, per_step = None, []
    for step, batch in enumerate(batches):
        batch = {k: v.to(dtype) for k, v in batch.items()}
        out = losses(critic, policy, batch, cfg)
        opt_c.zero_grad()
        (out["qf1_loss"] + out["qf2_loss"] + out["vf_loss"]).backward()
        opt_c.step()
        opt_p.zero_grad()
        out["policy_loss"].backward()
        opt_p.step()
        grads = {"grad." + k: v.grad.detach().clone() for k, v in critic.items() if v.grad is not None}
        grads.update(("grad.policy." + k, v.grad.detach().clone()) for k, v in policy.items())
        per_step.append(grads)
        if step == 0:
            step0 = {k: out[k].detach().clone() for k in ("qf1_loss", "qf2_loss", "vf_loss", "policy_loss", "weights")}
            step0.update(grads)
        if step % cfg["target_update_period"] == 0:
            with torch.no_grad():
                for n in ("qf1", "qf2"):
                    for k, v in critic.items():
                        if k.startswith(n + "."):
                            tgt = critic["target_" + k]
                            tgt.copy_(tgt * (1.0 - cfg["soft_target_tau"]) + v * cfg["soft_target_tau"])
    final = (OrderedDict((k, v.detach().clone()) for k, v in critic.items()), OrderedDict((k, v.detach().clone()) for k, v in policy.items()))
    return step0, final, per_step


def make_batch(B, Z, A, P, seed, terminals=False, scale=1.0, extreme_rows=(0, -1)):
    """A seeded batch; two of its rows hold an action component beyond +-0.999999 (+1 in the first, -1 in the second)."""
    g = torch.Generator().manual_seed(seed)
    action = (torch.rand(B, A, generator=g) * 2 - 1) * 0.98
    if extreme_rows:
        action[extreme_rows[0], 0], action[extreme_rows[1], A - 1] = 1.0, -1.0
    t = (torch.rand(B, generator=g) < 0.3).float() if terminals else torch.zeros(B)
    return dict(z=torch.randn(B, Z, generator=g) * scale, next_z=torch.randn(B, Z, generator=g) * scale, action=action,
                policy_input=torch.randn(B, P, generator=g) * scale, rewards=torch.randn(B, generator=g), terminals=t)
