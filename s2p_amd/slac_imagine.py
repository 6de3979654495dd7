"""Imagined returns (SPEC.md N3j): filter `context` frames with the posterior, then let a trained policy act inside the latent model
for H steps (`LatentModel.imagine`) and sum the reward head's means.  `imagined_returns` is one device batch of that; `behaviour`
rolls the same start states under the dataset's recorded actions (`LatentModel.predict`) and returns the dataset's own discounted
reward sum beside the model's.  `compare_policies` is `imagined_returns` for several policies on ONE filtering pass and common random
numbers, `paired` the statistics of such returns.  The `latent_z` policy input only: the policy reads z(h) [288]."""
import numpy as np
import torch

from .slac_predict import filter_context, gather


def discounted(rewards, discount):
    """sum_h discount^h rewards[:, h] -> fp64 [B], summed in fp64 on the device the rewards are on."""
    r = torch.as_tensor(rewards).to(torch.float64)
    g = float(discount) ** torch.arange(r.shape[1], dtype=torch.float64, device=r.device)
    return (r * g).sum(dim=1)


@torch.no_grad()
def imagined_returns(latent, policy, frames_u8_nhwc, actions, horizon, discount=0.99, critic=None, context=8, noise=None, sample=True,
                     posterior_noise=None, compute="fp32"):
    """frames_u8_nhwc [B,context+1,100,100,3] and actions [B,context,A] (longer ones are cut): z0 = z(context) of the posterior;
    `imagine` rolls `horizon` steps with tanh(mean) of `policy` in the loop; `predict_reward` scores [z(h) | a(h) | z(h+1)];
    returns [B] = sum_h discount^h reward_mean[:, h], summed in fp64 on the device.  With `critic` (a `CriticSLAC`):
    bootstrap = q_min(z(H), policy.act(z(H))) and value = returns + discount^H bootstrap.  -> dict of device tensors: z0, actions
    [B,H,A], z [B,H,288], z1_mean, z1_std, reward_mean, reward_std [B,H], returns fp64 [B], and bootstrap fp32 / value fp64 [B].
    `compute`: the rollout's mode, passed on to `imagine` ("bf16": SPEC.md N3n, needs `latent.fused_chain`)."""
    H = int(horizon)
    if H < 1:
        raise ValueError("horizon >= 1")
    z0, _ = filter_context(latent, frames_u8_nhwc, actions, int(context), sample, posterior_noise)
    return _rollout(latent, policy, z0, H, discount, critic, noise, sample, compute)


def _rollout(latent, policy, z0, H, discount, critic, noise, sample, compute):
    """What `imagined_returns` does from z0 on.  The default mode is today's call of `imagine`: a model without the keyword serves."""
    mode = {} if compute == "fp32" else dict(compute=compute)
    act, z1_mean, z1_std, z = latent.imagine(policy, z0, H, noise, sample, **mode)
    r_mean, r_std = latent.predict_reward(z0, z, act)
    out = dict(z0=z0, actions=act, z=z, z1_mean=z1_mean, z1_std=z1_std, reward_mean=r_mean, reward_std=r_std,
               returns=discounted(r_mean, discount))
    if critic is not None:
        zH = z[:, -1].contiguous()
        out["bootstrap"] = critic.q_min(zH, policy.act(zH))
        out["value"] = out["returns"] + float(discount) ** H * out["bootstrap"].to(torch.float64)
    return out


@torch.no_grad()
def behaviour(latent, data, starts, context, horizon, discount=0.99, noise=None, sample=True, posterior_noise=None):
    """The windows of `context` + `horizon` steps at rows `starts` of `data` (`slac_predict.windows` / `gather`): the same start
    states z(context) rolled under the dataset's recorded next `horizon` actions through `predict`.  -> dict: z0, actions [n,H,A]
    (the recorded ones), z, reward_mean, reward_std, returns fp64 [n] (the model's, under those actions) and data_returns fp64 [n] =
    sum_h discount^h rewards[start + context + h], the dataset's own."""
    context, H = int(context), int(horizon)
    if H < 1:
        raise ValueError("horizon >= 1")
    frames, actions, rewards = gather(data, starts, context + H)
    z0, actions = filter_context(latent, frames, actions, context, sample, posterior_noise)
    future = actions[:, context:].contiguous()
    _, _, z = latent.predict(z0, future, noise, sample)
    r_mean, r_std = latent.predict_reward(z0, z, future)
    data_r = torch.as_tensor(np.ascontiguousarray(rewards[:, context:])).to(latent.device)
    return dict(z0=z0, actions=future, z=z, reward_mean=r_mean, reward_std=r_std, returns=discounted(r_mean, discount),
                data_returns=discounted(data_r, discount))


@torch.no_grad()
def compare_policies(latent, policies, frames_u8_nhwc, actions, horizon, discount=0.99, critics=None, context=8, noise=None, sample=True,
                     posterior_noise=None, compute="fp32"):
    """`imagined_returns` of every policy of `policies` from the SAME start states under the SAME rollout noise: one filtering pass
    (the conv stacks are its cost), then `imagine` + `predict_reward` + `discounted` per policy.  `noise` [B,H,288] (None: drawn once,
    as `imagine` would draw it) is common to all, so two policies' returns differ by their actions alone and `paired` may difference
    them window by window.  `critics`: None, or one `CriticSLAC` per policy.  -> dict: z0 [B,288], returns fp64 [P,B], actions
    [P,B,H,A], reward_mean [P,B,H], and with critics bootstrap fp32 / value fp64 [P,B].  With one policy each row 0 is bitwise
    `imagined_returns` of the same arguments (and, drawn, of the same generator state)."""
    H, policies = int(horizon), list(policies)
    if H < 1 or not policies:
        raise ValueError("horizon >= 1 and at least one policy")
    if critics is not None and len(critics) != len(policies):
        raise ValueError("one critic per policy")
    z0, _ = filter_context(latent, frames_u8_nhwc, actions, int(context), sample, posterior_noise)
    if noise is None and sample:
        noise = torch.randn((z0.shape[0], H, z0.shape[1]), dtype=torch.float32, device=latent.device)
    rows = [_rollout(latent, po, z0, H, discount, None if critics is None else critics[i], noise, sample, compute)
            for i, po in enumerate(policies)]
    out = dict(z0=z0)
    for k in ("returns", "actions", "reward_mean") + (("bootstrap", "value") if critics is not None else ()):
        out[k] = torch.stack([r[k] for r in rows])
    return out


def paired(returns):
    """Statistics of returns [P, N] that share their windows and random numbers (`compare_policies`), in numpy fp64 -> dict:
    mean, se [P] (std(ddof=1) / sqrt(N); 0 for N == 1); order [P]: the policies by mean, descending, ties in the given order;
    best = order[0]; diff_mean, diff_se [P]: mean and standard error of the per-window differences returns[p] - returns[best]."""
    r = np.asarray(returns, dtype=np.float64)
    if r.ndim != 2 or r.shape[0] < 1 or r.shape[1] < 1:
        raise ValueError("returns is [P, N] with P, N >= 1")
    n = r.shape[1]
    se = lambda x: x.std(axis=1, ddof=1) / np.sqrt(n) if n > 1 else np.zeros(x.shape[0])
    mean = r.mean(axis=1)
    order = np.argsort(-mean, kind="stable")
    d = r - r[order[0]][None]
    return dict(mean=mean, se=se(r), order=order, best=int(order[0]), diff_mean=d.mean(axis=1), diff_se=se(d))
