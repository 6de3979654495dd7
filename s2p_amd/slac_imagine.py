"""Imagined returns (SPEC.md N3j): filter `context` frames with the posterior, then let a trained policy act inside the latent model
for H steps (`LatentModel.imagine`) and sum the reward head's means.  `imagined_returns` is one device batch of that; `behaviour`
rolls the same start states under the dataset's recorded actions (`LatentModel.predict`) and returns the dataset's own discounted
reward sum beside the model's.  The `latent_z` policy input only: the policy reads z(h) [288]."""
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
                     posterior_noise=None):
    """frames_u8_nhwc [B,context+1,100,100,3] and actions [B,context,A] (longer ones are cut): z0 = z(context) of the posterior;
    `imagine` rolls `horizon` steps with tanh(mean) of `policy` in the loop; `predict_reward` scores [z(h) | a(h) | z(h+1)];
    returns [B] = sum_h discount^h reward_mean[:, h], summed in fp64 on the device.  With `critic` (a `CriticSLAC`):
    bootstrap = q_min(z(H), policy.act(z(H))) and value = returns + discount^H bootstrap.  -> dict of device tensors: z0, actions
    [B,H,A], z [B,H,288], z1_mean, z1_std, reward_mean, reward_std [B,H], returns fp64 [B], and bootstrap fp32 / value fp64 [B]."""
    H = int(horizon)
    if H < 1:
        raise ValueError("horizon >= 1")
    z0, _ = filter_context(latent, frames_u8_nhwc, actions, int(context), sample, posterior_noise)
    act, z1_mean, z1_std, z = latent.imagine(policy, z0, H, noise, sample)
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
