"""Imagined returns (SPEC.md N3j, N3o): filter `context` frames with the posterior, then let a trained policy act inside the latent
model for H steps and sum the reward head's means.  `imagined_returns` is one device batch of that; `behaviour` rolls the same start
states under the dataset's recorded actions (`LatentModel.predict`) and returns the dataset's own discounted reward sum beside the
model's.  `compare_rollouts` (`compare_policies`: its default modes) is `imagined_returns` for several policies on ONE filtering pass
and common random numbers, `paired` the statistics of such returns.  Both policy inputs: a `latent_z` policy (obs_dim 288) reads z(h) (`LatentModel.imagine`); a
`feature_action` policy reads the window of the last S encoder features and S - 1 actions, so its rollout decodes and re-encodes a
frame per step (`LatentModel.imagine_feature_action`)."""
import numpy as np
import torch

from .slac import FEAT, Z1, Z2
from .slac_predict import filter_context, gather


def discounted(rewards, discount):
    """sum_h discount^h rewards[:, h] -> fp64 [B], summed in fp64 on the device the rewards are on."""
    r = torch.as_tensor(rewards).to(torch.float64)
    g = float(discount) ** torch.arange(r.shape[1], dtype=torch.float64, device=r.device)
    return (r * g).sum(dim=1)


def policy_frames(latent, policy):
    """The input type of `policy` by its obs_dim: None for `latent_z` (288), else S of a `feature_action` input S 256 + (S - 1) A;
    ValueError where no integer S >= 2 fits.  A duck-typed policy without an obs_dim reads z."""
    P = getattr(policy, "obs_dim", None)
    if P is None or int(P) == Z1 + Z2:
        return None
    P, A = int(P), latent.action_dim
    S = latent.feature_action_frames(P, A)
    if S is None:
        raise ValueError("obs_dim %d is neither %d (latent_z) nor S * %d + (S - 1) * %d for an integer S >= 2 (feature_action)"
                         % (P, Z1 + Z2, FEAT, A))
    return S


def feature_action_window(feat, actions, context, S):
    """window(0) of a `feature_action` rollout, `create_feature_actions`' layout [f_0 .. f_{S-1} | a_0 .. a_{S-2}]: the last S of the
    context's features feat [B,context+1,256] and the last S - 1 of its `context` actions (the ones between those frames)."""
    if context + 1 < S:
        raise ValueError("a feature_action policy of %d frames needs context + 1 >= %d, not context %d" % (S, S, context))
    B = feat.shape[0]
    f = feat[:, context + 1 - S:context + 1].reshape(B, -1)
    a = actions[:, context - (S - 1):context].reshape(B, -1)
    return torch.cat([f, a], dim=-1).contiguous()


@torch.no_grad()
def imagined_returns(latent, policy, frames_u8_nhwc, actions, horizon, discount=0.99, critic=None, context=8, noise=None, sample=True,
                     posterior_noise=None, compute="fp32", quantize=True, keep_frames=False):
    """frames_u8_nhwc [B,context+1,100,100,3] and actions [B,context,A] (longer ones are cut): z0 = z(context) of the posterior;
    the rollout runs `horizon` steps with tanh(mean) of `policy` in the loop; `predict_reward` scores [z(h) | a(h) | z(h+1)];
    returns [B] = sum_h discount^h reward_mean[:, h], summed in fp64 on the device.  The rollout follows the policy's obs_dim: 288 is
    `imagine`; anything else is `imagine_feature_action` from the window of the last S context features and S - 1 context actions
    (context + 1 >= S, else ValueError), with `quantize` and `keep_frames` passed on.  With `critic` (a `CriticSLAC`): bootstrap =
    q_min(z(H), policy.act(its input at H)) -- z(H), or window(H) -- and value = returns + discount^H bootstrap.  -> dict of device
    tensors: z0, actions [B,H,A], z [B,H,288], z1_mean, z1_std, reward_mean, reward_std [B,H], returns fp64 [B], and bootstrap fp32 /
    value fp64 [B]; a `feature_action` policy adds obs [B,H (+1 with a critic),obs_dim] and, with `keep_frames`, frames_u8.
    `compute`: the rollout's mode, passed on to `imagine` ("bf16": SPEC.md N3n, needs `latent.fused_chain`; a ValueError for a
    `feature_action` policy, whose rollout has no fused chain)."""
    H = int(horizon)
    if H < 1:
        raise ValueError("horizon >= 1")
    S = _check_mode(latent, [policy], compute)[0]
    z0, actions, feat = filter_context(latent, frames_u8_nhwc, actions, int(context), sample, posterior_noise, with_feat=True)
    window = feature_action_window(feat, actions, int(context), S) if S is not None else None
    return _rollout(latent, policy, z0, H, discount, critic, noise, sample, compute, window, quantize, keep_frames)


def _check_mode(latent, policies, compute):
    """S (None: latent_z) of every policy; the bf16 chain mode with a `feature_action` policy among them is refused."""
    kinds = [policy_frames(latent, po) for po in policies]
    if compute == "bf16" and any(S is not None for S in kinds):
        raise ValueError("compute='bf16' is the fused latent_z imagination kernel's mode: a feature_action rollout runs the per-layer "
                         "prior step between its conv stacks and has no bf16 chain")
    return kinds


def _rollout(latent, policy, z0, H, discount, critic, noise, sample, compute, window=None, quantize=True, keep_frames=False):
    """What `imagined_returns` does from z0 on.  The default mode is today's call of `imagine`: a model without the keyword serves.
    `window` [B,obs_dim] (None: a `latent_z` policy) selects the `feature_action` rollout."""
    extra = {}
    if window is None:
        mode = {} if compute == "fp32" else dict(compute=compute)
        act, z1_mean, z1_std, z = latent.imagine(policy, z0, H, noise, sample, **mode)
    else:
        act, z1_mean, z1_std, z, obs, frames = latent.imagine_feature_action(policy, z0, window, H, noise, sample, quantize,
                                                                             final_obs=critic is not None, keep_frames=keep_frames)
        extra = dict(obs=obs, frames_u8=frames) if keep_frames else dict(obs=obs)
    r_mean, r_std = latent.predict_reward(z0, z, act)
    out = dict(z0=z0, actions=act, z=z, z1_mean=z1_mean, z1_std=z1_std, reward_mean=r_mean, reward_std=r_std,
               returns=discounted(r_mean, discount), **extra)
    if critic is not None:
        zH = z[:, -1].contiguous()
        out["bootstrap"] = critic.q_min(zH, policy.act(zH if window is None else out["obs"][:, H]))
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
    """`compare_rollouts` with the `feature_action` rollout in its default mode (quantised frames, none kept): the call as it was
    before `feature_action` policies could be ranked, with the same parameter list."""
    return compare_rollouts(latent, policies, frames_u8_nhwc, actions, horizon, discount, critics, context, noise, sample, posterior_noise,
                            compute)


@torch.no_grad()
def compare_rollouts(latent, policies, frames_u8_nhwc, actions, horizon, discount=0.99, critics=None, context=8, noise=None, sample=True,
                     posterior_noise=None, compute="fp32", quantize=True, keep_frames=False):
    """`imagined_returns` of every policy of `policies` from the SAME start states under the SAME rollout noise: one filtering pass
    (the conv stacks are its cost), then the rollout + `predict_reward` + `discounted` per policy.  `noise` [B,H,288] (None: drawn once,
    as `imagine` would draw it) is common to all, so two policies' returns differ by their actions alone and `paired` may difference
    them window by window.  `latent_z` and `feature_action` policies may be mixed: each takes its own rollout from the shared z0, the
    latter from its window of the shared context features.  `critics`: None, or one `CriticSLAC` per policy.  -> dict: z0 [B,288],
    returns fp64 [P,B], actions [P,B,H,A], reward_mean [P,B,H], and with critics bootstrap fp32 / value fp64 [P,B]; with `keep_frames`
    frames_u8: per policy its imagined uint8 frames, None for a `latent_z` policy.  With one policy each row 0 is bitwise
    `imagined_returns` of the same arguments (and, drawn, of the same generator state)."""
    H, policies = int(horizon), list(policies)
    if H < 1 or not policies:
        raise ValueError("horizon >= 1 and at least one policy")
    if critics is not None and len(critics) != len(policies):
        raise ValueError("one critic per policy")
    kinds = _check_mode(latent, policies, compute)
    z0, actions, feat = filter_context(latent, frames_u8_nhwc, actions, int(context), sample, posterior_noise, with_feat=True)
    windows = [feature_action_window(feat, actions, int(context), S) if S is not None else None for S in kinds]
    if noise is None and sample:
        noise = torch.randn((z0.shape[0], H, z0.shape[1]), dtype=torch.float32, device=latent.device)
    rows = [_rollout(latent, po, z0, H, discount, None if critics is None else critics[i], noise, sample, compute, windows[i], quantize,
                     keep_frames) for i, po in enumerate(policies)]
    out = dict(z0=z0)
    for k in ("returns", "actions", "reward_mean") + (("bootstrap", "value") if critics is not None else ()):
        out[k] = torch.stack([r[k] for r in rows])
    if keep_frames:
        out["frames_u8"] = [r.get("frames_u8") for r in rows]
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
