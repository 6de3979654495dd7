"""Open-loop prediction from a trained SLAC latent model (SPEC.md N3i): filter `context` frames with the posterior, roll the
generative model forward on the next H actions alone (`LatentModel.predict`), decode, and score the predicted frames and rewards
against what happened.  `windows` picks the stretches of a dataset file this can be asked of; `open_loop` is one device batch."""
import numpy as np
import torch

from .metrics import image_metrics
from .slac import Z1, Z2


def windows(data, length, stride=None, limit=None):
    """Start rows i of runs of `length` transitions inside one trajectory of `data` (the on-disk schema: `timeouts`, and / or
    `terminals`, one flag per row).  A trajectory ends ON a flagged row and at the last row, so a window may END on a flagged row --
    its last frame is that row's `image_observations_tp1` -- but holds none in its rows i .. i+length-2.  Of a window:
    frames f(k) = image_observations[i+k], k < length, f(length) = image_observations_tp1[i+length-1]; a(k) = actions[i+k];
    r(k) = rewards[i+k].  Starts are `stride` rows apart from each trajectory's first row (default `length`: no overlap); `limit`
    keeps that many, evenly spread over the file.  -> int64 [n]; ValueError when the file holds no such window."""
    length = int(length)
    stride = length if stride is None else int(stride)
    if length < 1 or stride < 1 or (limit is not None and limit < 1):
        raise ValueError("length, stride and limit are at least 1")
    flags = [np.asarray(data[k]).reshape(-1).astype(bool) for k in ("timeouts", "terminals") if k in data]
    if not flags:
        raise ValueError("the dataset has neither `timeouts` nor `terminals`")
    end = np.logical_or.reduce(flags)
    n = end.shape[0]
    ends = np.flatnonzero(end)
    if n and (ends.size == 0 or ends[-1] != n - 1):
        ends = np.append(ends, n - 1)
    starts, first = [], 0
    for e in ends:
        starts.append(np.arange(first, e - length + 2, stride, dtype=np.int64))       # i + length - 1 <= e
        first = e + 1
    starts = np.concatenate(starts) if starts else np.zeros(0, dtype=np.int64)
    if starts.size == 0:
        raise ValueError("no trajectory of the dataset holds a window of %d steps" % length)
    if limit is not None and limit < starts.size:
        starts = starts[np.round(np.linspace(0, starts.size - 1, limit)).astype(np.int64)]
    return starts


def gather(data, starts, length):
    """The windows' frames uint8 [n,length+1,H,W,3], actions fp32 [n,length,A] and rewards fp32 [n,length] (numpy)."""
    rows = np.asarray(starts, dtype=np.int64)[:, None] + np.arange(length)[None]
    obs, tp1 = data["image_observations"], data["image_observations_tp1"]
    frames = np.concatenate([obs[rows], tp1[rows[:, -1]][:, None]], axis=1)
    actions = np.asarray(data["actions"], dtype=np.float32)[rows]
    rewards = np.asarray(data["rewards"], dtype=np.float32).reshape(len(obs))[rows]
    return frames, actions, rewards


def _nchw01(u8):
    """uint8 NHWC [..., H, W, 3] -> fp32 NCHW [n, 3, H, W] in [0, 1]."""
    x = u8.reshape(-1, *u8.shape[-3:]).permute(0, 3, 1, 2)
    return (x.float() / 255.0).contiguous()


def filter_context(latent, frames_u8_nhwc, actions, context, sample, posterior_noise, with_feat=False):
    """The filtering pass before a rollout: the encoder and `sample_posterior` see the first `context` + 1 frames and `context`
    actions (longer ones are cut).  `posterior_noise` [B,context+1,288] fixes the pass (None: drawn, or zeros when `sample` is False,
    so that a mean rollout is a function of its inputs alone).  -> z0 = z(context) [B,288] and the actions on the device; with
    `with_feat` also the encoder's features of the context frames [B,context+1,256] (what a `feature_action` window is cut from)."""
    dev = latent.device
    frames = torch.as_tensor(frames_u8_nhwc)
    actions = torch.as_tensor(actions).to(dev, torch.float32)
    if frames.dtype != torch.uint8 or frames.dim() != 5 or frames.shape[-1] != 3:
        raise ValueError("frames_u8_nhwc is uint8 [B,L+1,H,W,3]")
    B = frames.shape[0]
    if context < 1 or frames.shape[1] < context + 1 or actions.dim() != 3 or actions.shape[0] != B or actions.shape[1] < context:
        raise ValueError("frames [B,>=context+1,...] and actions [B,>=context,A] with context >= 1 are needed")
    feat = latent.encoder(frames[:, :context + 1].to(dev))
    if posterior_noise is None and not sample:
        posterior_noise = torch.zeros((B, context + 1, Z1 + Z2), dtype=torch.float32, device=dev)
    _, _, z1, z2 = latent.sample_posterior(feat, actions[:, :context], posterior_noise)
    z0 = torch.cat([z1[:, -1], z2[:, -1]], dim=-1)
    return (z0, actions, feat) if with_feat else (z0, actions)


@torch.no_grad()
def open_loop(latent, frames_u8_nhwc, actions, rewards=None, context=8, noise=None, sample=True, posterior_noise=None):
    """frames_u8_nhwc [B,L+1,100,100,3], actions [B,L,A], rewards [B,L] or None.  z0 = z(context) of `filter_context` (which takes
    `posterior_noise`); `predict(z0, actions[:, context:], noise, sample)` rolls the H = L - `context` remaining steps; the
    decoder's mean, clamped to [0, 1], is the predicted frame.  -> dict of device tensors:
    z0 [B,288], z1_mean, z1_std [B,H,32], z [B,H,288], frames [B,H,3,100,100], psnr, ssim [B,H] of the prediction and
    baseline_psnr, baseline_ssim [B,H] of repeating the last context frame (data_range 1; PSNR of identical frames is +inf),
    reward_mean, reward_std [B,H], and with `rewards` reward_abs_err [B,H]."""
    dev = latent.device
    frames, actions = torch.as_tensor(frames_u8_nhwc), torch.as_tensor(actions)
    if frames.dim() != 5 or actions.dim() != 3 or actions.shape[:2] != (frames.shape[0], frames.shape[1] - 1) or \
            frames.shape[1] - 1 <= context:
        raise ValueError("frames [B,L+1,...] and actions [B,L,A] with L > context >= 1 are needed")
    frames = frames.to(dev)
    z0, actions = filter_context(latent, frames, actions, context, sample, posterior_noise)
    B, L = actions.shape[:2]
    H = L - context
    future = actions[:, context:].contiguous()
    z1_mean, z1_std, z = latent.predict(z0, future, noise, sample)
    pred = latent.decoder(z)[0].clamp_(0.0, 1.0)
    truth = _nchw01(frames[:, context + 1:])
    last = _nchw01(frames[:, context:context + 1].expand(B, H, *frames.shape[2:]))
    psnr, ssim = image_metrics(pred.reshape(B * H, *pred.shape[2:]), truth, data_range=1.0)
    bpsnr, bssim = image_metrics(last, truth, data_range=1.0)
    r_mean, r_std = latent.predict_reward(z0, z, future)
    out = dict(z0=z0, z1_mean=z1_mean, z1_std=z1_std, z=z, frames=pred, psnr=psnr.reshape(B, H), ssim=ssim.reshape(B, H),
               baseline_psnr=bpsnr.reshape(B, H), baseline_ssim=bssim.reshape(B, H), reward_mean=r_mean, reward_std=r_std)
    if rewards is not None:
        rewards = torch.as_tensor(rewards).to(dev, torch.float32).reshape(B, L)
        out["reward_abs_err"] = (r_mean - rewards[:, context:]).abs()
    return out
