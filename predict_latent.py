"""Open-loop prediction from a trained SLAC latent model (SPEC.md N3i): which frames and rewards does `latent.pth` predict for the
next H actions after `context` frames it has seen, and how far are they from what happened?

  python predict_latent.py --data FILE --latent_dir DIR --out pred.npz [--context 8] [--horizon 8] [--windows 64] [--stride N]
                           [--batch 64] [--mean] [--seed 0] [--bf16] [--fused_chain] [--bf16_chain] [--frames]

Takes up to --windows stretches of --context + --horizon transitions from the trajectories of --data (`s2p_amd.slac_predict.windows`;
starts --stride rows apart, default no overlap), filters the first --context + 1 frames of each with the posterior, rolls the
generative model forward on the remaining actions alone and decodes.  Prints, per horizon step, the mean PSNR / SSIM of the predicted
frame and of the copy-the-last-context-frame baseline against the true frame, and the mean |predicted - true reward|.  --out holds
those columns (`psnr`, `ssim`, `baseline_psnr`, `baseline_ssim`, `reward_abs_err`, each [H]), the per-window values behind them
(`window_*` [n,H]), `reward_mean`, `reward_std` [n,H], `z` [n,H,288] and the windows' `starts`; with --frames also the predicted
`frames` as uint8 [n,H,100,100,3].  --mean rolls the means (no noise anywhere); --fused_chain runs every chain as one launch
(bitwise the same result); --bf16_chain gives those launches bf16 operands (SPEC.md N3m: mixed precision, not the same numbers)."""
import argparse

import numpy as np
import torch

from s2p_amd.latent_cli import add_chain_options, check_chain_options, load_latent, need_device

COLUMNS = ("psnr", "ssim", "baseline_psnr", "baseline_ssim", "reward_abs_err")


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", required=True, help="dataset file (.npz / .hdf5) with image_observations, image_observations_tp1, actions, rewards, timeouts")
    ap.add_argument("--latent_dir", required=True, help="directory holding latent.pth")
    ap.add_argument("--out", required=True, help="write the tables and z to this .npz")
    ap.add_argument("--context", type=int, default=8, help="transitions the posterior filters before the rollout starts")
    ap.add_argument("--horizon", type=int, default=8, help="open-loop steps H")
    ap.add_argument("--windows", type=int, default=64, help="windows taken from the file, evenly spread")
    ap.add_argument("--stride", type=int, help="rows between window starts (default: context + horizon)")
    ap.add_argument("--batch", type=int, default=64, help="windows per device batch")
    ap.add_argument("--mean", action="store_true", help="roll the means: no noise in the posterior or the rollout")
    ap.add_argument("--seed", type=int, default=0)
    add_chain_options(ap, bf16_help="bf16 conv stacks of the encoder and the decoder", bf16_chain=True,
                      fused_chain="posterior and prior chain as one launch each (bitwise the same result)")
    ap.add_argument("--frames", action="store_true", help="also write the predicted frames")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    check_chain_options(ap, a)
    if a.horizon < 1 or a.context < 1:
        ap.error("--horizon >= 1 and --context >= 1")
    if a.windows < 1 or a.batch < 1 or (a.stride is not None and a.stride < 1):
        ap.error("--windows, --batch and --stride are at least 1")
    return a


def main(argv=None):
    a = parse_args(argv)
    need_device("predict_latent.py")
    from s2p_amd.data import load_arrays
    from s2p_amd.slac_predict import gather, open_loop, windows
    data = load_arrays(a.data)
    length = a.context + a.horizon
    try:
        starts = windows(data, length, a.stride, a.windows)
    except ValueError as e:
        raise SystemExit("%s: %s" % (a.data, e))
    torch.manual_seed(a.seed)
    torch.cuda.manual_seed(a.seed)
    latent = load_latent(a, (3, 100, 100), int(np.asarray(data["actions"]).shape[1]))
    keep = ("z", "reward_mean", "reward_std") + COLUMNS + (("frames",) if a.frames else ())
    parts = {k: [] for k in keep}
    for lo in range(0, len(starts), a.batch):
        frames, actions, rewards = gather(data, starts[lo:lo + a.batch], length)
        out = open_loop(latent, frames, actions, rewards, context=a.context, sample=not a.mean)
        for k in keep:
            v = out[k]
            if k == "frames":
                v = (v * 255.0).round_().to(torch.uint8).permute(0, 1, 3, 4, 2)
            parts[k].append(v.cpu().numpy())
    res = {k: np.concatenate(v) for k, v in parts.items()}
    table = {k: res[k].astype(np.float64).mean(axis=0) for k in COLUMNS}
    print("%d windows of %d + %d steps from %s" % (len(starts), a.context, a.horizon, a.data))
    print("%4s %10s %10s %14s %14s %16s" % ("h", "psnr", "ssim", "baseline_psnr", "baseline_ssim", "|reward error|"))
    for h in range(a.horizon):
        print("%4d %10.4f %10.6f %14.4f %14.6f %16.6f" % ((h + 1,) + tuple(table[k][h] for k in COLUMNS)))
    save = dict(table, starts=starts, z=res["z"], reward_mean=res["reward_mean"], reward_std=res["reward_std"])
    save.update({"window_" + k: res[k] for k in COLUMNS})
    if a.frames:
        save["frames"] = res["frames"]
    np.savez(a.out, **save)
    print("wrote", a.out)
    return save


if __name__ == "__main__":
    main()
