"""Rank policies trained on SLAC latents by their imagined return (SPEC.md N3j, N3n): which `policy.pth` of several collects the most
discounted reward inside the model `latent.pth`, and is the difference to the best more than noise?  No simulator is needed.

  python select_policy.py --data FILE --latent_dir DIR --policy_dirs DIR [DIR ...] --out sel.npz [--context 8] [--horizon 16]
                          [--windows 256] [--stride N] [--batch 256] [--discount 0.99] [--mean] [--seed 0] [--bf16] [--bootstrap]
                          [--fused_chain] [--bf16_chain] [--float_frames] [--frames FILE.npy]

The windows, the filtering pass and the rollout are those of imagine_policy.py, but the model is loaded once, every batch of windows is
encoded and filtered ONCE, and every policy rolls from the same start states under the same rollout noise
(`s2p_amd.slac_imagine.compare_rollouts`).  The returns of two policies on one window then differ by their actions alone, and the
table prints, per policy in the order of their means, mean +- standard error over the windows and the PAIRED difference to the best
policy +- its standard error (`s2p_amd.slac_imagine.paired`): a difference of several standard errors is a real one.  The model's
return under the dataset's recorded actions and the dataset's true discounted reward sum over the same rows are printed once.
--out holds `returns` [P,n], `order` [P], `starts` [n], `policy_dirs` [P], `behaviour_return` and `data_return` [n], and with
--bootstrap `value` [P,n] = return + discount^H min(qf1, qf2)(z(H), pi(z(H))) from each directory's `critic.pth` (the table then
ranks by it).  --mean rolls the means; --fused_chain runs every chain as one launch (bitwise the same); --bf16_chain, which needs
--fused_chain, multiplies in bf16 inside the filtering chain (SPEC.md N3m) AND the rollout (N3n): mixed precision, not the same numbers.
Each policy's input type is read off its obs_dim and printed: 288 is `latent_z`; S * 256 + (S - 1) * A is `feature_action` (SPEC.md
N3o: every imagined step decodes z, quantises the frame to uint8 and encodes it again; --context + 1 >= S is needed).  Both kinds may
be mixed.  For `feature_action` policies --float_frames keeps the decoded frame as floats clamped to [0,1] instead of quantising it,
and --frames writes the imagined uint8 frames [n,H-1,100,100,3] of the best policy; --bf16_chain with such a policy is refused (its
rollout has no fused chain)."""
import argparse
import os

import numpy as np
import torch

from s2p_amd.latent_cli import (add_chain_options, check_chain_options, input_type_name, load_latent, need_device, net_shape,
                                policy_input_type)


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", required=True, help="dataset file (.npz / .hdf5) with image_observations, image_observations_tp1, actions, rewards, timeouts")
    ap.add_argument("--latent_dir", required=True, help="directory holding latent.pth")
    ap.add_argument("--policy_dirs", required=True, nargs="+", help="directories holding policy.pth (and critic.pth for --bootstrap), one per policy")
    ap.add_argument("--out", required=True, help="write the per-window returns, the ranking and the windows to this .npz")
    ap.add_argument("--context", type=int, default=8, help="transitions the posterior filters before the rollout starts")
    ap.add_argument("--horizon", type=int, default=16, help="imagined steps H")
    ap.add_argument("--windows", type=int, default=256, help="windows taken from the file, evenly spread")
    ap.add_argument("--stride", type=int, help="rows between window starts (default: context + horizon)")
    ap.add_argument("--batch", type=int, default=256, help="windows per device batch")
    ap.add_argument("--discount", type=float, default=0.99)
    ap.add_argument("--mean", action="store_true", help="roll the means: no noise in the posterior or the rollout")
    ap.add_argument("--seed", type=int, default=0)
    add_chain_options(ap, bf16_help="bf16 conv stack of the encoder")
    ap.add_argument("--bootstrap", action="store_true", help="rank by return + discount^H min(qf1, qf2)(z(H), pi(z(H))) from each critic.pth")
    add_chain_options(ap, fused_chain="every chain as one launch (bitwise the same result)", bf16_chain=True)
    ap.add_argument("--float_frames", action="store_true", help="feature_action policies: the encoder sees the decoded frame clamped to [0,1], "
                    "not quantised to uint8")
    ap.add_argument("--frames", help="feature_action policies: write the imagined uint8 frames [n,H-1,100,100,3] of the best policy to this .npy")
    return ap


def parse_args(argv=None, parser=None):
    ap = parser if parser is not None else build_parser()
    a = ap.parse_args(argv)
    check_chain_options(ap, a)
    if a.context < 1:
        ap.error("--context >= 1")
    if a.windows < 1 or a.batch < 1 or (a.stride is not None and a.stride < 1):
        ap.error("--windows, --batch and --stride are at least 1")
    return a


def check_policy(number, directory, data_actions, context, ap, bf16_chain):
    """What needs no device of --policy_dirs entry `number`: its `policy.pth` read, refused as imagine_policy.py does, its input type
    printed (by its number: the table names the directories).  -> (state_dict, hidden sizes, obs_dim, action_dim)."""
    sd = torch.load(os.path.join(directory, "policy.pth"), map_location="cpu")
    hidden, obs_dim, A = net_shape(sd)
    if A != data_actions:
        raise SystemExit("%s: policy.pth has %d actions, the dataset %d" % (directory, A, data_actions))
    S = policy_input_type(obs_dim, A, context, "%s: policy.pth" % directory)
    if S is not None and bf16_chain:
        ap.error("--bf16_chain with the feature_action policy of %s: the bf16 mode exists only in the fused latent_z rollout kernel "
                 "(a feature_action rollout has no fused chain)" % directory)
    print("policy %d: input type %s, obs_dim %d" % (number, input_type_name(S), obs_dim))
    return sd, hidden, obs_dim, A


def load_policy(directory, checked, bootstrap):
    """(policy, critic or None) of one --policy_dirs entry on the device, from what `check_policy` read."""
    from s2p_amd.offline_rl import CriticSLAC, Qfunction, TanhGaussianPolicy, Vfunction
    sd, hidden, obs_dim, A = checked
    policy = TanhGaussianPolicy(hidden_sizes=hidden, obs_dim=obs_dim, action_dim=A).load_state_dict(sd, strict=True)
    critic = None
    if bootstrap:
        csd = torch.load(os.path.join(directory, "critic.pth"), map_location="cpu")
        qh, qin, _ = net_shape(csd, "qf1.")
        q = [Qfunction(hidden_sizes=qh, output_size=1, input_size=qin) for _ in range(4)]
        critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=qh, output_size=1, input_size=net_shape(csd, "vf.")[1]))
        critic.load_state_dict(csd, strict=True)
    return policy, critic


def main(argv=None):
    ap = build_parser()
    a = parse_args(argv, ap)
    if a.horizon < 1:
        raise SystemExit("--horizon is at least 1")
    from s2p_amd.data import load_arrays
    from s2p_amd.slac_imagine import behaviour, compare_rollouts, paired
    from s2p_amd.slac_predict import gather, windows
    data = load_arrays(a.data)
    try:
        starts = windows(data, a.context + a.horizon, a.stride, a.windows)
    except ValueError as e:
        raise SystemExit("%s: %s" % (a.data, e))
    A = int(np.asarray(data["actions"]).shape[1])
    checked = [check_policy(i + 1, d, A, a.context, ap, a.bf16_chain) for i, d in enumerate(a.policy_dirs)]
    need_device("select_policy.py")
    loaded = [load_policy(d, c, a.bootstrap) for d, c in zip(a.policy_dirs, checked)]
    policies, critics = [p for p, _ in loaded], [c for _, c in loaded] if a.bootstrap else None
    torch.manual_seed(a.seed)
    torch.cuda.manual_seed(a.seed)
    latent = load_latent(a, (3, 100, 100), A)
    compute = "bf16" if a.bf16_chain else "fp32"
    # the modes of the feature_action rollout; left out, compare_rollouts runs its defaults (quantised frames, none kept)
    fa_mode = dict(quantize=False) if a.float_frames else {}
    if a.frames:
        fa_mode["keep_frames"] = True
    parts, imagined = {}, {}
    for lo in range(0, len(starts), a.batch):
        st = starts[lo:lo + a.batch]
        frames, actions, _ = gather(data, st, a.context)
        cp = compare_rollouts(latent, policies, frames, actions, a.horizon, a.discount, critics, a.context, sample=not a.mean, compute=compute,
                              **fa_mode)
        if a.frames:
            for p, fr in enumerate(cp["frames_u8"]):
                if fr is not None:
                    imagined.setdefault(p, []).append(fr[:, :a.horizon - 1].cpu().numpy())
        be = behaviour(latent, data, st, a.context, a.horizon, a.discount, sample=not a.mean)
        row = dict(returns=cp["returns"], behaviour_return=be["returns"], data_return=be["data_returns"])
        if a.bootstrap:
            row["value"] = cp["value"]
        for k, v in row.items():
            parts.setdefault(k, []).append(v.cpu().numpy())
    res = {k: np.concatenate(v, axis=-1) for k, v in parts.items()}
    score = "value" if a.bootstrap else "returns"
    st = paired(res[score])
    n = len(starts)
    print("%d windows of %d + %d steps from %s, discount %g, %s rollout; ranked by the imagined %s" %
          (n, a.context, a.horizon, a.data, a.discount, compute, "return + bootstrap" if a.bootstrap else "return"))
    print("%4s  %12s    %-9s  %12s    %-9s  %s" % ("rank", "mean", "SE", "to the best", "SE", "policy"))
    for rank, p in enumerate(st["order"]):
        print("%4d  %12.5f +- %-9.5f  %12.5f +- %-9.5f  %s" % (rank + 1, st["mean"][p], st["se"][p], st["diff_mean"][p], st["diff_se"][p],
                                                              a.policy_dirs[p]))
    for k, label in (("behaviour_return", "dataset actions, model return"), ("data_return", "dataset, true reward sum")):
        x = res[k].astype(np.float64)
        print("%-32s %12.5f +- %.5f" % (label, x.mean(), x.std(ddof=1) / np.sqrt(n) if n > 1 else 0.0))
    save = dict(res, order=st["order"], starts=starts, policy_dirs=np.array(a.policy_dirs))
    np.savez(a.out, **save)
    print("wrote", a.out)
    if a.frames:
        best = int(st["order"][0])
        if best in imagined:
            np.save(a.frames, np.concatenate(imagined[best]))
            print("wrote", a.frames, "(the imagined frames of %s)" % a.policy_dirs[best])
        else:
            print("--frames: the best policy, %s, is a latent_z policy and imagines no frames" % a.policy_dirs[best])
    return save


if __name__ == "__main__":
    main()
