"""Imagined returns of a policy trained on SLAC latents (SPEC.md N3j): from start states of a dataset, what discounted return does
`policy.pth` collect inside the model `latent.pth`?  No simulator is needed.

  python imagine_policy.py --data FILE --latent_dir DIR --policy_dir DIR --out imag.npz [--context 8] [--horizon 16]
                           [--windows 256] [--stride N] [--batch 256] [--discount 0.99] [--mean] [--seed 0] [--bf16]
                           [--fused_chain] [--bootstrap]

Takes up to --windows stretches of --context + --horizon transitions from the trajectories of --data (`s2p_amd.slac_predict.windows`),
filters the first --context + 1 frames of each with the posterior and, from z(context), (1) lets the deterministic policy (tanh of
its mean) act in the model for --horizon steps, (2) rolls the model under the dataset's recorded actions.  The policy's input type is
read off its obs_dim and printed: 288 is `latent_z` (the policy reads z); S * 256 + (S - 1) * A is `feature_action` (SPEC.md N3o: the
policy reads the last S encoder features and S - 1 actions, so every imagined step decodes z, quantises the frame to uint8 and encodes
it again; --context + 1 >= S is needed).
Prints mean +- standard error over the windows of the policy's imagined return, the model's return under the dataset's actions and
the dataset's true discounted reward sum over the same rows, and the mean |a| of the policy against the data.  --out holds those per
window (`policy_return`, `behaviour_return`, `data_return`; with --bootstrap also `bootstrap` and `policy_value` = return +
discount^H min(qf1, qf2)(z(H), pi(z(H))) from `critic.pth` in --policy_dir), the policy's `actions` [n,H,A] and `z` [n,H,288], and the
windows' `starts`.  --mean rolls the means (no noise anywhere); --fused_chain runs every chain as one launch (bitwise the same)."""
import argparse
import os

import numpy as np
import torch

from s2p_amd.latent_cli import add_chain_options, input_type_name, load_latent, need_device, net_shape, policy_input_type


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", required=True, help="dataset file (.npz / .hdf5) with image_observations, image_observations_tp1, actions, rewards, timeouts")
    ap.add_argument("--latent_dir", required=True, help="directory holding latent.pth")
    ap.add_argument("--policy_dir", required=True, help="directory holding policy.pth (and critic.pth for --bootstrap)")
    ap.add_argument("--out", required=True, help="write the per-window returns, the actions and z to this .npz")
    ap.add_argument("--context", type=int, default=8, help="transitions the posterior filters before the rollout starts")
    ap.add_argument("--horizon", type=int, default=16, help="imagined steps H")
    ap.add_argument("--windows", type=int, default=256, help="windows taken from the file, evenly spread")
    ap.add_argument("--stride", type=int, help="rows between window starts (default: context + horizon)")
    ap.add_argument("--batch", type=int, default=256, help="windows per device batch")
    ap.add_argument("--discount", type=float, default=0.99)
    ap.add_argument("--mean", action="store_true", help="roll the means: no noise in the posterior or the rollout")
    ap.add_argument("--seed", type=int, default=0)
    add_chain_options(ap, bf16_help="bf16 conv stack of the encoder", fused_chain="every chain as one launch (bitwise the same result)")
    ap.add_argument("--bootstrap", action="store_true", help="add discount^H min(qf1, qf2)(z(H), pi(z(H))) from critic.pth")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.context < 1:
        ap.error("--context >= 1")
    if a.windows < 1 or a.batch < 1 or (a.stride is not None and a.stride < 1):
        ap.error("--windows, --batch and --stride are at least 1")
    return a


def mean_se(x):
    x = np.asarray(x, dtype=np.float64)
    return float(x.mean()), float(x.std(ddof=1) / np.sqrt(x.size)) if x.size > 1 else 0.0


def main(argv=None):
    a = parse_args(argv)
    if a.horizon < 1:
        raise SystemExit("--horizon is at least 1")
    from s2p_amd.data import load_arrays
    from s2p_amd.offline_rl import CriticSLAC, Qfunction, TanhGaussianPolicy, Vfunction
    from s2p_amd.slac_imagine import behaviour, imagined_returns
    from s2p_amd.slac_predict import gather, windows
    data = load_arrays(a.data)
    try:
        starts = windows(data, a.context + a.horizon, a.stride, a.windows)
    except ValueError as e:
        raise SystemExit("%s: %s" % (a.data, e))
    sd = torch.load(os.path.join(a.policy_dir, "policy.pth"), map_location="cpu")
    hidden, obs_dim, A = net_shape(sd)
    if A != int(np.asarray(data["actions"]).shape[1]):
        raise SystemExit("policy.pth has %d actions, the dataset %d" % (A, int(np.asarray(data["actions"]).shape[1])))
    S = policy_input_type(obs_dim, A, a.context)
    print("policy.pth: input type %s, obs_dim %d" % (input_type_name(S), obs_dim))
    need_device("imagine_policy.py")
    torch.manual_seed(a.seed)
    torch.cuda.manual_seed(a.seed)
    policy = TanhGaussianPolicy(hidden_sizes=hidden, obs_dim=obs_dim, action_dim=A).load_state_dict(sd, strict=True)
    critic = None
    if a.bootstrap:
        csd = torch.load(os.path.join(a.policy_dir, "critic.pth"), map_location="cpu")
        qh, qin, _ = net_shape(csd, "qf1.")
        q = [Qfunction(hidden_sizes=qh, output_size=1, input_size=qin) for _ in range(4)]
        critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=qh, output_size=1, input_size=net_shape(csd, "vf.")[1]))
        critic.load_state_dict(csd, strict=True)
    latent = load_latent(a, (3, 100, 100), A)
    parts = {}
    for lo in range(0, len(starts), a.batch):
        st = starts[lo:lo + a.batch]
        frames, actions, _ = gather(data, st, a.context)
        im = imagined_returns(latent, policy, frames, actions, a.horizon, a.discount, critic, a.context, sample=not a.mean)
        be = behaviour(latent, data, st, a.context, a.horizon, a.discount, sample=not a.mean)
        row = dict(policy_return=im["returns"], behaviour_return=be["returns"], data_return=be["data_returns"], actions=im["actions"],
                   z=im["z"], data_actions=be["actions"])
        if critic is not None:
            row.update(bootstrap=im["bootstrap"], policy_value=im["value"])
        for k, v in row.items():
            parts.setdefault(k, []).append(v.cpu().numpy())
    res = {k: np.concatenate(v) for k, v in parts.items()}
    print("%d windows of %d + %d steps from %s, discount %g" % (len(starts), a.context, a.horizon, a.data, a.discount))
    names = [("policy_return", "policy, imagined return"), ("behaviour_return", "dataset actions, model return"),
             ("data_return", "dataset, true reward sum")] + ([("policy_value", "policy, return + bootstrap")] if critic is not None else [])
    for k, label in names:
        print("%-32s %12.5f +- %.5f" % ((label,) + mean_se(res[k])))
    print("mean |a|: policy %.4f, data %.4f" % (float(np.abs(res["actions"]).mean()), float(np.abs(res["data_actions"]).mean())))
    save = {k: v for k, v in res.items() if k != "data_actions"}
    save["starts"] = starts
    np.savez(a.out, **save)
    print("wrote", a.out)
    return save


if __name__ == "__main__":
    main()
