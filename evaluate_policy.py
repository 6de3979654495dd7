"""Evaluate a policy trained on SLAC latents (SPEC.md N3f): the stage after train_iql.py / train_cql.py.

  python evaluate_policy.py --latent_dir DIR --policy_dir DIR --env pkg.module:factory [--env_kwargs JSON]
                            --episodes 10 --max_path_length 1000 --num_envs 4
                            [--slac_policy_input_type feature_action|latent_z] [--reset_w_same_obs] [--bf16] [--out returns.npz]

Loads `latent.pth` from --latent_dir and `policy.pth` from --policy_dir (both strict), builds --num_envs environments and runs
--episodes deterministic episodes (tanh of the policy's mean, the reference's `MakeDeterministic`) in lock-step on one device batch.
--env names a callable `factory(**env_kwargs)` that returns an environment with `reset() -> uint8 [3,100,100]` and
`step(a) -> (obs, reward, done, info)`; `--env replay:PATH.npz` replays the trajectories of a dataset file instead (slot i starts at
trajectory i and moves on by --num_envs at every reset).  Prints the reference's `Average Returns` and the per-episode table, and
writes `returns`, `lengths`, `terminals` and `average_return` to --out."""
import argparse
import importlib
import json
import os
import types

import numpy as np
import torch

from s2p_amd.latent_cli import add_chain_options, check_chain_options, load_latent, need_device, net_shape


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--latent_dir", required=True, help="directory holding latent.pth")
    ap.add_argument("--policy_dir", required=True, help="directory holding policy.pth")
    ap.add_argument("--env", required=True, help="pkg.module:factory, or replay:PATH.npz")
    ap.add_argument("--env_kwargs", default="{}", help="JSON object handed to the factory")
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--max_path_length", type=int, default=1000)
    ap.add_argument("--num_envs", type=int, default=4)
    ap.add_argument("--slac_policy_input_type", choices=["feature_action", "latent_z"], default="feature_action")
    add_chain_options(ap, bf16_chain=True,
                      fused_chain="latent_z: run the posterior chain of every acting step as one launch (bitwise the same result)")
    ap.add_argument("--reset_w_same_obs", action="store_true", help="pad a new episode's window with its first frame, not with zero frames")
    add_chain_options(ap, bf16_help="bf16 conv stack of the encoder (the policy stays fp32)")
    ap.add_argument("--num_sequences", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0, help="seeds the posterior noise of latent_z")
    ap.add_argument("--out", help="write the per-episode arrays to this .npz")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    check_chain_options(ap, a)
    if a.episodes < 0 or a.max_path_length < 1 or not 1 <= a.num_envs <= 16:
        ap.error("--episodes >= 0, --max_path_length >= 1 and 1 <= --num_envs <= 16")
    return a


class ReplayCycle:
    """Slot `first` of `stride` slots over a dataset: every reset() moves on to the next trajectory of its share."""

    def __init__(self, arrays, first, stride):
        from s2p_amd.actor import ReplayEnv
        self.make, self.k, self.stride = (lambda k: ReplayEnv(arrays, k)), first - stride, stride
        self.n = self.make(0).num_trajectories

    def reset(self):
        self.k += self.stride
        self.env = self.make(self.k % self.n)
        return self.env.reset()

    def step(self, action):
        return self.env.step(action)


def make_envs(a):
    if a.env.startswith("replay:"):
        from s2p_amd.data import load_arrays
        arrays = load_arrays(a.env[len("replay:"):])
        return [ReplayCycle(arrays, i, a.num_envs) for i in range(a.num_envs)]
    module, _, name = a.env.partition(":")
    if not name:
        raise SystemExit("--env is pkg.module:factory or replay:PATH.npz")
    factory, kwargs = getattr(importlib.import_module(module), name), json.loads(a.env_kwargs)
    return [factory(**kwargs) for _ in range(a.num_envs)]


def main(argv=None):
    a = parse_args(argv)
    need_device("evaluate_policy.py")
    from s2p_amd.actor import SlacActor, run_episodes
    from s2p_amd.offline_rl import TanhGaussianPolicy
    torch.manual_seed(a.seed)
    torch.cuda.manual_seed(a.seed)
    sd = torch.load(os.path.join(a.policy_dir, "policy.pth"), map_location="cpu")
    hidden, obs_dim, A = net_shape(sd)
    policy = TanhGaussianPolicy(hidden_sizes=hidden, obs_dim=obs_dim, action_dim=A).load_state_dict(sd, strict=True)
    state_shape = (3, 100, 100)
    algo = types.SimpleNamespace(latent=load_latent(a, state_shape, A), state_shape=state_shape, action_shape=(A,), num_sequences=a.num_sequences)
    actor = SlacActor(policy, algo, a.num_envs, a.slac_policy_input_type, a.reset_w_same_obs)
    out = run_episodes(make_envs(a), actor, a.episodes, a.max_path_length)
    print("Average Returns %.6f" % out["average_return"])
    print("%8s %14s %8s %9s" % ("episode", "return", "length", "terminal"))
    for i, (r, n, t) in enumerate(zip(out["returns"], out["lengths"], out["terminals"])):
        print("%8d %14.6f %8d %9s" % (i, r, n, bool(t)))
    if a.out:
        np.savez(a.out, returns=out["returns"], lengths=out["lengths"], terminals=out["terminals"],
                 average_return=np.float64(out["average_return"]))
        print("wrote", a.out)
    return out


if __name__ == "__main__":
    main()
