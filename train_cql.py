"""Train CQL on SLAC latents from the device-resident replay buffer (SPEC.md N3e): the other last stage of the S2P pipeline, the
counterpart of the reference's `run_cql_image.sh`.

  python train_cql.py --real FILE [--gen FILE --uncertainty_type T --uncertainty_penalty_lambda L] --latent_dir DIR --steps N
                      --out DIR [--freeze_slac [--cache_features]] [--slac_policy_input_type feature_action|latent_z] [--bf16]
                      [--bf16_mlp] [--fused_chain] [--fused_chain_grad] [--bf16_chain] [--seed S]
                      [--num_random R] [--min_q_weight W] [--temp T] [--policy_eval_start E] [--deterministic_backup]

Loads `latent.pth` from --latent_dir (written by train_latent.py), fills the buffer as the reference's `load_data_in_buffer` does,
runs `CQLTrainer.train_from_torch` N times in the shipped configuration (`examples/iql/mujoco_finetune.py:120-143`), writes
`critic.pth` / `policy.pth` with the reference's keys plus `encoder.pth` / `latent.pth`, and reloads what it wrote.  --bf16_mlp runs
the wide layers of the critics and the policy on the bf16 matrix cores (SPEC.md N3l); the written files are fp32 as always."""
import os

import torch

from s2p_amd.latent_cli import build_algo, load_latent_pth, need_device, offline_networks, run_offline
from train_iql import build_parser as iql_parser, parse_args as iql_args

CQL_KWARGS = dict(discount=0.99, soft_target_tau=5e-3, policy_lr=1e-4, qf_lr=3e-4, reward_scale=1, use_automatic_entropy_tuning=True,
                  num_qs=2, min_q_version=3, with_lagrange=False, lagrange_thresh=-1.0, max_q_backup=False, slac_update_period=1)


def _more(ap):
    ap.description = __doc__
    ap.add_argument("--num_random", type=int, default=10, help="sampled actions per row and kind in the CQL term")
    ap.add_argument("--min_q_weight", type=float, default=5.0)
    ap.add_argument("--temp", type=float, default=1.0)
    ap.add_argument("--policy_eval_start", type=int, default=40000, help="steps of behaviour cloning before the SAC policy loss")
    ap.add_argument("--deterministic_backup", action="store_true", help="leave alpha * log_pi out of the backup")


def build_parser():
    return iql_parser(_more)


def parse_args(argv=None):
    a = iql_args(argv, _more)
    if a.num_random < 1 or not a.temp > 0:
        raise SystemExit("--num_random >= 1 and --temp > 0")
    return a


def main(argv=None):
    a = parse_args(argv)
    need_device("train_cql.py")
    from s2p_amd.cql import CQLTrainer
    from s2p_amd.data import load_arrays
    algo = build_algo(a, load_arrays(a.real), load_arrays(a.gen) if a.gen else None, batch_size_sac=a.batch_size,
                      batch_size_latent=a.batch_size_latent)
    critic, policy = offline_networks(a, algo.action_shape[0])
    gen_noise = torch.Generator(device="cuda:0").manual_seed(a.seed)
    trainer = CQLTrainer(None, policy, critic=critic, slac_algo=algo, freeze_slac=a.freeze_slac, slac_policy_input_type=a.slac_policy_input_type,
                         num_random=a.num_random, min_q_weight=a.min_q_weight, temp=a.temp, policy_eval_start=a.policy_eval_start,
                         deterministic_backup=a.deterministic_backup, generator=gen_noise, mlp_compute="bf16" if a.bf16_mlp else "fp32",
                         **CQL_KWARGS)
    run_offline(a, algo, trainer, critic, policy)
    critic2, policy2 = offline_networks(a, algo.action_shape[0])      # what was written loads strict and holds what was trained
    critic2.load_state_dict(torch.load(os.path.join(a.out, "critic.pth"), map_location="cpu"), strict=True)
    policy2.load_state_dict(torch.load(os.path.join(a.out, "policy.pth"), map_location="cpu"), strict=True)
    assert torch.equal(critic2.flat, critic.flat) and torch.equal(policy2.flat, policy.flat)
    load_latent_pth(algo.latent, a.out)
    print("wrote and reloaded %s/critic.pth, policy.pth, encoder.pth and latent.pth" % a.out)


if __name__ == "__main__":
    main()
