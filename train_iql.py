"""Train IQL on SLAC latents from the device-resident replay buffer (SPEC.md N3d): the last stage of the S2P pipeline.

  python train_iql.py --real FILE [--gen FILE --uncertainty_type T --uncertainty_penalty_lambda L] --latent_dir DIR --steps N
                      --out DIR [--freeze_slac [--cache_features]] [--slac_policy_input_type feature_action|latent_z] [--bf16]
                      [--bf16_mlp] [--fused_chain] [--fused_chain_grad] [--bf16_chain] [--seed S]

Loads `latent.pth` from --latent_dir (written by train_latent.py), fills the buffer as the reference's `load_data_in_buffer` does,
runs `IQLTrainer.train_from_torch` N times in the shipped configuration (`examples/iql/mujoco_finetune.py:91-119`) and writes
`critic.pth` / `policy.pth` with the reference's keys, plus `encoder.pth` / `latent.pth`.  With --freeze_slac the encoder never
changes: --cache_features encodes every stored frame once and samples cached features (SPEC.md N3g).  --fused_chain runs the
no-grad posterior chain of every step's `prepare_batch` as one launch (SPEC.md N3h; the same numbers, bit for bit), --fused_chain_grad
the chain that `update_latent` trains through as one launch forward and one backward (SPEC.md N3k; bit for bit again).
--bf16_mlp runs the wide layers of the IQL networks on the bf16 matrix cores (SPEC.md N3l): mixed precision, not the same numbers;
the weights, Adam and the written files stay fp32.  --bf16_chain (with --fused_chain) does the same inside the fused no-grad posterior
chain (SPEC.md N3m): bf16 operands, fp32 sums, heads and latents."""
import argparse

from s2p_amd.latent_cli import (add_chain_options, add_dataset_options, build_algo, check_chain_options, need_device, offline_networks,
                                policy_input_dim, run_offline, sample_form)  # noqa: F401  (policy_input_dim, sample_form: re-exported)

IQL_KWARGS = dict(discount=0.99, policy_lr=1e-4, qf_lr=3e-4, reward_scale=1, soft_target_tau=0.005, beta=1.0 / 10, quantile=0.7,
                  clip_score=100, target_update_period=2, slac_update_period=1)


def build_parser(extend=None):
    """`extend(parser)` adds a caller's own options (train_cql.py shares these options)."""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    add_dataset_options(ap)
    ap.add_argument("--latent_dir", required=True, help="directory holding latent.pth")
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--freeze_slac", action="store_true", help="do not train the latent model along")
    ap.add_argument("--cache_features", action="store_true",
                    help="with --freeze_slac: encode every stored frame once and sample cached features, not frames")
    add_chain_options(ap, bf16_chain=True,
                      fused_chain="run the no-grad posterior chain of prepare_batch as one launch (bitwise the same result)",
                      fused_chain_grad="run the posterior chain of update_latent as one launch forward and one backward (bitwise the same result)")
    ap.add_argument("--slac_policy_input_type", choices=["feature_action", "latent_z"], default="feature_action")
    add_chain_options(ap, bf16_help="bf16 conv stacks of the latent model (the IQL networks stay fp32: see --bf16_mlp)")
    ap.add_argument("--bf16_mlp", action="store_true",
                    help="bf16 matrix-core compute for the wide layers of the critics, vf and the policy, independent of --bf16: operands "
                         "rounded to bf16 as a tile loads them, fp32 sums, fp32 master weights, heads and Adam; the written critic.pth / "
                         "policy.pth are fp32 as always")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--batch_size_latent", type=int, default=32)
    ap.add_argument("--num_sequences", type=int, default=8)
    ap.add_argument("--hidden", type=int, default=1024, help="width of the two hidden layers of every IQL network")
    ap.add_argument("--log_every", type=int, default=100)
    if extend is not None:
        extend(ap)
    return ap


def parse_args(argv=None, extend=None):
    ap = build_parser(extend)
    a = ap.parse_args(argv)
    if a.steps < 0 or a.batch_size < 1:
        ap.error("--steps >= 0 and --batch_size >= 1")
    if a.uncertainty_type and not a.gen:
        ap.error("--uncertainty_type applies to a --gen dataset")
    check_chain_options(ap, a)
    if a.cache_features and not a.freeze_slac:
        ap.error("--cache_features needs --freeze_slac: a feature is a constant of the run only while the encoder is not trained")
    return a


def main(argv=None):
    a = parse_args(argv)
    need_device("train_iql.py")
    from s2p_amd.data import load_arrays
    from s2p_amd.iql import IQLTrainer
    algo = build_algo(a, load_arrays(a.real), load_arrays(a.gen) if a.gen else None, batch_size_sac=a.batch_size,
                      batch_size_latent=a.batch_size_latent)
    critic, policy = offline_networks(a, algo.action_shape[0])
    trainer = IQLTrainer(None, policy, critic=critic, slac_algo=algo, freeze_slac=a.freeze_slac,
                         slac_policy_input_type=a.slac_policy_input_type, mlp_compute="bf16" if a.bf16_mlp else "fp32", **IQL_KWARGS)
    run_offline(a, algo, trainer, critic, policy)
    print("wrote %s/critic.pth, policy.pth, encoder.pth and latent.pth" % a.out)


if __name__ == "__main__":
    main()
