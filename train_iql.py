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
import os

import torch

from s2p_amd.slac_algo import UNCERTAINTY_TYPES

IQL_KWARGS = dict(discount=0.99, policy_lr=1e-4, qf_lr=3e-4, reward_scale=1, soft_target_tau=0.005, beta=1.0 / 10, quantile=0.7,
                  clip_score=100, target_update_period=2, slac_update_period=1)


def parse_args(argv=None, extend=None):
    """`extend(parser)` adds a caller's own options before parsing (train_cql.py shares these options)."""
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--real", required=True, help="dataset of real transitions (.npz, or .hdf5 with h5py)")
    ap.add_argument("--gen", help="generated dataset (all_state_1step_random_action) made from the real one")
    ap.add_argument("--uncertainty_type", choices=[t for t in UNCERTAINTY_TYPES if t], default=None)
    ap.add_argument("--uncertainty_penalty_lambda", type=float, default=0.0)
    ap.add_argument("--latent_dir", required=True, help="directory holding latent.pth")
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--freeze_slac", action="store_true", help="do not train the latent model along")
    ap.add_argument("--cache_features", action="store_true",
                    help="with --freeze_slac: encode every stored frame once and sample cached features, not frames")
    ap.add_argument("--fused_chain", action="store_true",
                    help="run the no-grad posterior chain of prepare_batch as one launch (bitwise the same result)")
    ap.add_argument("--fused_chain_grad", action="store_true",
                    help="run the posterior chain of update_latent as one launch forward and one backward (bitwise the same result)")
    ap.add_argument("--bf16_chain", action="store_true",
                    help="with --fused_chain: bf16 matrix-core compute inside the fused no-grad latent chain (SPEC.md N3m), independent of --bf16 and "
                         "--bf16_mlp: weights and LDS activations rounded to bf16, fp32 sums, heads and outputs; mixed precision, not the same numbers")
    ap.add_argument("--slac_policy_input_type", choices=["feature_action", "latent_z"], default="feature_action")
    ap.add_argument("--bf16", action="store_true", help="bf16 conv stacks of the latent model (the IQL networks stay fp32: see --bf16_mlp)")
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
    a = ap.parse_args(argv)
    if a.steps < 0 or a.batch_size < 1:
        ap.error("--steps >= 0 and --batch_size >= 1")
    if a.uncertainty_type and not a.gen:
        ap.error("--uncertainty_type applies to a --gen dataset")
    if a.bf16_chain and not a.fused_chain:
        ap.error("--bf16_chain needs --fused_chain: the bf16 compute mode exists only in the fused chain kernels")
    if a.cache_features and not a.freeze_slac:
        ap.error("--cache_features needs --freeze_slac: a feature is a constant of the run only while the encoder is not trained")
    return a


def policy_input_dim(a, action_dim, feature_dim=256, z_dim=288):
    """finetune_rl.py:204: S features and S - 1 actions, or the latent."""
    return a.num_sequences * feature_dim + (a.num_sequences - 1) * action_dim if a.slac_policy_input_type == "feature_action" else z_dim


def sample_form(a, algo):
    """The `frames` argument of `random_batch`: with --cache_features, build the feature table first and report its size and time."""
    if not a.cache_features:
        return None
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    algo.cache_features()
    torch.cuda.synchronize()
    t = algo.buffer.features
    print("feature table: %d rows x %d fp32 = %.1f MB, built in %.2f s" % (t.shape[0], t.shape[1], t.numel() * 4 / 1e6,
                                                                         time.perf_counter() - t0))
    return "features"


def main(argv=None):
    a = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("train_iql.py needs a HIP device (no CPU fallback)")
    from s2p_amd.data import load_arrays
    from s2p_amd.iql import CriticSLAC, IQLTrainer, Qfunction, TanhGaussianPolicy, Vfunction
    from s2p_amd.slac_algo import SlacAlgorithm
    real = load_arrays(a.real)
    gen = load_arrays(a.gen) if a.gen else None
    rows = len(real["actions"]) + (len(gen["actions"]) if gen else 0)
    C, A = real["image_observations"].shape[3], real["actions"].shape[1]
    algo = SlacAlgorithm((C,) + real["image_observations"].shape[1:3], (A,), 1, "cuda:0", a.seed, batch_size_sac=a.batch_size,
                         batch_size_latent=a.batch_size_latent, buffer_size=max(rows, 1), num_sequences=a.num_sequences,
                         dtype=torch.bfloat16 if a.bf16 else torch.float32, frame_capacity=2 * rows + a.num_sequences + 1,
                         fused_chain=a.fused_chain, fused_chain_grad=a.fused_chain_grad,
                         chain_compute="bf16" if a.bf16_chain else "fp32")
    algo.latent.load_state_dict(torch.load(os.path.join(a.latent_dir, "latent.pth"), map_location="cpu"), strict=True)
    algo.load_data_in_buffer(real)
    if gen is not None:
        algo.load_data_in_buffer(gen, data_num=len(gen["actions"]), uncertainty_type=a.uncertainty_type,
                                 uncertainty_penalty_lambda=a.uncertainty_penalty_lambda, generated_for_slac=True,
                                 data_mix_type="all_state_1step_random_action")
    print("buffer: %d windows (%d real)" % (len(algo.buffer), algo.buffer._real_n))
    if len(algo.buffer) == 0:
        raise SystemExit("no window of %d steps in the data" % a.num_sequences)
    Z, hid = 288, [a.hidden, a.hidden]
    q = [Qfunction(hidden_sizes=hid, output_size=1, input_size=Z + A) for _ in range(4)]
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=hid, output_size=1, input_size=Z))
    policy = TanhGaussianPolicy(hidden_sizes=hid, obs_dim=policy_input_dim(a, A), action_dim=A)
    trainer = IQLTrainer(None, policy, critic=critic, slac_algo=algo, freeze_slac=a.freeze_slac,
                         slac_policy_input_type=a.slac_policy_input_type, mlp_compute="bf16" if a.bf16_mlp else "fp32", **IQL_KWARGS)
    frames = sample_form(a, algo)
    for step in range(1, a.steps + 1):
        trainer.train_from_torch(algo.buffer.random_batch(a.batch_size, frames=frames))
        if step % a.log_every == 0 or step == a.steps:
            trainer.end_epoch(step)
            print("step %d  %s" % (step, "  ".join("%s %.4f" % kv for kv in trainer.eval_statistics.items())))
    os.makedirs(a.out, exist_ok=True)
    torch.save(critic.state_dict(), os.path.join(a.out, "critic.pth"))
    torch.save(policy.state_dict(), os.path.join(a.out, "policy.pth"))
    algo.save_model(a.out)
    print("wrote %s/critic.pth, policy.pth, encoder.pth and latent.pth" % a.out)


if __name__ == "__main__":
    main()
