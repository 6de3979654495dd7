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

from train_iql import parse_args as iql_args, policy_input_dim, sample_form

CQL_KWARGS = dict(discount=0.99, soft_target_tau=5e-3, policy_lr=1e-4, qf_lr=3e-4, reward_scale=1, use_automatic_entropy_tuning=True,
                  num_qs=2, min_q_version=3, with_lagrange=False, lagrange_thresh=-1.0, max_q_backup=False, slac_update_period=1)


def parse_args(argv=None):
    def more(ap):
        ap.description = __doc__
        ap.add_argument("--num_random", type=int, default=10, help="sampled actions per row and kind in the CQL term")
        ap.add_argument("--min_q_weight", type=float, default=5.0)
        ap.add_argument("--temp", type=float, default=1.0)
        ap.add_argument("--policy_eval_start", type=int, default=40000, help="steps of behaviour cloning before the SAC policy loss")
        ap.add_argument("--deterministic_backup", action="store_true", help="leave alpha * log_pi out of the backup")

    a = iql_args(argv, more)
    if a.num_random < 1 or not a.temp > 0:
        raise SystemExit("--num_random >= 1 and --temp > 0")
    return a


def main(argv=None):
    a = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("train_cql.py needs a HIP device (no CPU fallback)")
    from s2p_amd.cql import CQLTrainer, CriticSLAC, Qfunction, TanhGaussianPolicy, Vfunction
    from s2p_amd.data import load_arrays
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

    def networks():
        Z, hid = 288, [a.hidden, a.hidden]
        q = [Qfunction(hidden_sizes=hid, output_size=1, input_size=Z + A) for _ in range(4)]
        return (CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=hid, output_size=1, input_size=Z)),
                TanhGaussianPolicy(hidden_sizes=hid, obs_dim=policy_input_dim(a, A), action_dim=A))

    critic, policy = networks()
    gen_noise = torch.Generator(device="cuda:0").manual_seed(a.seed)
    trainer = CQLTrainer(None, policy, critic=critic, slac_algo=algo, freeze_slac=a.freeze_slac, slac_policy_input_type=a.slac_policy_input_type,
                         num_random=a.num_random, min_q_weight=a.min_q_weight, temp=a.temp, policy_eval_start=a.policy_eval_start,
                         deterministic_backup=a.deterministic_backup, generator=gen_noise, mlp_compute="bf16" if a.bf16_mlp else "fp32",
                         **CQL_KWARGS)
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
    critic2, policy2 = networks()                       # what was written loads strict and holds what was trained
    critic2.load_state_dict(torch.load(os.path.join(a.out, "critic.pth"), map_location="cpu"), strict=True)
    policy2.load_state_dict(torch.load(os.path.join(a.out, "policy.pth"), map_location="cpu"), strict=True)
    assert torch.equal(critic2.flat, critic.flat) and torch.equal(policy2.flat, policy.flat)
    algo.latent.load_state_dict(torch.load(os.path.join(a.out, "latent.pth"), map_location="cpu"), strict=True)
    print("wrote and reloaded %s/critic.pth, policy.pth, encoder.pth and latent.pth" % a.out)


if __name__ == "__main__":
    main()
