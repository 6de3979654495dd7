"""Train the SLAC latent model on real (and generated) frames from the device-resident replay buffer (SPEC.md N3c).

  python train_latent.py --real FILE [--gen FILE --uncertainty_type T --uncertainty_penalty_lambda L] --steps N --out DIR
                         [--bf16] [--seed S] [--fused_chain_grad]

Loads the file(s) as the reference's `load_data_in_buffer` does (`rlkit/torch/slac/algo.py:154-416`), runs `update_latent` N times
and writes `encoder.pth` / `latent.pth` with the reference's keys.  --fused_chain_grad runs the posterior chain of every update as
one launch forward and one launch backward instead of 8 per time step and direction (SPEC.md N3k; the same numbers, bit for bit)."""
import argparse

import torch

from s2p_amd.data import load_arrays
from s2p_amd.slac_algo import UNCERTAINTY_TYPES, SlacAlgorithm


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--real", required=True, help="dataset of real transitions (.npz, or .hdf5 with h5py)")
    ap.add_argument("--gen", help="generated dataset (all_state_1step_random_action) made from the real one")
    ap.add_argument("--uncertainty_type", choices=[t for t in UNCERTAINTY_TYPES if t], default=None)
    ap.add_argument("--uncertainty_penalty_lambda", type=float, default=0.0)
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--bf16", action="store_true", help="bf16 conv stacks (the Gaussian heads stay fp32)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--num_sequences", type=int, default=8)
    ap.add_argument("--log_every", type=int, default=100)
    ap.add_argument("--fused_chain_grad", action="store_true",
                    help="run the posterior chain of every update as one launch forward and one backward (bitwise the same result)")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("train_latent.py needs a HIP device (no CPU fallback)")
    real = load_arrays(a.real)
    gen = load_arrays(a.gen) if a.gen else None
    rows = len(real["actions"]) + (len(gen["actions"]) if gen else 0)
    C = real["image_observations"].shape[3]
    # every window stores at most one new frame beyond its episode's reset frame; the generated file stores its own copy of the
    # observations it windows over
    algo = SlacAlgorithm((C,) + real["image_observations"].shape[1:3], (real["actions"].shape[1],), 1, "cuda:0", a.seed,
                         batch_size_latent=a.batch_size, buffer_size=max(rows, 1), num_sequences=a.num_sequences,
                         dtype=torch.bfloat16 if a.bf16 else torch.float32, frame_capacity=2 * rows + a.num_sequences + 1,
                         fused_chain_grad=a.fused_chain_grad)
    algo.load_data_in_buffer(real)
    if gen is not None:
        algo.load_data_in_buffer(gen, data_num=len(gen["actions"]), uncertainty_type=a.uncertainty_type,
                                 uncertainty_penalty_lambda=a.uncertainty_penalty_lambda, generated_for_slac=True,
                                 data_mix_type="all_state_1step_random_action")
    print("buffer: %d windows (%d real), %d frames stored" % (len(algo.buffer), algo.buffer._real_n, algo.buffer._head))
    if len(algo.buffer) == 0:
        raise SystemExit("no window of %d steps in the data" % a.num_sequences)
    for step in range(1, a.steps + 1):
        kld, image, reward = algo.update_latent()
        if step % a.log_every == 0 or step == a.steps:
            print("step %d  loss_kld %.4f  loss_image %.4f  loss_reward %.4f" % (step, float(kld), float(image), float(reward)))
    algo.save_model(a.out)
    print("wrote %s/encoder.pth and latent.pth" % a.out)


if __name__ == "__main__":
    main()
