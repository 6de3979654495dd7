"""Train the SLAC latent model on real (and generated) frames from the device-resident replay buffer (SPEC.md N3c).

  python train_latent.py --real FILE [--gen FILE --uncertainty_type T --uncertainty_penalty_lambda L] --steps N --out DIR
                         [--bf16] [--seed S] [--fused_chain_grad]

Loads the file(s) as the reference's `load_data_in_buffer` does (`rlkit/torch/slac/algo.py:154-416`), runs `update_latent` N times
and writes `encoder.pth` / `latent.pth` with the reference's keys.  --fused_chain_grad runs the posterior chain of every update as
one launch forward and one launch backward instead of 8 per time step and direction (SPEC.md N3k; the same numbers, bit for bit)."""
import argparse

from s2p_amd.data import load_arrays
from s2p_amd.latent_cli import add_chain_options, add_dataset_options, build_algo, need_device


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    add_dataset_options(ap)
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--out", required=True)
    add_chain_options(ap, bf16_help="bf16 conv stacks (the Gaussian heads stay fp32)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--num_sequences", type=int, default=8)
    ap.add_argument("--log_every", type=int, default=100)
    add_chain_options(ap, fused_chain_grad="run the posterior chain of every update as one launch forward and one backward (bitwise the same result)")
    return ap


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    need_device("train_latent.py")
    algo = build_algo(a, load_arrays(a.real), load_arrays(a.gen) if a.gen else None, frames_stored=True, batch_size_latent=a.batch_size)
    for step in range(1, a.steps + 1):
        kld, image, reward = algo.update_latent()
        if step % a.log_every == 0 or step == a.steps:
            print("step %d  loss_kld %.4f  loss_image %.4f  loss_reward %.4f" % (step, float(kld), float(image), float(reward)))
    algo.save_model(a.out)
    print("wrote %s/encoder.pth and latent.pth" % a.out)


if __name__ == "__main__":
    main()
