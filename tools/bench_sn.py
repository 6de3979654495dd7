"""Cost of the opt-in spectral normalization (SPEC.md D5s) at the bs-64 / 84x84 training shapes, in one process on one box:
  * the SN launches of each network: one training refresh (power iteration + W / sigma repack) and one gradient projection;
  * one train iteration (G step + D step) with the default options and with --norm_G spectralmatinstance --norm_D spectralinstance,
    eager and replayed from hipGraph segments.
Prints one JSON line.  usage: python tools/bench_sn.py [--steps 50] [--warmup 10]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from s2p_amd.options.train_options import TrainOptions  # noqa: E402
from s2p_amd.stepgraph import StepGraph  # noqa: E402
from s2p_amd.trainers.pix2pix_trainer import Pix2PixTrainer  # noqa: E402

SN = ["--norm_G", "spectralmatinstance", "--norm_D", "spectralinstance"]


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def trainer(extra, bs):
    opt = TrainOptions().parse(["--env_type", "cheetah", "--batchSize", str(bs), "--precision", "bf16", "--gpu_ids", "0",
                                "--checkpoints_dir", "/tmp/bench_sn"] + extra, quiet=True)
    torch.manual_seed(0)
    return Pix2PixTrainer(opt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    data = {k: t.cuda() for k, t in (("prev_image", torch.rand(a.batch, 3, 84, 84, generator=g) * 2 - 1),
                                      ("state", torch.randn(a.batch, 17, generator=g)),
                                      ("image", torch.rand(a.batch, 3, 84, 84, generator=g) * 2 - 1))}
    out = dict(batch=a.batch, steps=a.steps)
    for tag, extra in (("default", []), ("sn", SN)):
        tr = trainer(extra, a.batch)
        m = tr.pix2pix_model
        if tag == "sn":
            for name, net in (("G", m.netG), ("D", m.netD)):
                st = net.store
                out["%s_sn_params_M" % name] = round(sum(d["numel"] for d in st.sn) / 1e6, 3)
                out["%s_refresh_us" % name] = round(1e3 * timed(lambda: st.sn_refresh(True), a.steps, a.warmup), 1)
                out["%s_project_us" % name] = round(1e3 * timed(st.sn_project_grad, a.steps, a.warmup), 1)

        def step():
            tr.run_generator_one_step(data)
            tr.run_discriminator_one_step(data)
        out["%s_eager_ms" % tag] = round(timed(step, a.steps, a.warmup), 3)
        sg = StepGraph()
        tr.seg = sg
        sg.capture(step)
        out["%s_graph_ms" % tag] = round(timed(sg.replay, a.steps, a.warmup), 3)
        tr.seg = None
        del tr, m, sg
        torch.cuda.synchronize()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
