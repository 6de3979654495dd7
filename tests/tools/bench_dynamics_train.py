"""Times one ensemble-dynamics train step (SPEC.md N2b: forward, NLL head, backward, Adam) at the reference configuration
(E 7, hidden 256, 3 layers, obs 17, act 6) on the HIP path against the same model in torch's own ROCm ops (the restatement of
tests/ensemble_train_ref.py, eager, torch.optim.Adam).  A report, not a gate:

    python tests/tools/bench_dynamics_train.py [--batches 256 4096] [--iters 200] [--warmup 30] [--repeats 5]

Prints one JSON line per batch size: ms per step (median of the repeats; each repeat is `iters` back-to-back steps between two
synchronisations), samples/s (E * B rows per step) and the achieved fp32 TFLOP/s of the HIP path (6 E B sum(in * out) FLOP per
step) against the 157.3 TFLOP/s fp32 matrix peak."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ensemble_train_ref as R  # noqa: E402
from s2p_amd.dynamics import EnsembleTrainer, EnsembleTransition  # noqa: E402

PEAK_TFLOPS = 157.3


def timed(step, iters, warmup, repeats):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / iters)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    E, H, obs, act = 7, 256, 17, 6
    dev = torch.device("cuda:0")
    p = R.make_params(3, E, obs + act, H, 3, obs + 1, rand_bounds=False)
    flop_per_row = 6 * sum(i * o for i, o in [(obs + act, H), (H, H), (H, H), (H, 2 * (obs + 1))])
    for B in a.batches:
        g = torch.Generator().manual_seed(B)
        x = torch.randn(E, B, obs + act, generator=g).to(dev)
        y = (x[..., :obs + 1] + 0.3 * torch.randn(E, B, obs + 1, generator=g).to(dev)).contiguous()
        model = EnsembleTransition(obs, act, H, 3, ensemble_size=E).load_state_dict(p)
        tr = EnsembleTrainer(model)
        hip = timed(lambda: tr.train_step(x, y), a.iters, a.warmup, a.repeats)
        pt = {k: v.to(dev).clone().requires_grad_(True) for k, v in p.items()}
        opt = torch.optim.Adam(list(pt.values()), lr=1e-3)

        def eager():
            opt.zero_grad(set_to_none=True)
            R.loss_terms(pt, x, y)[0].backward()
            opt.step()
        ref = timed(eager, a.iters, a.warmup, a.repeats)
        print(json.dumps({"bench": "dynamics_train_step", "E": E, "hidden": H, "B": B, "hip_ms": round(hip[0], 4),
                          "hip_ms_min_max": [round(hip[1], 4), round(hip[2], 4)], "torch_eager_ms": round(ref[0], 4),
                          "torch_eager_ms_min_max": [round(ref[1], 4), round(ref[2], 4)], "speedup": round(ref[0] / hip[0], 2),
                          "hip_samples_per_s": round(E * B / hip[0] * 1e3), "hip_tflops": round(flop_per_row * E * B / hip[0] / 1e9, 2),
                          "fp32_matrix_peak_tflops": PEAK_TFLOPS, "iters": a.iters, "repeats": a.repeats}), flush=True)


if __name__ == "__main__":
    main()
