"""N3i measurement: the open-loop prior rollout as one launch (`LatentModel.fused_chain`, s2p_prior_chain_fwd) against the per-layer
path of the same commit (the yardstick), both in ONE process and run.

    python tests/tools/bench_latent_predict.py [--iters 50] [--warmup 5] [--repeats 5] [--horizons 8,32]

Sizes: Z 288, A 6, B 256, H 8 and 32.  Every figure is the median [min, max] of --repeats repeats of --iters calls between two
synchronisations, after --warmup calls.  One JSON line per figure, each with `unfused` (per-layer) and `fused`:
  (a) `predict` on given z0 / actions / noise, with the library calls of one call and whether the two paths agree bitwise;
  (b) the chain launch alone (device events), with its share of one CU's fp32 MFMA rate, and the two hoisted action terms alone;
  (c) `open_loop` end to end at context 8: encoder, posterior, rollout, decoder, both metrics passes, reward head."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("", "tests", os.path.join("tests", "tools")):
    sys.path.insert(0, os.path.join(ROOT, p))
import bench_actor  # noqa: E402
from bench_feature_cache import out, timed  # noqa: E402
from bench_posterior_chain import CU_FP32_MFMA_FLOPS_PER_CYCLE, MACS_PER_ROW_STEP, both, report  # noqa: E402
from s2p_amd import ops  # noqa: E402
from slac_chain_util import count_calls  # noqa: E402
from s2p_amd.slac import LatentModel, _action_term  # noqa: E402
from s2p_amd.slac_predict import open_loop  # noqa: E402

A, B, Z, Z1, Z2, CONTEXT = 6, 256, 288, 32, 256, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--horizons", default="8,32")
    a = ap.parse_args()
    t = lambda fn, iters=a.iters: timed(fn, iters, a.warmup, a.repeats)  # noqa: E731
    torch.manual_seed(0)
    latent = LatentModel((3, 100, 100), (A,), image_size=100)
    out(bench="latent_predict", device=torch.cuda.get_device_name(0), B=B, A=A, iters=a.iters, repeats=a.repeats)
    g = torch.Generator().manual_seed(0)
    r = np.random.RandomState(0)
    for H in [int(v) for v in a.horizons.split(",")]:
        z0, actions, noise = torch.randn(B, Z, generator=g).cuda(), (torch.rand(B, H, A, generator=g) * 2 - 1).cuda(), torch.randn(B, H, Z, generator=g).cuda()

        # (a) predict
        predict = lambda: latent.predict(z0, actions, noise)  # noqa: E731
        calls = both(latent, lambda: count_calls(predict))
        same = both(latent, lambda: [x.clone() for x in predict()])
        report("predict", both(latent, lambda: t(predict)), H=H, calls_unfused=calls["unfused"], calls_fused=calls["fused"],
               bitwise_equal=all(torch.equal(x, y) for x, y in zip(same["unfused"], same["fused"])))

        # (b) the launch alone, and the hoisted terms alone
        p1, p2 = latent.z1_prior.packed(), latent.z2_prior.packed()
        wa, wb = latent.z1_prior.packed_cols(Z2, Z2 + A), p2["g1"][1][0]
        rc, rb = _action_term(actions, wa)[1], _action_term(actions, wb)[1]
        mean, std, z = (torch.empty(B, H, c, device="cuda") for c in (Z1, Z1, Z))
        mlps = [ops.chain_mlp(p1, k1=Z2), ops.chain_mlp(p2)]
        us = bench_actor.kernel_us(lambda: ops.prior_chain_fwd(z0[:, Z1:], rc, rb, noise, mlps, mean, std, z))
        flops_per_tile = 2.0 * 16 * H * MACS_PER_ROW_STEP
        clock_hz = getattr(torch.cuda.get_device_properties(0), "clock_rate", 2400000) * 1e3
        out(bench="prior_chain_launch_alone", H=H, us=round(us, 2), us_per_step=round(us / H, 2), workgroups=(B + 15) // 16,
            mflop_per_workgroup=round(flops_per_tile / 1e6, 2), clock_mhz=round(clock_hz / 1e6),
            share_of_one_cu_fp32_mfma_rate=round(flops_per_tile / (us * 1e-6) / (CU_FP32_MFMA_FLOPS_PER_CYCLE * clock_hz), 3))
        hoist_us = bench_actor.kernel_us(lambda: (_action_term(actions, wa), _action_term(actions, wb)))
        out(bench="action_terms_alone", H=H, us=round(hoist_us, 2))

        # (c) open_loop end to end
        frames = torch.from_numpy(np.frombuffer(r.bytes(B * (CONTEXT + H + 1) * 30000), dtype=np.uint8).reshape(B, CONTEXT + H + 1, 100, 100, 3).copy()).cuda()
        acts = (torch.rand(B, CONTEXT + H, A, generator=g) * 2 - 1).cuda()
        rewards = torch.randn(B, CONTEXT + H, generator=g).cuda()
        report("open_loop", both(latent, lambda: t(lambda: open_loop(latent, frames, acts, rewards, context=CONTEXT), max(a.iters // 10, 2))), H=H)


if __name__ == "__main__":
    main()
