"""N3j measurement: the closed-loop imagination rollout as one launch (`LatentModel.fused_chain`, s2p_imagine_chain_fwd) against the
per-layer path of the same commit (the yardstick: 13 launches per step, all entry points the library had before), both in ONE
process and run.

    python tests/tools/bench_latent_imagine.py [--iters 50] [--warmup 5] [--repeats 5] [--horizon 16] [--batches 256,4096]
                                               [--widths 256,1024]

Sizes: Z 288, A 6, H 16, B 256 and 4096, policy width 256 and 1024.  Every figure is the median [min, max] of --repeats repeats of
--iters calls between two synchronisations, after --warmup calls.  One JSON line per figure, each with `unfused` (per-layer) and
`fused`:
  (a) `imagine` on given z0 / noise, with the library calls of one call and whether the two paths agree bitwise;
  (b) the chain launch alone (device events), with its share of one CU's fp32 MFMA rate;
  (c) `imagined_returns` end to end at context 8, B 256: encoder, posterior, rollout, reward head, the critic's bootstrap;
  (d) the fused `sample_posterior` (T 9) and fused `predict` (H 16) at B 256, for an A/B of the two older chains between builds."""
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
from s2p_amd.offline_rl import CriticSLAC, Qfunction, TanhGaussianPolicy, Vfunction  # noqa: E402
from s2p_amd.slac import LatentModel  # noqa: E402
from s2p_amd.slac_imagine import imagined_returns  # noqa: E402

A, Z, Z1, Z2, CONTEXT = 6, 288, 32, 256, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--batches", default="256,4096")
    ap.add_argument("--widths", default="256,1024")
    a = ap.parse_args()
    H = a.horizon
    t = lambda fn, iters=a.iters: timed(fn, iters, a.warmup, a.repeats)  # noqa: E731
    torch.manual_seed(0)
    latent = LatentModel((3, 100, 100), (A,), image_size=100)
    out(bench="latent_imagine", device=torch.cuda.get_device_name(0), A=A, H=H, iters=a.iters, repeats=a.repeats)
    g = torch.Generator().manual_seed(0)
    clock_hz = getattr(torch.cuda.get_device_properties(0), "clock_rate", 2400000) * 1e3
    policies = {}
    for W in [int(v) for v in a.widths.split(",")]:
        po = policies[W] = TanhGaussianPolicy(hidden_sizes=[W, W], obs_dim=Z, action_dim=A, init_w=0.05)
        macs = MACS_PER_ROW_STEP + Z * W + W * W + 16 * W + 2 * 16 * 256        # + the policy (a 16-column last tile) and two action chunks
        for B in [int(v) for v in a.batches.split(",")]:
            z0, noise = torch.randn(B, Z, generator=g).cuda(), torch.randn(B, H, Z, generator=g).cuda()

            # (a) imagine
            imagine = lambda: latent.imagine(po, z0, H, noise)  # noqa: E731
            calls = both(latent, lambda: count_calls(imagine))
            same = both(latent, lambda: [x.clone() for x in imagine()])
            report("imagine", both(latent, lambda: t(imagine)), B=B, W=W, calls_unfused=calls["unfused"], calls_fused=calls["fused"],
                   bitwise_equal=all(torch.equal(x, y) for x, y in zip(same["unfused"], same["fused"])))

            # (b) the launch alone
            p1, p2 = latent.z1_prior.packed(), latent.z2_prior.packed()
            wc, wb = latent.z1_prior.packed_cols(Z2, Z2 + A), p2["g1"][1][0]
            act, mean, std, z = (torch.empty(B, H, c, device="cuda") for c in (8, Z1, Z1, Z))
            mlps, pm = [ops.chain_mlp(p1, k1=Z2), ops.chain_mlp(p2)], ops.policy_mlp(po)
            us = bench_actor.kernel_us(lambda: ops.imagine_chain_fwd(z0, noise, mlps, wc, wb, A, pm, act, mean, std, z), n=50)
            flops_per_tile = 2.0 * 16 * H * macs
            out(bench="imagine_chain_launch_alone", B=B, W=W, us=round(us, 2), us_per_step=round(us / H, 2), workgroups=(B + 15) // 16,
                mflop_per_workgroup=round(flops_per_tile / 1e6, 2), clock_mhz=round(clock_hz / 1e6),
                share_of_one_cu_fp32_mfma_rate=round(flops_per_tile / (us * 1e-6) / (CU_FP32_MFMA_FLOPS_PER_CYCLE * clock_hz), 3))

    # (c) imagined_returns end to end
    B, W = 256, min(policies)
    q = [Qfunction(hidden_sizes=[W, W], output_size=1, input_size=Z + A) for _ in range(4)]
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=[W, W], output_size=1, input_size=Z))
    r = np.random.RandomState(0)
    frames = torch.from_numpy(np.frombuffer(r.bytes(B * (CONTEXT + 1) * 30000), dtype=np.uint8).reshape(B, CONTEXT + 1, 100, 100, 3).copy()).cuda()
    acts = (torch.rand(B, CONTEXT, A, generator=g) * 2 - 1).cuda()
    step = lambda: imagined_returns(latent, policies[W], frames, acts, H, critic=critic, context=CONTEXT)  # noqa: E731
    report("imagined_returns", both(latent, lambda: t(step, max(a.iters // 10, 2))), B=B, W=W)

    # (d) the two older chains, fused, for an A/B between builds
    latent.fused_chain = True
    feat, pa = torch.randn(B, CONTEXT + 1, 256, generator=g).cuda(), (torch.rand(B, CONTEXT, A, generator=g) * 2 - 1).cuda()
    pn = torch.randn(B, CONTEXT + 1, Z, generator=g).cuda()
    z0, fa, noise = torch.randn(B, Z, generator=g).cuda(), (torch.rand(B, H, A, generator=g) * 2 - 1).cuda(), torch.randn(B, H, Z, generator=g).cuda()
    with torch.no_grad():
        ms = t(lambda: latent.sample_posterior(feat, pa, pn))
        out(bench="sample_posterior_fused", B=B, T=CONTEXT + 1, ms=ms[0], ms_min_max=ms[1:])
    ms = t(lambda: latent.predict(z0, fa, noise))
    out(bench="predict_fused", B=B, H=H, ms=ms[0], ms_min_max=ms[1:])
    latent.fused_chain = False


if __name__ == "__main__":
    main()
