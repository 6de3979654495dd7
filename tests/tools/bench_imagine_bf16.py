"""N3n measurement: the bf16 compute mode of the fused imagination chain (`LatentModel.imagine(..., compute="bf16")`) against the fp32
fused launch of the same commit (the yardstick), both in ONE process and run, and `compare_policies` against repeated
`imagined_returns`.

    python tests/tools/bench_imagine_bf16.py [--batches 32,256,4096] [--widths 256,1024] [--horizon 16] [--iters 50] [--repeats 5]

Sizes: Z 288, A 6, H 16.  Every figure is the median [min, max] of --repeats repeats of --iters calls after --warmup calls: a launch
alone between two device events, a host figure between two synchronisations.  One JSON line per figure:
  (a) the launch alone, fp32 and bf16, with what bounds the bf16 one: the time of a 16-row workgroup's MFMAs at one 16x16x32 per 16
      cycles and SIMD (8 passes of 4 cycles, two waves per SIMD alternating), and of its weight bytes at 64 bytes per clock and CU;
  (b) `imagine` in both modes, and at W 1024 the per-layer path (13 launches per step);
  (c) `compare_policies` of 8 policies against 8 calls of `imagined_returns` (B 256, context 8, both modes);
  (d) the distance of the fp32 and the bf16 rollout from the fp64 fixture tests/golden/slac_imagine_golden_v1.npz, per step."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("", "oracle", "tests", os.path.join("tests", "tools")):
    sys.path.insert(0, os.path.join(ROOT, p))
import slac_imagine_ref as IM  # noqa: E402
from bench_feature_cache import out, timed  # noqa: E402
from s2p_amd import ops  # noqa: E402
from s2p_amd.offline_rl import TanhGaussianPolicy  # noqa: E402
from s2p_amd.slac_imagine import compare_policies, imagined_returns  # noqa: E402
from slac_chain_util import build_model  # noqa: E402

A, Z1, Z2, Z = 6, 32, 256, 288
LATENT_MACS = (256 * 256 + 256 * 256 + 256 * 64) + (288 * 256 + 256 * 256 + 256 * 512)     # per row and step, the chain columns
L2_BYTES_PER_CLOCK_CU, MFMA_CYCLES, MACS_PER_MFMA = 64, 16, 16 * 16 * 32


def event_us(fn, iters, warmup, repeats):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(repeats):
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / iters)
    return [round(statistics.median(ts), 2), round(min(ts), 2), round(max(ts), 2)]


def policy(W, seed=None):
    return TanhGaussianPolicy(hidden_sizes=[W, W], obs_dim=Z, action_dim=A).load_state_dict(IM.make_policy_params(W, A, seed))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,256,4096")
    ap.add_argument("--widths", default="256,1024")
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    H = a.horizon
    m = build_model(A)
    clock_hz = getattr(torch.cuda.get_device_properties(0), "clock_rate", 2400000) * 1e3
    out(bench="imagine_bf16", device=torch.cuda.get_device_name(0), A=A, H=H, iters=a.iters, repeats=a.repeats, clock_mhz=round(clock_hz / 1e6))
    g1, g2 = m.z1_prior, m.z2_prior
    wc, wb = g1.packed_cols(Z2, Z2 + A), g2.packed()["g1"][1][0]
    m32 = [ops.chain_mlp(g1.packed(), k1=Z2), ops.chain_mlp(g2.packed())]
    m16 = [ops.chain_mlp_bf16(g1.packed_bf16(k1=Z2)), ops.chain_mlp_bf16(g2.packed_bf16())]
    for W in [int(v) for v in a.widths.split(",")]:
        po = policy(W)
        p32, p16 = ops.policy_mlp(po), ops.policy_mlp_bf16(po)
        macs = LATENT_MACS + Z * W + W * W + W * 16                                  # the last layer is one 16-column tile
        for B in [int(v) for v in a.batches.split(",")]:
            g = torch.Generator().manual_seed(B + W)
            z0, eps = torch.randn(B, Z, generator=g).cuda(), torch.randn(B, H, Z, generator=g).cuda()
            act, mean, std, z = (torch.zeros(B, H, c, device="cuda") for c in (8, Z1, Z1, Z))
            u32 = event_us(lambda: ops.imagine_chain_fwd(z0, eps, m32, wc, wb, A, p32, act, mean, std, z), a.iters, a.warmup, a.repeats)
            u16 = event_us(lambda: ops.imagine_chain_fwd_bf16(z0, eps, m16, wc, wb, A, p16, act, mean, std, z), a.iters, a.warmup, a.repeats)
            out(bench="launch_alone", W=W, B=B, fp32_us=u32[0], fp32_us_min_max=u32[1:], bf16_us=u16[0], bf16_us_min_max=u16[1:],
                speedup=round(u32[0] / u16[0], 3), fp32_us_per_step=round(u32[0] / H, 2), bf16_us_per_step=round(u16[0] / H, 2),
                workgroups=(B + 15) // 16,
                bf16_mfma_on_4_simds_us=round(H * 16 * macs / MACS_PER_MFMA / 4 * MFMA_CYCLES / clock_hz * 1e6, 2),
                bf16_weights_at_64_bytes_per_clock_us=round(H * 2 * macs / L2_BYTES_PER_CLOCK_CU / clock_hz * 1e6, 2))
            res = {}
            for name, fused, kw in (("fp32", True, {}), ("bf16", True, dict(compute="bf16"))) + \
                    ((("per_layer", False, {}),) if W == 1024 else ()):
                m.fused_chain = fused
                res[name] = timed(lambda: m.imagine(po, z0, H, eps, **kw), a.iters, a.warmup, a.repeats)
            m.fused_chain = False
            out(bench="imagine", W=W, B=B, **{k + "_ms": v[0] for k, v in res.items()}, **{k + "_ms_min_max": v[1:] for k, v in res.items()},
                speedup=round(res["fp32"][0] / res["bf16"][0], 3))

    # (c) compare_policies against repeated imagined_returns
    B, C, P = 256, 8, 8
    r = np.random.RandomState(0)
    frames = np.frombuffer(r.bytes(B * (C + 1) * 100 * 100 * 3), dtype=np.uint8).reshape(B, C + 1, 100, 100, 3)
    actions = r.uniform(-1, 1, (B, C, A)).astype(np.float32)
    pols = [policy(256, seed=100 + i) for i in range(P)]
    for mode, cc in (("fp32", "fp32"), ("bf16", "bf16")):
        m.fused_chain, m.chain_compute = True, cc
        one = timed(lambda: [imagined_returns(m, po, frames, actions, H, context=C, compute=mode) for po in pols], 5, 2, a.repeats)
        cmp_ = timed(lambda: compare_policies(m, pols, frames, actions, H, context=C, compute=mode), 5, 2, a.repeats)
        m.fused_chain, m.chain_compute = False, "fp32"
        out(bench="compare_policies", mode=mode, policies=P, B=B, context=C, H=H, W=256, eight_imagined_returns_ms=one[0],
            eight_imagined_returns_ms_min_max=one[1:], compare_policies_ms=cmp_[0], compare_policies_ms_min_max=cmp_[1:],
            speedup=round(one[0] / cmp_[0], 3))

    # (d) the fixture: reported, not gated (rounding flips travel down the rollout)
    golden = np.load(os.path.join(ROOT, "tests", "golden", "slac_imagine_golden_v1.npz"))
    po = policy(IM.W)
    z0, noise = [t.cuda() for t in IM.make_inputs(IM.B, IM.H)]
    m.fused_chain = True
    for mode in ("fp32", "bf16"):
        got = dict(zip(("actions", "z1_mean", "z1_std", "z"), m.imagine(po, z0, IM.H, noise, compute=mode)))
        for k, v in got.items():
            out(bench="fixture_distance", mode=mode, quantity=k, per_step=[float("%.3e" % e) for e in IM.step_err(v, golden["sampled." + k])],
                ref32_err=[float("%.3e" % e) for e in golden["sampled.%s.ref32_err" % k]])
    m.fused_chain = False


if __name__ == "__main__":
    main()
