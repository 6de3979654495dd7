"""N3m measurement: the bf16 compute mode of the fused no-grad latent chains (`LatentModel.chain_compute = "bf16"`) against the fp32
fused chains of the same commit (the yardstick), both in ONE process and run.

    python tests/tools/bench_chain_bf16.py [--rows 20000] [--batches 32,256,4096] [--iters 50] [--warmup 5] [--repeats 5]

Sizes: Z 288, A 6, S 8, H 1024 (tests/tools/bench_iql.py / bench_cql.py), on the --rows real + --rows generated buffer of
tests/tools/bench_feature_cache.py.  Every host figure is the median [min, max] of --repeats repeats of --iters calls between two
synchronisations, after --warmup calls; a launch alone is timed with device events.  One JSON line per figure, each with `fp32` and
`bf16`, per batch size B:
  (a) the chain launch alone (posterior, T = S + 1) with what bounds it: the time the weight traffic of a 16-row workgroup would take
      at 64 bytes per clock and CU, and the time of its MFMAs at one per 16 cycles and SIMD; and the prior launch at H 8 and 32;
  (b) no-grad `sample_posterior` on given features, `predict` at H 8 and 32;
  (c) `prepare_batch` on a FeatureBatch;
  (d) cached `train_from_torch` of IQL and CQL, with mlp_compute "fp32" and "bf16";
  (e) the imagination chain (fp32 in both modes: the third older fused chain) at H 8."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("", "tests", os.path.join("tests", "tools")):
    sys.path.insert(0, os.path.join(ROOT, p))
import bench_actor  # noqa: E402
import bench_cql  # noqa: E402
import bench_iql  # noqa: E402
from bench_feature_cache import datasets, out, timed  # noqa: E402
from s2p_amd import ops  # noqa: E402
from s2p_amd.offline_rl import TanhGaussianPolicy  # noqa: E402
from s2p_amd.slac import _PosteriorFn, _action_term  # noqa: E402
from s2p_amd.slac_algo import SlacAlgorithm  # noqa: E402

S, A, H, W, C, FEAT, Z1, Z2, Z = 8, 6, 100, 100, 3, 256, 32, 256, 288
MACS_T0 = (256 * 256 + 256 * 256 + 256 * 64) + (32 * 256 + 256 * 256 + 256 * 512)                 # per row, t = 0
MACS_STEP = (256 * 256 + 256 * 256 + 256 * 64) + (288 * 256 + 256 * 256 + 256 * 512)              # per row, t >= 1
L2_BYTES_PER_CLOCK_CU, MFMA_CYCLES, MACS_PER_MFMA = 64, 16, 16 * 16 * 32


def both(latent, make):
    """make() -> the figure, taken once per mode; -> {fp32: ..., bf16: ...}"""
    res = {}
    for mode in ("fp32", "bf16"):
        latent.chain_compute = mode
        res[mode] = make()
    latent.chain_compute = "fp32"
    return res


def report(bench, ms, **kw):
    f, b = ms["fp32"], ms["bf16"]
    out(bench=bench, fp32_ms=f[0], fp32_ms_min_max=f[1:], bf16_ms=b[0], bf16_ms_min_max=b[1:], speedup=round(f[0] / b[0], 3),
        saving_ms=round(f[0] - b[0], 4), fp32_spread_ms=round(f[2] - f[1], 4), **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--episode", type=int, default=1000)
    ap.add_argument("--batches", default="32,256,4096")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    N = a.rows
    t = lambda fn: timed(fn, a.iters, a.warmup, a.repeats)  # noqa: E731
    real, gen = datasets(N, min(a.episode, N))
    algo = SlacAlgorithm((C, H, W), (A,), 1, "cuda:0", 0, buffer_size=2 * N, num_sequences=S, frame_capacity=3 * N + S + 1, fused_chain=True)
    algo.load_data_in_buffer(real)
    algo.load_data_in_buffer(gen, data_num=N, generated_for_slac=True, data_mix_type="all_state_1step_random_action",
                             uncertainty_penalty_lambda=0.0)
    del real, gen
    buf, latent = algo.buffer, algo.latent
    algo.cache_features()
    torch.cuda.synchronize()
    clock_hz = getattr(torch.cuda.get_device_properties(0), "clock_rate", 2400000) * 1e3
    out(bench="chain_bf16", device=torch.cuda.get_device_name(0), windows=len(buf), S=S, A=A, iters=a.iters, repeats=a.repeats,
        clock_mhz=round(clock_hz / 1e6))
    heads = (latent.z1_posterior_init, latent.z2_prior_init, latent.z1_posterior, latent.z2_prior)
    policy = TanhGaussianPolicy([1024, 1024], Z, A)

    for B in [int(v) for v in a.batches.split(",")]:
        g = torch.Generator().manual_seed(B)
        feat, action, noise = (torch.randn(B, S + 1, FEAT, generator=g).cuda(), torch.randn(B, S, A, generator=g).cuda(),
                               torch.randn(B, S + 1, Z, generator=g).cuda())
        # (a) the launches alone
        packs = [m.packed() for m in heads]
        ra, rb = _PosteriorFn._hoisted(feat, action, packs[2], packs[3])[2:]
        mean, std, z = (torch.empty(B, S + 1, c, device="cuda") for c in (Z1, Z1, Z))
        m32, m16 = [ops.chain_mlp(p) for p in packs], [ops.chain_mlp_bf16(m.packed_bf16()) for m in heads]
        us32 = bench_actor.kernel_us(lambda: ops.posterior_chain_fwd(feat[:, 0], ra, rb, noise, m32, mean, std, z))
        us16 = bench_actor.kernel_us(lambda: ops.posterior_chain_fwd_bf16(feat[:, 0], ra, rb, noise, m16, mean, std, z))
        macs = MACS_T0 + S * MACS_STEP
        out(bench="posterior_launch_alone", B=B, fp32_us=round(us32, 2), bf16_us=round(us16, 2), speedup=round(us32 / us16, 3),
            workgroups=(B + 15) // 16, bf16_weight_kib_per_workgroup=round(2 * macs / 1024, 1),
            weights_at_64_bytes_per_clock_us=round(2 * macs / L2_BYTES_PER_CLOCK_CU / clock_hz * 1e6, 2),
            mfma_on_4_simds_us=round(16 * macs / MACS_PER_MFMA / 4 * MFMA_CYCLES / clock_hz * 1e6, 2), barriers=6 * (S + 1))
        z0 = torch.randn(B, Z, generator=g).cuda()
        for Hz in (8, 32):
            acts, eps = torch.randn(B, Hz, A, generator=g).cuda(), torch.randn(B, Hz, Z, generator=g).cuda()
            g1, g2 = latent.z1_prior, latent.z2_prior
            rc, rb2 = _action_term(acts, g1.packed_cols(Z2, Z2 + A))[1], _action_term(acts, g2.packed()["g1"][1][0])[1]
            pm, ps, pz = (torch.empty(B, Hz, c, device="cuda") for c in (Z1, Z1, Z))
            p32 = [ops.chain_mlp(g1.packed(), k1=Z2), ops.chain_mlp(g2.packed())]
            p16 = [ops.chain_mlp_bf16(g1.packed_bf16(k1=Z2)), ops.chain_mlp_bf16(g2.packed_bf16())]
            u32 = bench_actor.kernel_us(lambda: ops.prior_chain_fwd(z0[:, Z1:], rc, rb2, eps, p32, pm, ps, pz), n=50)
            u16 = bench_actor.kernel_us(lambda: ops.prior_chain_fwd_bf16(z0[:, Z1:], rc, rb2, eps, p16, pm, ps, pz), n=50)
            out(bench="prior_launch_alone", B=B, H=Hz, fp32_us=round(u32, 2), bf16_us=round(u16, 2), speedup=round(u32 / u16, 3),
                fp32_us_per_step=round(u32 / Hz, 2), bf16_us_per_step=round(u16 / Hz, 2))

            # (b) predict
            def predict():
                return latent.predict(z0, acts, eps)
            report("predict", both(latent, lambda: t(predict)), B=B, H=Hz)

        # (b) sample_posterior on given features
        def posterior():
            with torch.no_grad():
                return latent.sample_posterior(feat, action, noise)
        report("sample_posterior_no_grad", both(latent, lambda: t(posterior)), B=B)

        # (c) prepare_batch on a FeatureBatch
        batch = buf.random_batch(B, frames="features")
        report("prepare_batch_on_features", both(latent, lambda: t(lambda: algo.prepare_batch(batch["observations"], batch["actions"]))), B=B)

        # (d) the cached step
        for kind, mod in (("iql", bench_iql), ("cql", bench_cql)):
            for mlp in ("fp32", "bf16"):
                def make():
                    tr = mod.trainer("cuda:0", slac_algo=algo, freeze_slac=True, mlp_compute=mlp)
                    return t(lambda: tr.train_from_torch(buf.random_batch(B, frames="features")))
                report("train_from_torch_cached", both(latent, make), trainer=kind, mlp_compute=mlp, B=B)

        # (e) the third older fused chain
        eps8 = torch.randn(B, 8, Z, generator=g).cuda()
        report("imagine_fp32_in_both_modes", both(latent, lambda: t(lambda: latent.imagine(policy, z0, 8, eps8))), B=B, H=8)


if __name__ == "__main__":
    main()
