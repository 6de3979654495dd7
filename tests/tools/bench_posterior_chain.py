"""N3h measurement: the fused no-grad posterior chain (`LatentModel.fused_chain`, s2p_posterior_chain_fwd) against the per-layer path
(the behaviour without the flag: the yardstick), both in ONE process and run.

    python tests/tools/bench_posterior_chain.py [--rows 50000] [--iters 50] [--warmup 5] [--repeats 5] [--envs 1,4,16]

Sizes: Z 288, A 6, B 256, S 8, H 1024 (tests/tools/bench_iql.py / bench_cql.py), on the --rows real + --rows generated buffer of
tests/tools/bench_feature_cache.py.  Every figure is the median [min, max] of --repeats repeats of --iters calls between two
synchronisations, after --warmup calls.  One JSON line per figure, each with `unfused` and `fused`:
  (a) no-grad `sample_posterior` on given features, and the library calls of one call;
  (b) `prepare_batch` on a FeatureBatch -- the acceptance: fused faster by more than the unfused path's own [min, max] spread;
  (c) `train_from_torch` with freeze_slac on cached features, IQL and CQL;
  (d) the chain launch alone (device events), with its share of one CU's fp32 MFMA rate;
  (e) the `latent_z` actor step at --envs environments."""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("", "tests", os.path.join("tests", "tools")):
    sys.path.insert(0, os.path.join(ROOT, p))
import bench_actor  # noqa: E402
import bench_cql  # noqa: E402
import bench_iql  # noqa: E402
from bench_feature_cache import datasets, out, timed  # noqa: E402
from s2p_amd import ops  # noqa: E402
from slac_chain_util import count_calls  # noqa: E402
from s2p_amd.actor import SlacActor  # noqa: E402
from s2p_amd.offline_rl import TanhGaussianPolicy  # noqa: E402
from s2p_amd.slac import _PosteriorFn  # noqa: E402
from s2p_amd.slac_algo import SlacAlgorithm  # noqa: E402

S, A, H, W, C, B, FEAT, Z = 8, 6, 100, 100, 3, 256, 256, 288
MACS_PER_ROW = (256 * 256 + 256 * 256 + 256 * 64) + (32 * 256 + 256 * 256 + 256 * 512)            # t = 0
MACS_PER_ROW_STEP = (256 * 256 + 256 * 256 + 256 * 64) + (288 * 256 + 256 * 256 + 256 * 512)      # t >= 1
CU_FP32_MFMA_FLOPS_PER_CYCLE = 256                                                                # 4 SIMDs x v_mfma_f32_16x16x4_f32


def both(latent, make):
    """make() -> the step to time, built once per setting of the flag; -> {unfused: [med, min, max], fused: ...}"""
    res = {}
    for name, on in (("unfused", False), ("fused", True)):
        latent.fused_chain = on
        res[name] = make()
    latent.fused_chain = False
    return res


def report(bench, ms, **kw):
    u, f = ms["unfused"], ms["fused"]
    out(bench=bench, unfused_ms=u[0], unfused_ms_min_max=u[1:], fused_ms=f[0], fused_ms_min_max=f[1:], speedup=round(u[0] / f[0], 3),
        saving_ms=round(u[0] - f[0], 4), unfused_spread_ms=round(u[2] - u[1], 4), **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--episode", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--envs", default="1,4,16")
    a = ap.parse_args()
    N = a.rows
    t = lambda fn, iters=a.iters: timed(fn, iters, a.warmup, a.repeats)  # noqa: E731
    real, gen = datasets(N, min(a.episode, N))
    algo = SlacAlgorithm((C, H, W), (A,), 1, "cuda:0", 0, buffer_size=2 * N, num_sequences=S, frame_capacity=3 * N + S + 1)
    algo.load_data_in_buffer(real)
    algo.load_data_in_buffer(gen, data_num=N, generated_for_slac=True, data_mix_type="all_state_1step_random_action",
                             uncertainty_penalty_lambda=0.0)
    del real, gen
    buf, latent = algo.buffer, algo.latent
    algo.cache_features()
    torch.cuda.synchronize()
    out(bench="posterior_chain", device=torch.cuda.get_device_name(0), windows=len(buf), B=B, S=S, A=A, iters=a.iters, repeats=a.repeats)

    # (a) sample_posterior on given features
    g = torch.Generator().manual_seed(0)
    feat, action, noise = (torch.randn(B, S + 1, FEAT, generator=g).cuda(), torch.randn(B, S, A, generator=g).cuda(),
                           torch.randn(B, S + 1, Z, generator=g).cuda())

    def posterior():
        with torch.no_grad():
            return latent.sample_posterior(feat, action, noise)
    calls = both(latent, lambda: count_calls(posterior))
    same = both(latent, lambda: [x.clone() for x in posterior()])
    report("sample_posterior_no_grad", both(latent, lambda: t(posterior)), calls_unfused=calls["unfused"], calls_fused=calls["fused"],
           bitwise_equal=all(torch.equal(x, y) for x, y in zip(same["unfused"], same["fused"])))

    # (b) prepare_batch on a FeatureBatch
    batch = buf.random_batch(B, frames="features")
    ms = both(latent, lambda: t(lambda: algo.prepare_batch(batch["observations"], batch["actions"])))
    report("prepare_batch_on_features", ms, faster_by_more_than_the_unfused_spread=bool(ms["unfused"][0] - ms["fused"][0] > ms["unfused"][2] - ms["unfused"][1]))

    # (c) the cached step
    for kind, mod in (("iql", bench_iql), ("cql", bench_cql)):
        def make():
            tr = mod.trainer("cuda:0", slac_algo=algo, freeze_slac=True)
            return t(lambda: tr.train_from_torch(buf.random_batch(B, frames="features")))
        report("train_from_torch_cached", both(latent, make), trainer=kind)

    # (d) the launch alone
    packs = [m.packed() for m in (latent.z1_posterior_init, latent.z2_prior_init, latent.z1_posterior, latent.z2_prior)]
    ra, rb = _PosteriorFn._hoisted(feat, action, packs[2], packs[3])[2:]
    mean, std, z = (torch.empty(B, S + 1, c, device="cuda") for c in (32, 32, Z))
    mlps = [ops.chain_mlp(p) for p in packs]
    us = bench_actor.kernel_us(lambda: ops.posterior_chain_fwd(feat[:, 0], ra, rb, noise, mlps, mean, std, z))
    flops_per_tile = 2.0 * 16 * (MACS_PER_ROW + S * MACS_PER_ROW_STEP)
    clock_hz = getattr(torch.cuda.get_device_properties(0), "clock_rate", 2400000) * 1e3
    out(bench="chain_launch_alone", us=round(us, 2), workgroups=(B + 15) // 16, mflop_per_workgroup=round(flops_per_tile / 1e6, 2),
        clock_mhz=round(clock_hz / 1e6), share_of_one_cu_fp32_mfma_rate=round(flops_per_tile / (us * 1e-6) / (CU_FP32_MFMA_FLOPS_PER_CYCLE * clock_hz), 3))
    hoist_us = bench_actor.kernel_us(lambda: _PosteriorFn._hoisted(feat, action, packs[2], packs[3]))
    out(bench="hoisted_terms_alone", us=round(hoist_us, 2))

    # (e) the latent_z actor step
    stand_in = types.SimpleNamespace(latent=latent, state_shape=(C, H, W), action_shape=(A,), num_sequences=S)
    policy = TanhGaussianPolicy([1024, 1024], Z, A)
    for n in [int(v) for v in a.envs.split(",")]:
        def make():
            envs, actor = bench_actor.Envs(n), SlacActor(policy, stand_in, n, "latent_z")
            actor.reset(envs.frames)

            def step():
                act = actor.act()
                actor.observe(envs.step(act), act)
            return t(step)
        report("latent_z_actor_step", both(latent, make), num_envs=n)


if __name__ == "__main__":
    main()
