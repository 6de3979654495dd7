"""N3g measurement: frozen-SLAC IQL / CQL steps on cached encoder features against the same steps on frames, in ONE process and run.

    python tests/tools/bench_feature_cache.py [--rows 50000] [--iters 50] [--warmup 5] [--repeats 5]

Sizes: Z 288, A 6, H 1024, P 2090, B 256 (tests/tools/bench_iql.py / bench_cql.py) on the synthetic buffer of
tests/tools/bench_slac_buffer.py, --rows real + --rows generated rows of 100x100x3 frames.  Every figure is the median [min, max] of
--repeats repeats of --iters calls between two synchronisations, after --warmup calls.  One JSON line per figure:
  (a) `train_from_torch` with freeze_slac, IQL and CQL, fp32 and bf16 stacks: `random_batch(256)` (frames: what the step did before the
      cache existed, the yardstick) against `random_batch(256, frames="features")`;
  (b) `random_batch(256, frames="features")` alone, and its launch alone with its GB/s against the 8 TB/s HBM peak;
  (c) `prepare_batch` on a FeatureBatch: what the posterior chain costs once the encoder is gone;
  (d) `attach_features`: seconds and frames/s for the whole pool, and the table's bytes;
  (e) steps (and epochs of the buffer's windows) until (d) is paid back by the per-step saving of (a)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("", "tests", os.path.join("tests", "tools")):
    sys.path.insert(0, os.path.join(ROOT, p))
import bench_cql  # noqa: E402
import bench_iql  # noqa: E402
from s2p_amd import ops  # noqa: E402
from s2p_amd.slac import LatentModel  # noqa: E402
from s2p_amd.slac_algo import SlacAlgorithm  # noqa: E402

S, A, H, W, C, B, FEAT = 8, 6, 100, 100, 3, 256, 256
HBM_PEAK = 8e12


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
    return [round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)]


def out(**kw):
    print(json.dumps(kw), flush=True)


def datasets(N, EP):
    r = np.random.RandomState(0)

    def frames(n):
        return np.frombuffer(r.bytes(n * H * W * C), dtype=np.uint8).reshape(n, H, W, C)
    timeouts = np.zeros(N, dtype=bool)
    timeouts[EP - 1::EP] = True
    obs_idx = np.full((N, S + 1), int(1e9), dtype=np.int64)
    i = np.arange(N)
    ok = i % EP >= S
    obs_idx[ok] = i[ok, None] - S + np.arange(S + 1)[None, :]
    real = dict(actions=r.uniform(-1, 1, (N, A)).astype(np.float32), rewards=r.randn(N).astype(np.float32), timeouts=timeouts,
                image_observations=frames(N), image_observations_tp1=frames(N))
    gen = dict(actions=r.uniform(-1, 1, (N, A)).astype(np.float32), rewards=r.randn(N).astype(np.float32), timeouts=timeouts,
               image_observations=real["image_observations"], image_observations_tp1=frames(N), original_actions=real["actions"],
               original_rewards=real["rewards"], slac_observation_indices=obs_idx, slac_action_indices=obs_idx[:, :-1].copy())
    return real, gen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--episode", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    N = a.rows
    t = lambda fn, iters=a.iters: timed(fn, iters, a.warmup, a.repeats)  # noqa: E731
    real, gen = datasets(N, min(a.episode, N))
    algo = SlacAlgorithm((C, H, W), (A,), 1, "cuda:0", 0, buffer_size=2 * N, num_sequences=S, frame_capacity=3 * N + S + 1)
    algo.load_data_in_buffer(real)
    algo.load_data_in_buffer(gen, data_num=N, generated_for_slac=True, data_mix_type="all_state_1step_random_action",
                             uncertainty_penalty_lambda=0.0)
    del real, gen
    buf = algo.buffer
    torch.cuda.synchronize()
    out(bench="feature_cache", device=torch.cuda.get_device_name(0), windows=len(buf), frames=buf._head,
        pool_gb=round(buf._head * H * W * C / 1e9, 3), B=B, iters=a.iters, repeats=a.repeats)
    sd = algo.latent.state_dict()
    for dtype in (torch.float32, torch.bfloat16):
        name = str(dtype).split(".")[-1]
        if dtype != torch.float32:                         # the same buffer and weights under the other compute dtype of the stacks
            algo.latent = LatentModel((C, H, W), (A,), dtype=dtype, device="cuda:0")
            algo.latent.load_state_dict(sd, strict=True)
            buf.dtype = dtype
        # (d) the build
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        algo.cache_features()
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t0
        out(bench="attach_features", stacks=name, seconds=round(build_s, 3), frames=buf._head, frames_per_s=round(buf._head / build_s),
            table_bytes=buf.features.numel() * 4)
        # (a) the step on either batch form
        for kind, mod in (("iql", bench_iql), ("cql", bench_cql)):
            ms = {}
            for form in ("packed", "features"):
                tr = mod.trainer("cuda:0", slac_algo=algo, freeze_slac=True)
                ms[form] = t(lambda: tr.train_from_torch(buf.random_batch(B, frames=form)))
            saving = ms["packed"][0] - ms["features"][0]
            steps = build_s * 1e3 / saving if saving > 0 else None
            out(bench="train_from_torch_freeze_slac", trainer=kind, stacks=name, frames_ms=ms["packed"][0], frames_ms_min_max=ms["packed"][1:],
                cached_ms=ms["features"][0], cached_ms_min_max=ms["features"][1:], speedup=round(ms["packed"][0] / ms["features"][0], 3),
                break_even_steps=None if steps is None else round(steps),
                break_even_epochs=None if steps is None else round(steps * B / len(buf), 3))
        if dtype == torch.float32:
            # (b) the sample and its launch alone
            ms = t(lambda: buf.random_batch(B, frames="features"))
            out(bench="random_batch_features", ms=ms[0], ms_min_max=ms[1:])
            ids = torch.from_numpy(np.random.randint(0, len(buf), size=B)).cuda()
            P = S * FEAT + (S - 1) * A
            moved = B * (S + 1) * FEAT * 4 * 2 + 2 * B * ops.pad_to(P, 4) * 4 + B * (S * A * 2 + A + 2) * 4
            ms = t(lambda: ops.feature_window_gather(buf.features, buf.table, ids, buf.action_, buf.reward_, buf.done_), 200)
            out(bench="feature_window_gather_launch", ms=ms[0], ms_min_max=ms[1:], moved_mb=round(moved / 1e6, 3),
                gb_per_s=round(moved / ms[0] / 1e6, 1), hbm_peak_fraction=round(moved / (ms[0] * 1e-3) / HBM_PEAK, 5))
            # (c) the chain alone
            batch = buf.random_batch(B, frames="features")
            ms = t(lambda: algo.prepare_batch(batch["observations"], batch["actions"]))
            out(bench="prepare_batch_on_features", ms=ms[0], ms_min_max=ms[1:])
            fb = buf.random_batch(B)
            ms = t(lambda: algo.prepare_batch(fb["observations"], fb["actions"]))
            out(bench="prepare_batch_on_frames", ms=ms[0], ms_min_max=ms[1:])
            ms = t(lambda: buf.random_batch(B))
            out(bench="random_batch_frames", ms=ms[0], ms_min_max=ms[1:])
        buf.detach_features()


if __name__ == "__main__":
    main()
