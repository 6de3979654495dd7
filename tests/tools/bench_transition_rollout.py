"""N2c measurement: the state-transition rollout of a whole dataset.  Workload of the reference: N = 500 000 rows in 500 trajectories
of 1 000, obs 17, A 6, E 7, H 256, 3 hidden layers.  Three forms, timed in one process, median of 5 runs with min and max:
  1. sweep  -- the device part of transition_rollout.generate: EnsembleTransition.rollout_sweep from host arrays to host arrays
               (uploads and downloads included);
  2. step   -- what the package offered before the sweep: per trajectory, host normalise + concat + rollout_step + .cpu();
  3. torch  -- the reference's own form: tests/transition_rollout_ref.py with the ensemble on torch's device ops.
Also: the sweep on device-resident inputs (its fp32 TFLOP/s against the 157 TFLOP/s matrix peak) and the pack launch alone (GB/s).
    python tests/tools/bench_transition_rollout.py [--rows 500000] [--traj 500] [--runs 5] [--chunk 16384]
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("", "oracle", "tests"):
    sys.path.insert(0, os.path.join(R, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ensemble_oracle as EO  # noqa: E402
import transition_rollout_ref as REF  # noqa: E402
from s2p_amd import ops, transition_rollout as TR  # noqa: E402
from s2p_amd.dynamics import EnsembleTransition  # noqa: E402


def timed(fn, runs):
    fn()                                                      # warm-up: allocator, first launches
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return dict(median_ms=round(float(np.median(ts)), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=500000)
    ap.add_argument("--traj", type=int, default=500)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=16384)
    a = ap.parse_args(argv)
    N, T, E, H, OD, A = a.rows, a.traj, 7, 256, 17, 6
    assert N % T == 0 and N // T > 8
    dev = torch.device("cuda:0")
    m = EnsembleTransition(OD, A, H, 3, ensemble_size=E).init_parameters(0)
    sd = m.state_dict()
    r = np.random.RandomState(0)
    scale, shift = r.uniform(0.2, 5.0, OD).astype(np.float32), r.uniform(-3, 3, OD).astype(np.float32)
    obs = (r.randn(N, OD) * scale + shift).astype(np.float32)
    timeouts = np.zeros(N, dtype=bool)
    timeouts[N // T - 1::N // T] = True
    data = dict(observations=obs, actions=r.uniform(-1, 1, (N, A)).astype(np.float32), rewards=r.randn(N).astype(np.float32),
                next_observations=obs, terminals=np.zeros(N, dtype=bool), timeouts=timeouts)
    cfg = dict(obs_mean=shift, obs_std=scale, next_obs_mean=shift, next_obs_std=scale, reward_mean=2.991, reward_std=1.092)
    stats = tuple(cfg[k] for k in TR.CFG_KEYS)
    starts, ends = TR.trajectories(timeouts)
    actions, members = TR.draw(starts, ends, -1.0, 1.0, E, 0, action_dim=A)

    def sweep():
        return [t.cpu().numpy() for t in m.rollout_sweep(obs, actions, members, *stats, chunk=a.chunk)]

    def step():
        out = []
        for s, e in zip(starts.tolist(), ends.tolist()):
            x = np.concatenate([(obs[s:e + 1] - shift) / scale, actions[s:e + 1]], 1)
            out.append([t.cpu().numpy() for t in m.rollout_step(torch.from_numpy(x), members[s:e + 1], *stats[2:])])
        return [np.concatenate(c, 0) for c in zip(*out)]

    sd_dev = {k: v.to(dev) for k, v in sd.items() if "saved" not in k}

    def torch_form():
        return REF.rollout(data, cfg, lambda x: EO.ensemble_forward(sd_dev, x, OD), -1.0, 1.0, 0, n_members=E, device=dev)

    res = dict(rows=N, trajectories=T, E=E, H=H, chunk=a.chunk, runs=a.runs, device=torch.cuda.get_device_name(0))
    got, want = sweep(), step()
    res["sweep_vs_step_rel_err"] = max(float(np.abs(g - w).max() / np.abs(w).max()) for g, w in zip(got, want))
    res["sweep"], res["step"], res["torch"] = timed(sweep, a.runs), timed(step, a.runs), timed(torch_form, a.runs)
    # the device part alone, inputs resident: compute rate of the layer chain
    od, ad, md = torch.from_numpy(obs).to(dev), torch.from_numpy(actions).to(dev), torch.from_numpy(members).to(dev)
    res["sweep_device_only"] = timed(lambda: m.rollout_sweep(od, ad, md, *stats, chunk=a.chunk), a.runs)
    flop = 2.0 * E * ((OD + A) * H + 2 * H * H + H * 2 * (OD + 1)) * N
    res["sweep_tflops_fp32"] = round(flop / (res["sweep_device_only"]["median_ms"] * 1e-3) / 1e12, 2)
    res["fraction_of_157_tflops_peak"] = round(res["sweep_tflops_fp32"] / 157.0, 3)
    x, om, os_ = torch.empty((N, 24), device=dev), torch.from_numpy(shift).to(dev), torch.from_numpy(scale).to(dev)
    res["pack_x20"] = timed(lambda: [ops.transition_pack(od, ad, om, os_, x) for _ in range(20)], a.runs)   # 20 launches back to back
    res["pack_gbs"] = round((OD + A + 24) * 4.0 * N / (res["pack_x20"]["median_ms"] / 20 * 1e-3) / 1e9, 1)
    res["sweep_over_step"] = round(res["sweep"]["median_ms"] / res["step"]["median_ms"], 3)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
