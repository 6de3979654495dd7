"""Times the bf16 compute mode of the grouped MLP layers (SPEC.md N3l) against the fp32 mode of the same library, both in one process
and run, at the production sizes (Z 288, A 6, H 1024, P 2090, B 256, num_random 10: 7 936 rows through each Q network).  A report,
not a gate:

    python tests/tools/bench_mlp_bf16.py [--iters 30] [--warmup 5] [--repeats 3]

Prints JSON lines, each as soon as it is measured; every time is the median of the repeats [min, max], a repeat being `iters`
back-to-back calls between two synchronisations:
  `mlp_bf16_launch`  every wide grouped launch of the CQL step alone -- the critics' forward (K 296 and K 1024), their split backward
                     (at the trainer's S), the dgrad through the critics -- and every wide launch of the IQL step (256 and 512
                     rows), through the fp32 entry and the _bf16 entry of the same table, with TFLOP/s against the 157 (fp32) and
                     2 500 (bf16) matrix peaks and `ranges_apart`: the bf16 maximum below the fp32 minimum;
  `mlp_bf16_step`    `train_from_latents` of CQLTrainer and IQLTrainer with mlp_compute "fp32" and "bf16"."""
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
import cql_ref as C  # noqa: E402
import iql_ref as R  # noqa: E402
from s2p_amd._lib import check, lib, ptr, stream  # noqa: E402
from s2p_amd.cql import CQLTrainer, CriticSLAC, Qfunction, TanhGaussianPolicy, Vfunction  # noqa: E402
from s2p_amd.iql import IQLTrainer  # noqa: E402
from s2p_amd.mlp import entry_point  # noqa: E402

Z, A, H, P, B, RN = 288, 6, 1024, 2090, 256, 10
PEAK = {"fp32": 157.0, "bf16": 2500.0}
IQL_CFG = dict(discount=0.99, policy_lr=1e-4, qf_lr=3e-4, reward_scale=1, soft_target_tau=0.005, beta=0.1, quantile=0.7, clip_score=100,
               target_update_period=2)


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


def trainer(kind, dev, critic_sd, policy_sd, mode):
    q = [Qfunction(hidden_sizes=[H, H], output_size=1, input_size=Z + A) for _ in range(4)]
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=[H, H], output_size=1, input_size=Z), device=dev)
    policy = TanhGaussianPolicy(hidden_sizes=[H, H], obs_dim=P, action_dim=A, device=dev)
    critic.load_state_dict(critic_sd)
    policy.load_state_dict(policy_sd)
    if kind == "iql":
        return IQLTrainer(None, policy, critic=critic, mlp_compute=mode, **IQL_CFG)
    cfg = {k: v for k, v in C.CFG.items() if k != "target_entropy"}
    return CQLTrainer(None, policy, critic=critic, mlp_compute=mode, **dict(cfg, num_random=RN, policy_eval_start=0))


def emit(**kw):
    print(json.dumps(kw), flush=True)


def flops(groups, G, N, kind):
    """2 rows K N per group and product: one forward, one for the dgrad, one or two (with an input half) backward."""
    total = 0.0
    for g in groups[:G]:
        total += 2.0 * g.rows * g.K * N * (1 + (1 if kind.startswith("bwd") and g.dprev else 0))
    return total


def launch_rows(who, name, kind, table, splits, ws, a):
    L, st = lib(), stream()
    for i, (gs, G, N, act) in enumerate(table):
        if N <= 16:
            continue
        S = splits[i] if splits else 0
        k = "bwd_split" if S else kind
        row = dict(bench="mlp_bf16_launch", step=who, launch="%s_%d" % (name, i), kind=k, G=G, N=N, K=gs[0].K, rows=[g.rows for g in gs[:G]], S=S)
        fl = flops(gs, G, N, k)
        for mode in ("fp32", "bf16"):
            fn = getattr(L, entry_point(k, N, mode))
            tail = (S, ptr(ws), ws.numel() * 4, st) if S else (st,)
            ms = timed(lambda: check(fn(gs, G, N, act, *tail), k), a.iters, a.warmup, a.repeats)
            tf = fl / (ms[0] * 1e-3) / 1e12
            row[mode] = dict(ms=ms, tflops=round(tf, 1), of_peak=round(tf / PEAK[mode], 3))
        row["speedup"] = round(row["fp32"]["ms"][0] / row["bf16"]["ms"][0], 2)
        row["ranges_apart"] = row["bf16"]["ms"][2] < row["fp32"]["ms"][1]
        emit(**row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    critic_sd, policy_sd = R.init_params(Z, A, H, P, seed=1, last_scale=30.0)
    cb = {k: v.to(dev) for k, v in C.make_batch(B, Z, A, P, 7, terminals=True, scale=0.5).items()}
    noise = {k: v.to(dev) for k, v in C.make_noise(B, A, RN, 8).items()}
    cargs = (cb["z"], cb["next_z"], cb["action"], cb["policy_input"], cb["policy_next_input"], cb["rewards"], cb["terminals"])
    iargs = (cb["z"], cb["next_z"], cb["action"], cb["policy_input"], cb["rewards"], cb["terminals"])
    # the launches alone, on the tables (and the data of one step) of an fp32-mode trainer
    tr = trainer("cql", dev, critic_sd, policy_sd, "fp32")
    tr.train_from_latents(*cargs, noise=noise)
    t = tr._tables(B)
    launch_rows("cql", "critic_fwd", "fwd", t["critic_fwd"], None, None, a)
    launch_rows("cql", "critic_bwd", "bwd", t["critic_bwd"], t["critic_split"], t["split_ws"], a)
    launch_rows("cql", "qpol_dgrad", "dgrad", t["qpol_dgrad"], None, None, a)
    ti = trainer("iql", dev, critic_sd, policy_sd, "fp32")
    ti.train_from_latents(*iargs)
    t = ti._tables(B)
    launch_rows("iql", "fwd", "fwd", t["fwd"], None, None, a)
    launch_rows("iql", "bwd", "bwd", t["bwd"], None, None, a)
    del tr, ti
    for kind, step_args, kw in (("cql", cargs, dict(noise=noise)), ("iql", iargs, {})):
        row = dict(bench="mlp_bf16_step", trainer=kind, Z=Z, A=A, H=H, P=P, B=B, num_random=RN, iters=a.iters, repeats=a.repeats)
        for mode in ("fp32", "bf16"):
            tr = trainer(kind, dev, critic_sd, policy_sd, mode)
            row[mode + "_ms"] = timed(lambda: tr.train_from_latents(*step_args, **kw), a.iters, a.warmup, a.repeats)
            row[mode + "_calls"] = {k: v for k, v in tr.launches.items() if k.startswith("s2p_mlp_linear_")}
        row["speedup"] = round(row["fp32_ms"][0] / row["bf16_ms"][0], 3)
        row["ranges_apart"] = row["bf16_ms"][2] < row["fp32_ms"][1]
        emit(**row)


if __name__ == "__main__":
    main()
