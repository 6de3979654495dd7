"""Times one CQL step on SLAC latents (SPEC.md N3e) at the production sizes (Z 288, A 6, H 1024, P 2090, B 256, num_random 10:
7 936 rows through each Q network) on the HIP path against the same step in torch's own ROCm ops (the restatement of
tests/cql_ref.py, eager, torch.optim.Adam) in the same process and run.  A report, not a gate:

    python tests/tools/bench_cql.py [--iters 100] [--warmup 10] [--repeats 5] [--buffer] [--buffer_iters 30]

Prints JSON lines, each as soon as it is measured: `cql_train_from_latents` (ms per step, median of the repeats [min, max]; each
repeat is `iters` back-to-back steps between two synchronisations; the library calls and torch copies of a step by name),
`cql_split_backward` (each wide critic layer's backward on all its rows with s2p_mlp_linear_bwd and with s2p_mlp_linear_bwd_split
at S = 1, 2, 4, 8), `cql_grouped_launches` (every grouped launch alone with its fp32 TFLOP/s against the 157 TFLOP/s matrix peak;
`critic_bwd` there is the unsplit form), `cql_torch_eager_step`, and with --buffer `cql_train_from_torch` on a synthetic 100x100x3 buffer with freeze_slac and with the latent update."""
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
from s2p_amd._lib import check, lib, stream  # noqa: E402
from s2p_amd.cql import CQLTrainer, CriticSLAC, Qfunction, TanhGaussianPolicy, Vfunction  # noqa: E402

Z, A, H, P, B, RN = 288, 6, 1024, 2090, 256, 10
CFG = dict(C.CFG, num_random=RN, policy_eval_start=0)
PEAK_TFLOPS = 157.0


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


def trainer(dev, critic_sd=None, policy_sd=None, p=P, **kw):
    q = [Qfunction(hidden_sizes=[H, H], output_size=1, input_size=Z + A) for _ in range(4)]
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=[H, H], output_size=1, input_size=Z), device=dev)
    policy = TanhGaussianPolicy(hidden_sizes=[H, H], obs_dim=p, action_dim=A, device=dev)
    if critic_sd is not None:
        critic.load_state_dict(critic_sd)
        policy.load_state_dict(policy_sd)
    cfg = {k: v for k, v in CFG.items() if k != "target_entropy"}
    return CQLTrainer(None, policy, critic=critic, **dict(cfg, **kw))


def eager_stepper(critic_sd, policy_sd, batch, noise, dev):
    """tests/cql_ref.py's step on the device: the parameters, `log_alpha` and the three torch.optim.Adam objects live across the
    steps (cql_ref.Stepper), as the HIP trainer's do."""
    st = C.Stepper({k: v.to(dev) for k, v in critic_sd.items()}, {k: v.to(dev) for k, v in policy_sd.items()}, torch.float32, CFG)
    return lambda: st.step(batch, noise)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def launch_flops(groups, G, N, backward):
    """2 rows K N per group forward; the backward's weight and input halves are one such product each (the first layer has no input half)."""
    total = 0
    for g in groups[:G]:
        one = 2.0 * g.rows * g.K * N
        total += one * ((1 + (1 if g.dprev else 0)) if backward else 1)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--eager_iters", type=int, default=20)
    ap.add_argument("--buffer", action="store_true", help="also time train_from_torch on a synthetic frame buffer")
    ap.add_argument("--buffer_iters", type=int, default=30)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    critic_sd, policy_sd = R.init_params(Z, A, H, P, seed=1, last_scale=30.0)
    batch = {k: v.to(dev) for k, v in C.make_batch(B, Z, A, P, 7, terminals=True, scale=0.5).items()}
    noise = {k: v.to(dev) for k, v in C.make_noise(B, A, RN, 8).items()}
    tr = trainer(dev, critic_sd, policy_sd)
    args = (batch["z"], batch["next_z"], batch["action"], batch["policy_input"], batch["policy_next_input"], batch["rewards"], batch["terminals"])
    # every line is printed as soon as it is measured: a stage that fails loses only itself
    common = dict(Z=Z, A=A, H=H, P=P, B=B, num_random=RN, iters=a.iters, repeats=a.repeats)
    hip = timed(lambda: tr.train_from_latents(*args, noise=noise), a.iters, a.warmup, a.repeats)
    launches = dict(tr.launches)
    t, L, st = tr._tables(B), lib(), stream()
    emit(bench="cql_train_from_latents", q_rows=t["M"], hip_ms=hip[0], hip_ms_min_max=hip[1:], calls_per_step=launches,
         library_calls_per_step=sum(v for k, v in launches.items() if k.startswith("s2p_")),
         torch_copies_per_step=launches.get("torch copy", 0), split_S_per_critic_bwd_launch=t["critic_split"], **common)
    own = timed(lambda: tr.train_from_latents(*args), a.iters, a.warmup, a.repeats)
    emit(bench="cql_train_from_latents_drawing_its_noise", hip_ms=own[0], hip_ms_min_max=own[1:], calls_per_step=dict(tr.launches), **common)
    # the critics' wide layers on all their rows: s2p_mlp_linear_bwd (one wave per weight tile) against the row split
    ws = t["split_ws"]
    for i, ((gs, G, N, act), S_used) in enumerate(zip(t["critic_bwd"], t["critic_split"])):
        if N <= 16:
            continue
        row = {"S_in_the_trainer": S_used, "unsplit": timed(lambda: check(L.s2p_mlp_linear_bwd(gs, G, N, act, st), "bwd"), a.iters, a.warmup, 3)}
        for S in (1, 2, 4, 8):
            need = L.s2p_mlp_linear_bwd_split_workspace(gs, G, N, S)
            if need > ws.numel() * 4:
                ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
            row["S%d" % S] = timed(lambda: check(L.s2p_mlp_linear_bwd_split(gs, G, N, act, S, ws.data_ptr(), ws.numel() * 4, st), "split"),
                                   a.iters, a.warmup, 3)
        emit(bench="cql_split_backward", launch="critic_bwd_%d_G%d_N%d_K%d" % (i, G, N, gs[0].K), rows=t["M"], ms_median_min_max=row)
    for name, entry, backward in (("policy_fwd", "s2p_mlp_linear_fwd", False), ("qpol_fwd", "s2p_mlp_linear_fwd", False),
                                  ("qpol_dgrad", "s2p_mlp_linear_dgrad", True), ("policy_bwd", "s2p_mlp_linear_bwd", True),
                                  ("policy2_fwd", "s2p_mlp_linear_fwd", False), ("critic_fwd", "s2p_mlp_linear_fwd", False),
                                  ("critic_bwd", "s2p_mlp_linear_bwd", True)):
        fn, stages = getattr(L, entry), {}
        for i, (gs, G, N, act) in enumerate(t[name]):
            ms = timed(lambda: check(fn(gs, G, N, act, st), entry), a.iters, a.warmup, 3)
            flops = launch_flops(gs, G, N, backward)
            if entry == "s2p_mlp_linear_dgrad":
                flops /= 2                      # (the input half alone)
            stages["%s_%d_G%d_N%d" % (name, i, G, N)] = dict(ms=ms, tflops=round(flops / (ms[0] * 1e-3) / 1e12, 2),
                                                              of_peak=round(flops / (ms[0] * 1e-3) / 1e12 / PEAK_TFLOPS, 3))
        emit(bench="cql_grouped_launches", table=name, entry=entry, launches=stages)
    ref = timed(eager_stepper(critic_sd, policy_sd, batch, noise, dev), a.eager_iters, 3, a.repeats)
    emit(bench="cql_torch_eager_step", torch_eager_ms=ref[0], torch_eager_ms_min_max=ref[1:], hip_ms=hip[0], speedup=round(ref[0] / hip[0], 2),
         iters=a.eager_iters, repeats=a.repeats)
    if not a.buffer:
        return
    import slac_buffer_ref as SB
    from s2p_amd.slac_algo import SlacAlgorithm
    data = SB.real_dataset(4, 80, 100, 100)
    for name, freeze in (("freeze_slac", True), ("with_update_latent_fp32", False)):
        algo = SlacAlgorithm((3, 100, 100), (SB.A,), 1, dev, seed=0, buffer_size=512, num_sequences=SB.S, frame_capacity=1024)
        algo.load_data_in_buffer(data, **dict(SB.LOAD_ARGS["real"], data_num=320))
        trb = trainer(dev, p=SB.S * 256 + (SB.S - 1) * SB.A, slac_algo=algo, freeze_slac=freeze)
        ms = timed(lambda: trb.train_from_torch(algo.buffer.random_batch(B)), a.buffer_iters, 3, a.repeats)
        print(json.dumps({"bench": "cql_train_from_torch", "case": name, "B": B, "windows": len(algo.buffer), "hip_ms": ms[0],
                          "hip_ms_min_max": ms[1:], "iters": a.buffer_iters, "repeats": a.repeats}), flush=True)


if __name__ == "__main__":
    main()
