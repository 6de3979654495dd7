"""Times one IQL step on SLAC latents (SPEC.md N3d) at the production sizes (Z 288, A 6, H 1024, P 2090, B 256) on the HIP path
against the same networks and the same step in torch's own ROCm ops (the restatement of tests/iql_ref.py, eager, torch.optim.Adam)
in the same process and run.  A report, not a gate:

    python tests/tools/bench_iql.py [--iters 200] [--warmup 30] [--repeats 5] [--buffer] [--buffer_iters 50]

Prints JSON lines: `iql_train_from_latents` (ms per step, median of the repeats [min, max]; each repeat is `iters` back-to-back steps
between two synchronisations; library calls and kernel launches per step; the stages of the HIP step timed the same way), and with
--buffer `iql_train_from_torch` on a synthetic 100x100x3 buffer: with freeze_slac, and the full step with update_latent on the fp32
and the bf16 conv stacks."""
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
import iql_ref as R  # noqa: E402
from s2p_amd._lib import check, lib, stream  # noqa: E402
from s2p_amd.iql import CriticSLAC, IQLTrainer, Qfunction, TanhGaussianPolicy, Vfunction  # noqa: E402
from s2p_amd.mlp import run  # noqa: E402

Z, A, H, P, B = 288, 6, 1024, 2090, 256
CFG = dict(discount=0.99, policy_lr=1e-4, qf_lr=3e-4, reward_scale=1, soft_target_tau=0.005, beta=0.1, quantile=0.7, clip_score=100,
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


def trainer(dev, critic_sd=None, policy_sd=None, p=P, **kw):
    q = [Qfunction(hidden_sizes=[H, H], output_size=1, input_size=Z + A) for _ in range(4)]
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=[H, H], output_size=1, input_size=Z), device=dev)
    policy = TanhGaussianPolicy(hidden_sizes=[H, H], obs_dim=p, action_dim=A, device=dev)
    if critic_sd is not None:
        critic.load_state_dict(critic_sd)
        policy.load_state_dict(policy_sd)
    return IQLTrainer(None, policy, critic=critic, **dict(CFG, **kw))


def eager_stepper(critic_sd, policy_sd, batch, dev):
    critic = {k: v.to(dev).clone().requires_grad_(not k.startswith("target")) for k, v in critic_sd.items()}
    policy = {k: v.to(dev).clone().requires_grad_(True) for k, v in policy_sd.items()}
    opt_c = torch.optim.Adam([v for k, v in critic.items() if not k.startswith("target")], lr=CFG["qf_lr"])
    opt_p = torch.optim.Adam(list(policy.values()), lr=CFG["policy_lr"])
    src = [(critic["target_" + k], v) for k, v in critic.items() if k.startswith(("qf1.", "qf2."))]
    n = [0]

    def step():
        out = R.losses(critic, policy, batch)
        opt_c.zero_grad(set_to_none=True)
        (out["qf1_loss"] + out["qf2_loss"] + out["vf_loss"]).backward()
        opt_c.step()
        opt_p.zero_grad(set_to_none=True)
        out["policy_loss"].backward()
        opt_p.step()
        if n[0] % CFG["target_update_period"] == 0:
            with torch.no_grad():
                for tgt, v in src:
                    tgt.copy_(tgt * (1.0 - CFG["soft_target_tau"]) + v * CFG["soft_target_tau"])
        n[0] += 1
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--buffer", action="store_true", help="also time train_from_torch on a synthetic frame buffer")
    ap.add_argument("--buffer_iters", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    critic_sd, policy_sd = R.init_params(Z, A, H, P, seed=1, last_scale=30.0)
    batch = {k: v.to(dev) for k, v in R.make_batch(B, Z, A, P, 7, terminals=True, scale=0.5, extreme_rows=None).items()}
    tr = trainer(dev, critic_sd, policy_sd)
    args = (batch["z"], batch["next_z"], batch["action"], batch["policy_input"], batch["rewards"], batch["terminals"])
    hip = timed(lambda: tr.train_from_latents(*args), a.iters, a.warmup, a.repeats)
    ref = timed(eager_stepper(critic_sd, policy_sd, batch, dev), a.iters, a.warmup, a.repeats)
    t, L, st = tr._tables(B), lib(), stream()
    calls = len(t["fwd"]) + 2 + len(t["bwd"]) + 2 + 0.5
    stages = {
        "staging_copies": timed(lambda: _stage(tr, t, args), a.iters, a.warmup, 3),
        "forward_%d_launches" % len(t["fwd"]): timed(lambda: run(t["fwd"]), a.iters, a.warmup, 3),
        "backward_%d_launches" % len(t["bwd"]): timed(lambda: run(t["bwd"], "s2p_mlp_linear_bwd"), a.iters, a.warmup, 3),
        "two_adam_steps": timed(lambda: (tr.critic_optimizer.step(), tr.policy_optimizer.step()), a.iters, a.warmup, 3),
    }
    for i, (g, G, N, act) in enumerate(t["fwd"]):
        stages["forward_launch_%d_G%d_N%d" % (i, G, N)] = timed(lambda: check(L.s2p_mlp_linear_fwd(g, G, N, act, st), "fwd"), a.iters, a.warmup, 3)
    for i, (g, G, N, act) in enumerate(t["bwd"]):
        stages["backward_launch_%d_G%d_N%d" % (i, G, N)] = timed(lambda: check(L.s2p_mlp_linear_bwd(g, G, N, act, st), "bwd"), a.iters, a.warmup, 3)
    print(json.dumps({"bench": "iql_train_from_latents", "Z": Z, "A": A, "H": H, "P": P, "B": B, "hip_ms": hip[0], "hip_ms_min_max": hip[1:],
                      "torch_eager_ms": ref[0], "torch_eager_ms_min_max": ref[1:], "speedup": round(ref[0] / hip[0], 2),
                      "library_calls_per_step": calls, "kernel_launches_per_step": calls + 2, "staging_copies_per_step": 8,
                      "stages_ms_median_min_max": stages, "iters": a.iters, "repeats": a.repeats}), flush=True)
    if not a.buffer:
        return
    import slac_buffer_ref as SB
    from s2p_amd.slac_algo import SlacAlgorithm
    data = SB.real_dataset(4, 80, 100, 100)
    for name, dtype, freeze in (("freeze_slac", torch.float32, True), ("with_update_latent_fp32", torch.float32, False),
                                ("with_update_latent_bf16", torch.bfloat16, False)):
        algo = SlacAlgorithm((3, 100, 100), (SB.A,), 1, dev, seed=0, buffer_size=512, num_sequences=SB.S, frame_capacity=1024, dtype=dtype)
        algo.load_data_in_buffer(data, **dict(SB.LOAD_ARGS["real"], data_num=320))
        trb = trainer(dev, slac_algo=algo, freeze_slac=freeze)
        ms = timed(lambda: trb.train_from_torch(algo.buffer.random_batch(B)), a.buffer_iters, 5, a.repeats)
        print(json.dumps({"bench": "iql_train_from_torch", "case": name, "B": B, "windows": len(algo.buffer), "hip_ms": ms[0],
                          "hip_ms_min_max": ms[1:], "iters": a.buffer_iters, "repeats": a.repeats}), flush=True)


def _stage(tr, t, args):
    z, next_z, action, policy_input, rewards, terminals = args
    t["xq"][:, :Z] = z
    t["xq"][:, Z:Z + A] = action
    t["xv"][:B, :Z] = t["xq"][:, :Z]
    t["xv"][B:, :Z] = next_z
    t["xp"][:, :P] = policy_input
    t["action"].copy_(action)
    t["reward"].copy_(rewards.reshape(B))
    t["terminal"].copy_(terminals.reshape(B))


if __name__ == "__main__":
    main()
