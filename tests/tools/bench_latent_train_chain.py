"""N3k measurement: the posterior chain under grad as one launch per direction (`LatentModel.fused_chain_grad`,
s2p_posterior_chain_fwd_save / s2p_posterior_chain_bwd) against the per-layer path (the behaviour without the flag, whose code
this change leaves alone: the yardstick), both in ONE process and run.

    python tests/tools/bench_latent_train_chain.py [--iters 50] [--warmup 5] [--repeats 5] [--skip_iql]

S 8, A 6.  Every figure is the median [min, max] of --repeats repeats of --iters calls between two synchronisations, after --warmup
calls.  One JSON line per figure, each with `per_layer` and `fused`:
  (a) grad-mode `sample_posterior` + the backward of a sum, at B 32 and B 256, with the library calls of one call -- the
      acceptance: fused faster at both, the two [min, max] ranges apart;
  (b) each new launch alone (device events), with its share of one CU's fp32 MFMA rate (the yardstick of DESIGN.md 6b.11);
  (c) `calculate_loss` + backward + Adam at B 32 on fp32 and bf16 stacks (the step of tests/tools/bench_slac_latent.py);
  (d) IQL `train_from_torch` with `update_latent`, fp32 and bf16 stacks (the cases of tests/tools/bench_iql.py --buffer)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("", "tests", os.path.join("tests", "tools")):
    sys.path.insert(0, os.path.join(ROOT, p))
import bench_actor  # noqa: E402
import bench_iql  # noqa: E402
import slac_buffer_ref as SB  # noqa: E402
import slac_latent_ref as REF  # noqa: E402
from bench_feature_cache import out, timed  # noqa: E402
from bench_posterior_chain import CU_FP32_MFMA_FLOPS_PER_CYCLE, MACS_PER_ROW, MACS_PER_ROW_STEP  # noqa: E402
from s2p_amd import ops  # noqa: E402
from s2p_amd.slac import LatentModel, _PosteriorFn  # noqa: E402
from s2p_amd.slac_algo import SlacAlgorithm  # noqa: E402
from slac_chain_util import build_model, count_calls  # noqa: E402

S, A, FEAT, Z, HID = 8, 6, 256, 288, 256
BWD_MACS_PER_ROW_STEP = (512 * 256 + 256 * 256 + 256 * 288) + (64 * 256 + 256 * 256 + 256 * 256)    # the six dgrads of a step


def both(latent, make):
    """make() -> the figure, built once per setting of the flag; -> {per_layer: ..., fused: ...}"""
    res = {}
    for name, on in (("per_layer", False), ("fused", True)):
        latent.fused_chain_grad = on
        res[name] = make()
    latent.fused_chain_grad = False
    return res


def report(bench, ms, **kw):
    u, f = ms["per_layer"], ms["fused"]
    out(bench=bench, per_layer_ms=u[0], per_layer_ms_min_max=u[1:], fused_ms=f[0], fused_ms_min_max=f[1:], speedup=round(u[0] / f[0], 3),
        saving_ms=round(u[0] - f[0], 4), ranges_apart_and_fused_faster=bool(f[2] < u[1]), **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip_iql", action="store_true")
    a = ap.parse_args()
    t = lambda fn, iters=a.iters: timed(fn, iters, a.warmup, a.repeats)  # noqa: E731
    out(bench="latent_train_chain", device=torch.cuda.get_device_name(0), S=S, A=A, iters=a.iters, repeats=a.repeats)
    m = build_model(A)
    clock_hz = getattr(torch.cuda.get_device_properties(0), "clock_rate", 2400000) * 1e3
    share = lambda flops, us: round(flops / (us * 1e-6) / (CU_FP32_MFMA_FLOPS_PER_CYCLE * clock_hz), 3)  # noqa: E731

    for B in (32, 256):
        g = torch.Generator().manual_seed(B)
        feat, action, noise = (torch.randn(B, S + 1, FEAT, generator=g).cuda().requires_grad_(True),
                               torch.randn(B, S, A, generator=g).cuda().requires_grad_(True), torch.randn(B, S + 1, Z, generator=g).cuda())
        params = m._chain_params()

        # (a) sample_posterior under grad + the backward of a sum
        def step():
            mean, std, z1, z2 = m.sample_posterior(feat, action, noise)
            return torch.autograd.grad(mean.sum() + std.sum() + z1.sum() + z2.sum(), [feat, action] + params)
        calls = both(m, lambda: count_calls(step))
        same = both(m, lambda: [x.clone() for x in step()])
        report("sample_posterior_grad_and_backward", both(m, lambda: t(step)), B=B, calls_per_layer=calls["per_layer"],
               calls_fused=calls["fused"], calls_total=[sum(calls["per_layer"].values()), sum(calls["fused"].values())],
               bitwise_equal=all(torch.equal(x, y) for x, y in zip(same["per_layer"], same["fused"])))

        # (b) each new launch alone
        with torch.no_grad():
            packs = [h.packed() for h in (m.z1_posterior_init, m.z2_prior_init, m.z1_posterior, m.z2_prior)]
            ra, rb = _PosteriorFn._hoisted(feat, action, packs[2], packs[3])[2:]
            f32 = lambda *s: torch.empty(*s, device="cuda")  # noqa: E731
            mean, std, z = f32(B, S + 1, 32), f32(B, S + 1, 32), f32(B, S + 1, Z)
            a0, b0 = [f32(B, HID), f32(B, HID), f32(B, 64)], [f32(B, HID), f32(B, HID), f32(B, 512)]
            sv = [f32(S, B, HID), f32(S, B, HID), f32(S, B, 64), f32(S, B, HID), f32(S, B, HID), f32(S, B, 512), f32(S, B, Z)]
            grads = [f32(S, B, 64), f32(S, B, HID), f32(S, B, HID), f32(S, B, 512), f32(S, B, HID), f32(S, B, HID), f32(S, B, Z)]
            state, mlps = ops.chain_state(a0, b0, sv), [ops.chain_mlp(p) for p in packs]
            bmlps = [ops.chain_mlp_bwd(packs[2]), ops.chain_mlp_bwd(packs[3])]
            dmean, dstd, dz = torch.ones(B, S + 1, 32, device="cuda"), torch.ones(B, S + 1, 32, device="cuda"), torch.ones(B, S + 1, Z, device="cuda")
            fwd_us = bench_actor.kernel_us(lambda: ops.posterior_chain_fwd_save(feat[:, 0], ra, rb, noise, mlps, mean, std, z, state))
            nosave_us = bench_actor.kernel_us(lambda: ops.posterior_chain_fwd(feat[:, 0], ra, rb, noise, mlps, mean, std, z))
            bwd_us = bench_actor.kernel_us(lambda: ops.posterior_chain_bwd(noise, dmean, dstd, dz, bmlps, state, grads))
        fwd_flops, bwd_flops = 2.0 * 16 * (MACS_PER_ROW + S * MACS_PER_ROW_STEP), 2.0 * 16 * S * BWD_MACS_PER_ROW_STEP
        out(bench="chain_launches_alone", B=B, workgroups=(B + 15) // 16, clock_mhz=round(clock_hz / 1e6), fwd_save_us=round(fwd_us, 2),
            fwd_no_save_us=round(nosave_us, 2), bwd_us=round(bwd_us, 2), fwd_mflop_per_workgroup=round(fwd_flops / 1e6, 2),
            bwd_mflop_per_workgroup=round(bwd_flops / 1e6, 2), fwd_save_share_of_one_cu_fp32_mfma_rate=share(fwd_flops, fwd_us),
            bwd_share_of_one_cu_fp32_mfma_rate=share(bwd_flops, bwd_us))
    del m

    # (c) the latent train step of bench_slac_latent.py
    B = 32
    g = torch.Generator().manual_seed(0)
    frames = (torch.rand(B, S + 1, 100, 100, 3, generator=g) * 255).to(torch.uint8).cuda()
    action, reward = torch.randn(B, S, A, generator=g).cuda(), torch.randn(B, S, 1, generator=g).cuda()
    done = (torch.rand(B, S, 1, generator=g) < 0.1).float().cuda()
    params = REF.make_params(A)
    for dt in (torch.float32, torch.bfloat16):
        lm = LatentModel((3, 100, 100), (A,), image_size=100, dtype=dt)
        lm.load_state_dict(REF.full_state_dict(params))
        opt = torch.optim.Adam(lm.parameters(), lr=1e-4)

        def train():
            opt.zero_grad(set_to_none=True)
            sum(lm.calculate_loss(frames, action, reward, done)).backward()
            opt.step()
        report("calculate_loss_backward_adam", both(lm, lambda: t(train)), B=B, stacks=str(dt).split(".")[-1])
        del lm, opt
    if a.skip_iql:
        return

    # (d) IQL train_from_torch with update_latent
    data = SB.real_dataset(4, 80, 100, 100)
    for dt in (torch.float32, torch.bfloat16):
        algo = SlacAlgorithm((3, 100, 100), (SB.A,), 1, "cuda:0", seed=0, buffer_size=512, num_sequences=SB.S, frame_capacity=1024, dtype=dt)
        algo.load_data_in_buffer(data, **dict(SB.LOAD_ARGS["real"], data_num=320))

        def make():
            tr = bench_iql.trainer("cuda:0", slac_algo=algo, freeze_slac=False)
            return t(lambda: tr.train_from_torch(algo.buffer.random_batch(bench_iql.B)))
        report("iql_train_from_torch_with_update_latent", both(algo.latent, make), B=bench_iql.B, stacks=str(dt).split(".")[-1])
        del algo


if __name__ == "__main__":
    main()
