"""N3p measurement: the fused posterior chain under grad in bf16 compute (`LatentModel.chain_grad_compute = "bf16"`,
s2p_posterior_chain_fwd_save_bf16 / s2p_posterior_chain_bwd_bf16) against the fp32 `fused_chain_grad` path of the same build, whose
kernels this mode leaves alone: the yardstick.  Both in ONE process and run.

    python tests/tools/bench_latent_train_chain_bf16.py [--iters 50] [--warmup 5] [--repeats 5] [--skip_iql]

S 8, A 6.  Host-timed figures are the median [min, max] of --repeats repeats of --iters calls between two synchronisations, after
--warmup calls; launches alone are timed by device events (median [min, max] of --repeats measurements).  One JSON line per figure:
  (a) the two launches alone at B 32 and B 256, each on its own and as a pair -- the acceptance: the bf16 pair's [min, max] below
      the fp32 pair's at both;
  (b) the pack launch of the four heads (one s2p_chain_pack_bf16 each) against the torch route (`.to(bfloat16)`, `.t().contiguous()`);
  (c) grad-mode `sample_posterior` + the backward of a sum at B 32 and B 256, warm packs, with the library calls of one call;
  (d) `calculate_loss` + backward + Adam at B 32 on fp32 and bf16 stacks (the parameters change every step: the packs are remade);
  (e) IQL `train_from_torch` with `update_latent`, fp32 and bf16 stacks."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("", "oracle", "tests", os.path.join("tests", "tools")):
    sys.path.insert(0, os.path.join(ROOT, p))
import bench_iql  # noqa: E402
import slac_buffer_ref as SB  # noqa: E402
import slac_latent_ref as REF  # noqa: E402
from bench_feature_cache import out, timed  # noqa: E402
from s2p_amd import ops  # noqa: E402
from s2p_amd.slac import LatentModel, _PosteriorFn  # noqa: E402
from s2p_amd.slac_algo import SlacAlgorithm  # noqa: E402
from slac_chain_util import build_model, count_calls  # noqa: E402

S, A, FEAT, Z, HID = 8, 6, 256, 288, 256
HEADS = ("z1_posterior_init", "z2_prior_init", "z1_posterior", "z2_prior")


def both(latent, make):
    """make() -> the figure, built once per mode with fused_chain_grad on; -> {fp32: ..., bf16: ...}"""
    res = {}
    latent.fused_chain_grad = True
    for mode in ("fp32", "bf16"):
        latent.chain_grad_compute = mode
        res[mode] = make()
    latent.fused_chain_grad, latent.chain_grad_compute = False, "fp32"
    return res


def report(bench, ms, **kw):
    u, f = ms["fp32"], ms["bf16"]
    out(bench=bench, fp32_ms=u[0], fp32_ms_min_max=u[1:], bf16_ms=f[0], bf16_ms_min_max=f[1:], speedup=round(u[0] / f[0], 3),
        saving_ms=round(u[0] - f[0], 4), ranges_apart_and_bf16_faster=bool(f[2] < u[1]), **kw)


def spread(fn, iters, repeats):
    """Device-event time of one fn(), microseconds: [median, min, max] of `repeats` runs of `iters` calls."""
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    v = []
    for _ in range(repeats):
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        v.append(e0.elapsed_time(e1) * 1e3 / iters)
    v.sort()
    return [round(v[len(v) // 2], 2), round(v[0], 2), round(v[-1], 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip_iql", action="store_true")
    a = ap.parse_args()
    t = lambda fn, iters=a.iters: timed(fn, iters, a.warmup, a.repeats)  # noqa: E731
    out(bench="latent_train_chain_bf16", device=torch.cuda.get_device_name(0), S=S, A=A, iters=a.iters, repeats=a.repeats)
    m = build_model(A)
    heads = [getattr(m, h) for h in HEADS]

    for B in (32, 256):
        g = torch.Generator().manual_seed(B)
        feat, action, noise = (torch.randn(B, S + 1, FEAT, generator=g).cuda().requires_grad_(True),
                               torch.randn(B, S, A, generator=g).cuda().requires_grad_(True), torch.randn(B, S + 1, Z, generator=g).cuda())
        params = m._chain_params()

        # (a) the launches alone
        with torch.no_grad():
            packs, bpacks = [h.packed() for h in heads], [h.packed_bf16_grad() for h in heads]
            ra, rb = _PosteriorFn._hoisted(feat, action, packs[2], packs[3])[2:]
            f32 = lambda *s: torch.empty(*s, device="cuda")  # noqa: E731
            mean, std, z = f32(B, S + 1, 32), f32(B, S + 1, 32), f32(B, S + 1, Z)
            a0, b0 = [f32(B, HID), f32(B, HID), f32(B, 64)], [f32(B, HID), f32(B, HID), f32(B, 512)]
            sv = [f32(S, B, HID), f32(S, B, HID), f32(S, B, 64), f32(S, B, HID), f32(S, B, HID), f32(S, B, 512), f32(S, B, Z)]
            grads = [f32(S, B, 64), f32(S, B, HID), f32(S, B, HID), f32(S, B, 512), f32(S, B, HID), f32(S, B, HID), f32(S, B, Z)]
            state = ops.chain_state(a0, b0, sv)
            mlps, bmlps = [ops.chain_mlp(p) for p in packs], [ops.chain_mlp_bwd(packs[2]), ops.chain_mlp_bwd(packs[3])]
            mlps16, bmlps16 = [ops.chain_mlp_bf16(p) for p in bpacks], [ops.chain_mlp_bwd_bf16(bpacks[2]), ops.chain_mlp_bwd_bf16(bpacks[3])]
            dmean, dstd, dz = torch.ones(B, S + 1, 32, device="cuda"), torch.ones(B, S + 1, 32, device="cuda"), torch.ones(B, S + 1, Z, device="cuda")
            fwd32 = lambda: ops.posterior_chain_fwd_save(feat[:, 0], ra, rb, noise, mlps, mean, std, z, state)  # noqa: E731
            fwd16 = lambda: ops.posterior_chain_fwd_save_bf16(feat[:, 0], ra, rb, noise, mlps16, mean, std, z, state)  # noqa: E731
            nosave16 = lambda: ops.posterior_chain_fwd_bf16(feat[:, 0], ra, rb, noise, mlps16, mean, std, z)  # noqa: E731
            bwd32 = lambda: ops.posterior_chain_bwd(noise, dmean, dstd, dz, bmlps, state, grads)  # noqa: E731
            bwd16 = lambda: ops.posterior_chain_bwd_bf16(noise, dmean, dstd, dz, bmlps16, state, grads)  # noqa: E731
            r = {k: spread(fn, a.iters, a.repeats) for k, fn in (("fwd_save_fp32_us", fwd32), ("fwd_save_bf16_us", fwd16), ("fwd_no_save_bf16_us", nosave16),
                                                        ("bwd_fp32_us", bwd32), ("bwd_bf16_us", bwd16),
                                                        ("pair_fp32_us", lambda: (fwd32(), bwd32())), ("pair_bf16_us", lambda: (fwd16(), bwd16())))}
        out(bench="chain_launches_alone", B=B, workgroups=(B + 15) // 16, median_min_max=True, **r,
            fwd_bf16_faster=bool(r["fwd_save_bf16_us"][2] < r["fwd_save_fp32_us"][1]), bwd_bf16_faster=bool(r["bwd_bf16_us"][2] < r["bwd_fp32_us"][1]),
            pair_ranges_apart_and_bf16_faster=bool(r["pair_bf16_us"][2] < r["pair_fp32_us"][1]))

        # (c) sample_posterior under grad + the backward of a sum, warm packs
        def step():
            mean, std, z1, z2 = m.sample_posterior(feat, action, noise)
            return torch.autograd.grad(mean.sum() + std.sum() + z1.sum() + z2.sum(), [feat, action] + params)
        calls = both(m, lambda: count_calls(step))
        report("sample_posterior_grad_and_backward", both(m, lambda: t(step)), B=B, calls_fp32=calls["fp32"], calls_bf16=calls["bf16"])

    # (b) the packs of the four heads: one launch each against the torch route
    def torch_route():
        for h in heads:
            w1, _, w2, _, w3, _ = [p.detach() for p in h.layer_params()]
            (lo, hi), = h.groups[0]
            for w in (w1[:, lo:hi], w2, w3):
                wb = w.to(torch.bfloat16).contiguous()
                wb.t().contiguous()

    def pack_route():
        for h in heads:
            h._bf16g_key = None
            h.packed_bf16_grad()
    with torch.no_grad():
        for h in heads:
            h.packed()
        res = dict(torch_route=t(torch_route), pack_launch=t(pack_route))
        out(bench="bf16_packs_of_the_four_heads", torch_route_ms=res["torch_route"], pack_launch_ms=res["pack_launch"],
            torch_route_device_us=spread(torch_route, a.iters, a.repeats), pack_launch_device_us=spread(pack_route, a.iters, a.repeats),
            calls_pack_launch=count_calls(pack_route))
    del m

    # (d) the latent train step of bench_slac_latent.py
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
        ms = both(lm, lambda: t(train))
        lm.fused_chain_grad = False
        per_layer = t(train)
        report("calculate_loss_backward_adam", ms, B=B, stacks=str(dt).split(".")[-1], per_layer_ms=per_layer[0], per_layer_ms_min_max=per_layer[1:])
        del lm, opt
    if a.skip_iql:
        return

    # (e) IQL train_from_torch with update_latent
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
