"""N3o measurement: the closed-loop rollout of a `feature_action` policy (`LatentModel.imagine_feature_action`: policy, prior step,
decoder, s2p_decoded_to_frames, encoder, s2p_feature_action_push per step) against the same loop written from the pieces the package
offered before it (the yardstick: `policy.act`, a one-step `predict`, `Decoder.forward`, torch `clamp` / `round` / `div`,
`Encoder.forward` on the float frames, `torch.cat` shifting), both in ONE process and run.

    python tests/tools/bench_imagine_feature_action.py [--iters 20] [--warmup 3] [--repeats 5] [--horizon 16] [--batches 32,256]
                                                       [--widths 256,1024] [--dtypes fp32,bf16]

Sizes: S 8, A 6 (obs_dim 2090), H 16, B 32 and 256, policy width 256 and 1024, fp32 and bf16 conv stacks.  Every wall-clock figure is
the median [min, max] of --repeats repeats of --iters calls between two synchronisations, after --warmup calls.  One JSON line per
figure:
  (a) `imagine_feature_action` and the yardstick loop, ms per call, and whether their first actions agree;
  (b) the pieces of one step alone (device events, us): policy, prior step, decoder, hand-off, encoder, push;
  (c) the hand-off launch alone with its GB/s (bytes read + written) against the 8 TB/s HBM peak;
  (d) `imagined_returns` end to end at context 8, B 256, for a `latent_z` and a `feature_action` policy of equal width."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("", "tests", os.path.join("tests", "tools")):
    sys.path.insert(0, os.path.join(ROOT, p))
import bench_actor  # noqa: E402
from bench_feature_cache import out, timed  # noqa: E402
from s2p_amd import ops  # noqa: E402
from s2p_amd._lib import chunk_elems  # noqa: E402
from s2p_amd.offline_rl import TanhGaussianPolicy  # noqa: E402
from s2p_amd.slac import HID, LatentModel, _chain_step, _f32  # noqa: E402
from s2p_amd.slac_imagine import imagined_returns  # noqa: E402

S, A, Z, Z1, Z2, F, CONTEXT = 8, 6, 288, 32, 256, 256, 8
P = S * F + (S - 1) * A
NF = S * F
HBM_PEAK = 8e12


def yardstick(latent, po, z0, window, noise, H):
    """The rollout from the pieces of the package before `imagine_feature_action`; -> actions [B,H,A]."""
    z, acts = z0, []
    with torch.no_grad():
        for h in range(H):
            a = po.act(window)
            acts.append(a)
            z = latent.predict(z, a[:, None].contiguous(), noise[:, h:h + 1].contiguous())[2][:, 0]
            if h == H - 1:
                break
            img = latent.decoder(z[:, None])[0]
            img = torch.round(img.clamp_(0.0, 1.0) * 255.0) / 255.0
            f = latent.encoder(img)[:, 0]
            window = torch.cat([window[:, F:NF], f, window[:, NF + A:], a], dim=1)
    return torch.stack(acts, 1)


def step_pieces(latent, po, B, g):
    """us of each piece of one step at batch B, each alone between device events."""
    dev, dt = latent.device, latent.decoder.dtype
    z0, noise = torch.randn(B, Z, generator=g).cuda(), torch.randn(B, 1, Z, generator=g).cuda()
    _, (mean, std, z), (g1, g2, p1, p2, wc, wb, xz) = latent._rollout_start(z0, 1, noise, True)
    win = [_f32((B, (P + 3) // 4 * 4), dev, True) for _ in range(2)]
    a = _f32((B, 8), dev, True)
    rc, rb, h1, h2 = (_f32((B, HID), dev) for _ in range(4))
    bufa, bufb = (h1, h2, _f32((B, g1.Npad), dev)), (h1, h2, _f32((B, g2.Npad), dev))
    zin = torch.randn(B, 1, 1, Z, generator=g).to(dt).cuda()
    xin = torch.empty((B, 100, 100, chunk_elems(dt)), dtype=dt, device=dev)
    u8 = torch.empty((B, 100, 100, 3), dtype=torch.uint8, device=dev)

    def prior():
        ops.linear_fwd_into(a, wc, None, HID, rc)
        ops.linear_fwd_into(a, wb, None, HID, rb)
        _chain_step(g1, p1, g2, p2, bufa, bufb, rc, rb, noise, mean, std, z, 0, xz, xz)
    with torch.no_grad():
        y = latent.decoder.run(zin)
        f = latent.encoder.run(xin).reshape(B, -1).float()
        us = dict(policy=bench_actor.kernel_us(lambda: po.act(win[0][:, :P]), n=50),
                  prior_step=bench_actor.kernel_us(prior, n=50),
                  decoder=bench_actor.kernel_us(lambda: latent.decoder.run(zin), n=20),
                  hand_off=bench_actor.kernel_us(lambda: ops.decoded_to_frames(y, 3, True, x=xin), n=100),
                  hand_off_u8=bench_actor.kernel_us(lambda: ops.decoded_to_frames(y, 3, True, x=xin, u8_out=u8), n=100),
                  encoder=bench_actor.kernel_us(lambda: latent.encoder.run(xin), n=20),
                  push=bench_actor.kernel_us(lambda: ops.feature_action_push(win[0], win[1], S, F, A, f, a), n=100))
    es = 4 if dt == torch.float32 else 2
    px = B * 10000
    return us, px * 2 * chunk_elems(dt) * es, px * (2 * chunk_elems(dt) * es + 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--batches", default="32,256")
    ap.add_argument("--widths", default="256,1024")
    ap.add_argument("--dtypes", default="fp32,bf16")
    a = ap.parse_args()
    H = a.horizon
    t = lambda fn, iters=a.iters: timed(fn, iters, a.warmup, a.repeats)  # noqa: E731
    out(bench="imagine_feature_action", device=torch.cuda.get_device_name(0), S=S, A=A, H=H, iters=a.iters, repeats=a.repeats)
    g = torch.Generator().manual_seed(0)
    widths = [int(v) for v in a.widths.split(",")]
    latents = {}
    for name in a.dtypes.split(","):
        torch.manual_seed(0)
        latent = latents[name] = LatentModel((3, 100, 100), (A,), image_size=100, dtype=torch.bfloat16 if name == "bf16" else torch.float32)
        for B in [int(v) for v in a.batches.split(",")]:
            z0, noise = torch.randn(B, Z, generator=g).cuda(), torch.randn(B, H, Z, generator=g).cuda()
            window = (torch.randn(B, P, generator=g) * 0.1).cuda()
            for W in widths:
                po = TanhGaussianPolicy(hidden_sizes=[W, W], obs_dim=P, action_dim=A, init_w=0.05)
                new = lambda: latent.imagine_feature_action(po, z0, window, H, noise)  # noqa: E731
                old = lambda: yardstick(latent, po, z0, window, noise, H)  # noqa: E731
                a0, b0 = new()[0][:, 0], old()[:, 0]
                m_new, m_old = t(new), t(old)
                out(bench="rollout", dtype=name, B=B, W=W, ms=m_new[0], ms_min_max=m_new[1:], yardstick_ms=m_old[0],
                    yardstick_ms_min_max=m_old[1:], speedup=round(m_old[0] / m_new[0], 3), first_action_equal=bool(torch.equal(a0, b0)))
                us, bytes_x, bytes_both = step_pieces(latent, po, B, g)
                out(bench="step_pieces_us", dtype=name, B=B, W=W, **{k: round(v, 2) for k, v in us.items()},
                    sum_us=round(sum(v for k, v in us.items() if k != "hand_off_u8"), 2))
                if W == widths[0]:
                    out(bench="hand_off_launch_alone", dtype=name, B=B, pixels=B * 10000, us=round(us["hand_off"], 2),
                        gb_per_s=round(bytes_x / us["hand_off"] / 1e3, 1), share_of_hbm_peak=round(bytes_x / (us["hand_off"] * 1e-6) / HBM_PEAK, 4),
                        with_u8_us=round(us["hand_off_u8"], 2), with_u8_gb_per_s=round(bytes_both / us["hand_off_u8"] / 1e3, 1))

    # (d) imagined_returns end to end, a latent_z and a feature_action policy of equal width
    B, W = 256, widths[0]
    r = np.random.RandomState(0)
    frames = torch.from_numpy(np.frombuffer(r.bytes(B * (CONTEXT + 1) * 30000), dtype=np.uint8).reshape(B, CONTEXT + 1, 100, 100, 3).copy()).cuda()
    acts = (torch.rand(B, CONTEXT, A, generator=g) * 2 - 1).cuda()
    for name, latent in latents.items():
        for kind, obs_dim in (("latent_z", Z), ("feature_action", P)):
            po = TanhGaussianPolicy(hidden_sizes=[W, W], obs_dim=obs_dim, action_dim=A, init_w=0.05)
            ms = t(lambda: imagined_returns(latent, po, frames, acts, H, context=CONTEXT), max(a.iters // 4, 2))
            out(bench="imagined_returns", dtype=name, policy=kind, B=B, W=W, ms=ms[0], ms_min_max=ms[1:])


if __name__ == "__main__":
    main()
