"""N3f measurement: milliseconds per environment step of policy evaluation at num_envs 1, 4 and 16 (Z 288, A 6, H 1024, P 2090, frames
3 x 100 x 100, S 8) against `ReplayEnv`.  Three forms, timed in one process, median of 5 windows of 200 steps with min and max:
  a. actor  -- `SlacActor`: one upload of N frames, one encoder pass over N frames, the push, three skinny layers, one download;
  b. pieces -- what the package had before it: the 8-frame uint8 window rebuilt on the host, `Encoder.forward` over 8 N frames,
               the concatenation on the device and `TanhGaussianPolicy.act`;
  c. torch  -- the reference's form on torch's own device ops: the window uploaded and encoded by torch convs, the policy input
               copied to the host and back, torch linears.
Also each of the three kernels alone (device events over 200 launches), the skinny layers with their GB/s against the 8 TB/s HBM
peak (bytes = weights + bias + input rows + output rows, each once).
    python tests/tools/bench_actor.py [--steps 200] [--runs 5] [--envs 1,4,16]
Prints one JSON line."""
import argparse
import json
import os
import sys
import time
import types
from collections import deque

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("", "oracle", "tests"):
    sys.path.insert(0, os.path.join(R, p))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import slac_oracle as SO  # noqa: E402
from s2p_amd._lib import check, lib, ptr, stream  # noqa: E402
from s2p_amd.actor import ReplayEnv, SlacActor  # noqa: E402
from s2p_amd.offline_rl import TanhGaussianPolicy  # noqa: E402
from s2p_amd.slac import LatentModel  # noqa: E402

A, H, S, FEAT = 6, 1024, 8, 256
P = S * FEAT + (S - 1) * A
HBM_PEAK = 8e12


def windows(fn, steps, runs):
    """`fn()` is one environment step that ends in a host synchronisation -> ms per step over `runs` windows of `steps`."""
    for _ in range(20):
        fn()                                                  # warm-up: allocator, code objects, the dispatcher's choices
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3 / steps)
    return dict(median_ms=round(float(np.median(ts)), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def kernel_us(fn, n=200):
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(5):
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / n)
    return float(np.median(ts))


class Envs:
    """N `ReplayEnv`s over one long synthetic trajectory each, restarted when it ends."""

    def __init__(self, N, T=64):
        r = np.random.RandomState(0)
        self.envs = [ReplayEnv(dict(image_observations=r.randint(0, 256, size=(T, 3, 100, 100)).astype(np.uint8),
                                    rewards=np.zeros(T, dtype=np.float32), terminals=np.zeros(T, dtype=bool))) for _ in range(N)]
        self.frames = np.stack([e.reset() for e in self.envs])

    def step(self, actions):
        for i, e in enumerate(self.envs):
            o, _, done, _ = e.step(actions[i])
            self.frames[i] = e.reset() if done else o
        return self.frames


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--envs", default="1,4,16")
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_actor.py needs a HIP device"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    latent = LatentModel((3, 100, 100), (A,), device="cuda:0")
    algo = types.SimpleNamespace(latent=latent, state_shape=(3, 100, 100), action_shape=(A,), num_sequences=S)
    policy = TanhGaussianPolicy([H, H], P, A)
    psd = {k: v.to(dev) for k, v in policy.state_dict().items()}
    enc_p = {k: v.detach() for k, v in latent.encoder.state_dict().items()}
    out = dict(config=dict(A=A, H=H, S=S, P=P, steps=a.steps, runs=a.runs), envs={})
    for N in [int(n) for n in a.envs.split(",")]:
        # a. the actor
        envs, actor = Envs(N), SlacActor(policy, algo, N)
        actor.reset(envs.frames)

        def step_actor():
            act = actor.act()
            actor.observe(envs.step(act), act)
        res = dict(actor=windows(step_actor, a.steps, a.runs))

        # b. the pieces of the parent commit
        envs_b = Envs(N)
        win = [deque([np.zeros((3, 100, 100), np.uint8)] * (S - 1) + [envs_b.frames[i].copy()], maxlen=S) for i in range(N)]
        acts = [deque([np.zeros(A, np.float32)] * (S - 1), maxlen=S - 1) for _ in range(N)]

        def step_pieces():
            state = np.stack([np.stack(w) for w in win]).transpose(0, 1, 3, 4, 2)          # [N,S,100,100,3]: Encoder.forward's uint8 layout
            with torch.no_grad():
                feat = latent.encoder(torch.from_numpy(np.ascontiguousarray(state)))
                action = torch.from_numpy(np.stack([np.stack(q) for q in acts])).to(dev)
                fa = torch.cat([feat.reshape(N, -1), action.reshape(N, -1)], dim=1)
                act = policy.act(fa).cpu().numpy()
            frames = envs_b.step(act)
            for i in range(N):
                win[i].append(frames[i].copy()); acts[i].append(act[i])
        res["pieces"] = windows(step_pieces, a.steps, a.runs)

        # c. the reference's form on torch's own device ops
        envs_c = Envs(N)
        win_c = [deque([np.zeros((3, 100, 100), np.uint8)] * (S - 1) + [envs_c.frames[i].copy()], maxlen=S) for i in range(N)]
        acts_c = [deque([np.zeros(A, np.float32)] * (S - 1), maxlen=S - 1) for _ in range(N)]

        def step_torch():
            with torch.no_grad():
                state = torch.tensor(np.stack([np.stack(w) for w in win_c]), dtype=torch.uint8, device=dev).float().div_(255.0)
                feat = SO.encoder_forward(enc_p, state).view(N, -1)
                action = torch.tensor(np.stack([np.stack(q) for q in acts_c]).reshape(N, -1), dtype=torch.float, device=dev)
                o = torch.cat([feat, action], dim=1).cpu().numpy()
                h = torch.from_numpy(o).float().to(dev)
                h = F.relu(F.linear(h, psd["fc0.weight"], psd["fc0.bias"]))
                h = F.relu(F.linear(h, psd["fc1.weight"], psd["fc1.bias"]))
                act = torch.tanh(F.linear(h, psd["last_fc.weight"], psd["last_fc.bias"])).cpu().numpy()
            frames = envs_c.step(act)
            for i in range(N):
                win_c[i].append(frames[i].copy()); acts_c[i].append(act[i])
        res["torch"] = windows(step_torch, a.steps, a.runs)
        res["actor_over_pieces"] = round(res["pieces"]["median_ms"] / res["actor"]["median_ms"], 3)
        res["actor_over_torch"] = round(res["torch"]["median_ms"] / res["actor"]["median_ms"], 3)

        # the kernels alone
        ob, L, st = actor.ob, lib(), stream()
        k = {}
        k["u8_chw_to_nhwc01_us"] = round(kernel_us(lambda: check(L.s2p_u8_chw_to_nhwc01(0, ptr(ob._frames), N, 3, 100, 100, ptr(ob._nhwc), 4, st), "u8")), 2)
        feat = torch.randn(N, FEAT, device=dev)
        k["feature_action_push_us"] = round(kernel_us(lambda: check(L.s2p_feature_action_push(
            ptr(ob._buf[0]), ptr(ob._buf[1]), ob.pitch, N, S, FEAT, A, ptr(feat), FEAT, ptr(ob._act), ob._act.shape[1], ptr(ob._code),
            ptr(ob.fill), st), "push")), 2)
        with torch.no_grad():
            k["encoder_us"] = round(kernel_us(lambda: latent.encoder.run(ob._nhwc), 50), 2)
        for li, (groups, G, Nout, act_id) in enumerate(actor._tables[0]):
            kp = policy.packed.off[li][2]
            nbytes = 4 * (Nout * kp + Nout + N * kp + N * Nout)
            for name, entry in (("skinny", L.s2p_mlp_linear_fwd_skinny), ("tiles", L.s2p_mlp_linear_fwd)):
                us = kernel_us(lambda: check(entry(groups, G, Nout, act_id, st), name))
                k["layer%d_%s_us" % (li, name)] = round(us, 2)
                if name == "skinny":
                    k["layer%d_skinny_GBps" % li] = round(nbytes / us * 1e-3, 1)
                    k["layer%d_skinny_hbm_share" % li] = round(nbytes / (us * 1e-6) / HBM_PEAK, 4)
        res["kernels"] = k
        out["envs"][str(N)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
