"""N3c measurement: sampling from the device-resident SLAC replay buffer against the host path of the reference buffer.

Sizes: `random_batch(256)` and `sample_latent(32)` at 100x100x3, S = 8, --rows real + --rows generated rows (default 50 000 each) of
synthetic frames.  The yardstick is this tool's own restatement of `rlkit/torch/slac/buffer.py:127-167`: a Python loop copying each
window's 9 CHW frames into one host array, one host-to-device copy, `.float().div_(255)`.  Reports ms per call (median [min, max] of
REPS repeats of ITERS calls between two synchronisations, after a warm-up), the gather kernel's achieved GB/s against the 8 TB/s HBM
peak DESIGN.md uses, and `prepare_batch` / `update_latent` fed by each path."""
import argparse, os, statistics, sys, time
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("", "tests"): sys.path.insert(0, os.path.join(R, p))
import numpy as np
import torch
from s2p_amd import ops
from s2p_amd.slac_algo import SlacAlgorithm, all_state_windows, sequential_windows

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=50000)
ap.add_argument("--episode", type=int, default=1000)
ap.add_argument("--bf16", action="store_true")
a = ap.parse_args()
S, A, H, W, C = 8, 6, 100, 100, 3
N, EP = a.rows, a.episode
WARM, ITERS, REPS = 3, 10, 5
HBM_PEAK = 8e12
dt = torch.bfloat16 if a.bf16 else torch.float32


def timed(fn, iters=ITERS):
    for _ in range(WARM): fn()
    out = []
    for _ in range(REPS):
        torch.cuda.synchronize(); t = time.perf_counter()
        for _ in range(iters): fn()
        torch.cuda.synchronize(); out.append((time.perf_counter() - t) / iters * 1e3)
    return statistics.median(out), min(out), max(out)


r = np.random.RandomState(0)
def frames(n): return np.frombuffer(r.bytes(n * H * W * C), dtype=np.uint8).reshape(n, H, W, C)
timeouts = np.zeros(N, dtype=bool); timeouts[EP - 1::EP] = True
obs_idx = np.full((N, S + 1), int(1e9), dtype=np.int64)
i = np.arange(N); ok = i % EP >= S
obs_idx[ok] = i[ok, None] - S + np.arange(S + 1)[None, :]
real = dict(actions=r.uniform(-1, 1, (N, A)).astype(np.float32), rewards=r.randn(N).astype(np.float32), timeouts=timeouts,
            image_observations=frames(N), image_observations_tp1=frames(N))
gen = dict(actions=r.uniform(-1, 1, (N, A)).astype(np.float32), rewards=r.randn(N).astype(np.float32), timeouts=timeouts,
           image_observations=real["image_observations"], image_observations_tp1=frames(N), original_actions=real["actions"],
           original_rewards=real["rewards"], slac_observation_indices=obs_idx, slac_action_indices=obs_idx[:, :-1].copy())

t0 = time.perf_counter()
algo = SlacAlgorithm((C, H, W), (A,), 1, "cuda:0", 0, buffer_size=2 * N, num_sequences=S, dtype=dt, frame_capacity=3 * N + S + 1)
algo.load_data_in_buffer(real)
algo.load_data_in_buffer(gen, data_num=N, generated_for_slac=True, data_mix_type="all_state_1step_random_action",
                         uncertainty_penalty_lambda=0.0)
torch.cuda.synchronize()
buf = algo.buffer
print("device:", torch.cuda.get_device_name(0), " %d real + %d generated rows -> %d windows, %d frames (%.2f GB) in the pool; load %.1f s; %s stacks"
      % (N, N, len(buf), buf._head, buf._head * H * W * C / 1e9, time.perf_counter() - t0, str(dt).split(".")[-1]))

# the host path: the reference's per-window lists of CHW frame views, over the same data
parts = [np.transpose(x, (0, 3, 1, 2)) for x in (real["image_observations"], real["image_observations_tp1"], gen["image_observations_tp1"])]
s_real, _ = sequential_windows(real, S)
s_gen, _, _ = all_state_windows(gen, S)
s_gen = np.where(s_gen >= N, s_gen + N, s_gen)                        # [obs | tp1_gen] -> [obs | tp1_real | tp1_gen]
host_table = np.concatenate([s_real, s_gen])
assert len(host_table) == len(buf)


def host_state(idxes):
    state_ = np.empty((len(idxes), S + 1, C, H, W), dtype=np.uint8)
    for k, idx in enumerate(idxes):
        state_[k, ...] = np.array([parts[s // N][s % N] for s in host_table[idx]], dtype=np.uint8)
    return torch.tensor(state_, dtype=torch.uint8, device="cuda:0").float().div_(255.0)


# same windows from both paths (torch's device-side div_ by a scalar multiplies by the reciprocal: the last bit may differ from u8 / 255)
idx = np.random.randint(0, len(buf), size=8)
hs, ds = host_state(idx), buf.random_batch(8, idxes=idx, frames="float")["observations"]
assert torch.equal((hs * 255).round(), (ds * 255).round()) and float((hs - ds).abs().max()) <= 2.0 ** -23, "device and host path differ"

for bs, name in ((256, "random_batch(256)"), (32, "sample_latent(32)")):
    per_frame = H * W * C * 2 + H * W * 16                     # read once, written as uint8 and as one 16-byte chunk per pixel
    moved = bs * (S + 1) * per_frame
    d = timed(lambda: buf.random_batch(bs) if bs == 256 else buf.sample_latent(bs))
    ids = torch.from_numpy(np.random.randint(0, len(buf), size=bs)).cuda()
    k = timed(lambda: ops.window_gather_u8(buf.pool, buf.table, ids, dt), iters=50)
    h = timed(lambda: host_state(np.random.randint(0, len(buf), size=bs)), iters=3)
    print("%-18s device path %.3f ms [%.3f, %.3f] (gather launch alone %.3f ms: %.0f MB, %.0f GB/s = %.0f%% of the HBM peak);  host path %.1f ms [%.1f, %.1f];  x%.0f"
          % (name, d[0], d[1], d[2], k[0], moved / 1e6, moved / k[0] / 1e6, 100 * moved / (k[0] * 1e-3) / HBM_PEAK, h[0], h[1], h[2], h[0] / d[0]))


def dev_batch(bs): return buf.sample_latent(bs)
def host_batch(bs):
    idxes = np.random.randint(0, len(buf), size=bs)
    return host_state(idxes), buf.action_[idxes], buf.reward_[idxes], buf.done_[idxes]


for label, batch in (("device", dev_batch), ("host", host_batch)):
    def prepare():
        s, act, _, _ = batch(256)
        return algo.prepare_batch(s, act)

    def update():
        algo.learning_steps_latent += 1
        s, act, rew, done = batch(32)
        algo.optim_latent.zero_grad()
        sum(algo.latent.calculate_loss(s, act, rew, done)).backward()
        algo.optim_latent.step()

    print("%-6s path: sample(256) + prepare_batch %.2f ms [%.2f, %.2f];  sample(32) + update_latent %.2f ms [%.2f, %.2f]"
          % ((label,) + timed(prepare, iters=3) + timed(update, iters=5)))
