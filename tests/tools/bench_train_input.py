"""N1d measurement: how fast train.py's own loop runs when its batches come from the DataLoader (--nThreads 0, --nThreads 8) and
from the device-resident dataset (--device_data), against the same step on one static batch (the ceiling bench.py measures).

Dataset: seeded synthetic frames, --frames (default 50 000) of them, once 84x84 and once 100x100 resized to 84, S 17; bs 64, bf16,
the default losses; eager and --hip_graph.  Every variant is a `train.BatchLoop` over `train.open_loader`, i.e. the code train.py
runs per batch, with its own trainer.  The variants of one configuration alternate in one process after a warm-up; a figure is the
median [min, max] of REPS windows of STEPS steps between two synchronisations.  Also: every loader alone (ms per batch; the host
loaders with and without the upload of the batch), and the gather launch alone with its GB/s against the 8 TB/s HBM peak DESIGN.md
uses.  Only one configuration's loader workers are alive at a time (8 processes)."""
import argparse, gc, json, os, shutil, statistics, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, R)
import numpy as np
import torch
import train
from s2p_amd import ops
from s2p_amd.options.train_options import TrainOptions
from s2p_amd.trainers.pix2pix_trainer import Pix2PixTrainer

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=50000)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--workers", type=int, default=8)
ap.add_argument("--sources", type=int, nargs="+", default=[84, 100], help="stored frame sizes (resized to 84)")
ap.add_argument("--out", type=str, default="", help="also write the figures as JSON here")
a = ap.parse_args()
S, SIZE, HBM_PEAK = 17, 84, 8e12
KEYS = ("prev_image", "state", "image")
assert torch.cuda.is_available(), "this tool measures on a HIP device"
assert a.frames // a.batch >= a.warmup + a.reps * a.steps + 2, "one epoch must cover every window of a variant"


def med(xs):
    return [statistics.median(xs), min(xs), max(xs)]


def fmt(m, unit="ms"):
    return "%.3f %s [%.3f, %.3f]" % (m[0], unit, m[1], m[2])


def window(fn, n):
    torch.cuda.synchronize(); t = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


class Variant:
    """One way of feeding train.py's loop: its options, trainer, loader, BatchLoop and the (one-epoch) batch stream."""

    def __init__(self, name, path, flags):
        self.name = name
        self.opt = TrainOptions().parse(["--env_type=cheetah", "--dataroot=" + path, "--batchSize", str(a.batch), "--gpu_ids=0",
                                         "--crop_size", str(SIZE), "--checkpoints_dir", os.path.join(os.path.dirname(path), "ckpt")] + flags,
                                        quiet=True)
        torch.manual_seed(1234)
        self.trainer = Pix2PixTrainer(self.opt)
        self.dl = train.open_loader(self.opt, self.trainer)
        self.loop = train.BatchLoop(self.opt, self.trainer, self.dl)
        self.stream = enumerate(self.loop.batches())
        self.ms = []

    def step(self):
        self.loop.step(*next(self.stream))

    def close(self):
        self.stream = None                       # (ends the loader's worker processes)
        self.loop = self.dl = self.trainer = None


def loaders_alone(path, src):
    """ms per batch of each loader with nothing trained, and the gather launch on its own."""
    out = {}
    for name, flags in (("nThreads 0", ["--nThreads", "0"]), ("nThreads %d" % a.workers, ["--nThreads", str(a.workers)])):
        opt = TrainOptions().parse(["--env_type=cheetah", "--dataroot=" + path, "--batchSize", str(a.batch), "--crop_size", str(SIZE)] + flags,
                                   quiet=True)
        for upload in (False, True):
            it = iter(train.create_dataloader(opt))
            def one():
                d = next(it)
                if upload:
                    for k in KEYS: d[k].to("cuda:0", non_blocking=True)
            for _ in range(a.warmup): one()
            out[name + (" + upload" if upload else "")] = med([window(one, a.steps) for _ in range(a.reps)])
            del it
    opt = TrainOptions().parse(["--env_type=cheetah", "--dataroot=" + path, "--batchSize", str(a.batch), "--crop_size", str(SIZE),
                                "--device_data"], quiet=True)
    dl = train.create_device_loader(opt, "cuda:0")
    it = iter(dl)
    for _ in range(a.warmup): next(it)
    out["device_data"] = med([window(lambda: next(it), a.steps) for _ in range(a.reps)])
    ds = dl.dataset
    idx = next(dl.batches()).to("cuda:0")
    bufs = ds.gather(idx.cpu())
    launch = lambda: ops.frame_pair_gather(ds.pool, ds.states, idx, ds.out_size(), bufs["prev_image"], bufs["image"], bufs["state"])
    for _ in range(a.warmup): launch()
    k = med([window(launch, 4 * a.steps) for _ in range(a.reps)])
    moved = a.batch * (2 * 3 * src * src + 2 * 3 * SIZE * SIZE * 4 + 2 * S * 4 + 8)       # frames read, two fp32 NCHW frames + state written
    out["gather launch"] = k
    out["gather bytes"] = moved
    out["gather GB/s"] = [moved / (t * 1e-3) / 1e9 for t in (k[0], k[2], k[1])]
    return out


results = {"device": torch.cuda.get_device_name(0), "frames": a.frames, "batch": a.batch, "steps": a.steps, "reps": a.reps, "configs": []}
print("device:", results["device"], " %d frames, bs %d, bf16, %d x %d steps per figure" % (a.frames, a.batch, a.reps, a.steps), flush=True)
tmp = tempfile.mkdtemp(prefix="s2p_train_input_")
try:
    for src in a.sources:
        r = np.random.RandomState(src)
        path = os.path.join(tmp, "cheetah_%d" % src, "cheetah.npz")
        os.makedirs(os.path.dirname(path))
        np.savez(path, image_observations=np.frombuffer(r.bytes(a.frames * src * src * 3), dtype=np.uint8).reshape(a.frames, src, src, 3),
                 observations=r.randn(a.frames, S).astype(np.float32))
        alone = loaders_alone(path, src)
        print("\n%dx%d -> %d, loaders alone (ms per batch of %d):" % (src, src, SIZE, a.batch))
        for k, v in alone.items():
            if isinstance(v, list) and not k.endswith("GB/s"): print("  %-22s %s" % (k, fmt(v)))
        print("  gather launch moves %.2f MB: %.0f GB/s [%.0f, %.0f] = %.0f%% of the HBM peak" % (
            alone["gather bytes"] / 1e6, *alone["gather GB/s"], 100 * alone["gather GB/s"][0] * 1e9 / HBM_PEAK), flush=True)
        for graph in (False, True):
            g = ["--hip_graph"] if graph else []
            vs = [Variant("nThreads 0", path, g + ["--nThreads", "0"]), Variant("nThreads %d" % a.workers, path, g + ["--nThreads", str(a.workers)]),
                  Variant("device_data", path, g + ["--device_data"])]
            for v in vs:
                for _ in range(a.warmup): v.step()
            # the ceiling: the device variant's step on the batch it holds, nothing loaded or gathered
            dv = vs[2]
            if graph:
                ceiling = dv.loop.sg.replay
            else:
                fixed = {k: t.clone() for k, t in dv.dl.dataset.gather(next(dv.dl.batches())).items()}
                ceiling = lambda: dv.loop.step(0, fixed)
            for _ in range(a.warmup): ceiling()
            ceil_ms = []
            for _ in range(a.reps):
                for v in vs: v.ms.append(window(v.step, a.steps))
                ceil_ms.append(window(ceiling, a.steps))
            cfg = {"source": src, "hip_graph": graph, "loaders_alone": alone, "static batch": med(ceil_ms)}
            print("\n%dx%d -> %d, %s: train.py's loop, ms per step and images/s" % (src, src, SIZE, "--hip_graph" if graph else "eager"))
            for name, m in [(v.name, med(v.ms)) for v in vs] + [("static batch", cfg["static batch"])]:
                cfg[name] = m
                print("  %-14s %s  %6.0f images/s [%.0f, %.0f]  x%.3f of the static batch" % (
                    name, fmt(m), a.batch / m[0] * 1e3, a.batch / m[2] * 1e3, a.batch / m[1] * 1e3, m[0] / cfg["static batch"][0]), flush=True)
            results["configs"].append(cfg)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                json.dump(results, open(a.out, "w"), indent=1)
            for v in vs: v.close()
            del vs, dv, ceiling
            gc.collect(); torch.cuda.empty_cache()
finally:
    shutil.rmtree(tmp, ignore_errors=True)
