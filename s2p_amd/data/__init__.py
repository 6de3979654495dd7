"""Data loading for S2P: (previous image, next state, next image) triples.

On-disk schema mirrors the RL side of the reference so the bulk-augmentation caller can reuse it
(`state_transition_rollout.py:62-68,222-243`): `image_observations` uint8 [T,H,W,3] (NHWC),
`observations` fp32 [T,S], optional `next_observations` fp32 [T,S], optional `timeouts` bool [T].
`.npz` always works; `.hdf5` needs h5py (absent in this image -> clear error).
Images are mapped uint8 -> [-1,1] (SPADE convention)."""
import os

import numpy as np
import torch


def load_arrays(path):
    if os.path.isdir(path):
        raise IsADirectoryError(path)
    if path.endswith(".npz"):
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    if path.endswith(".hdf5") or path.endswith(".h5"):
        try:
            import h5py
        except ImportError as e:
            raise RuntimeError("reading %s needs h5py, which is not installed; convert to .npz" % path) from e
        with h5py.File(path, "r") as f:
            return {k: f[k][()] for k in f.keys()}
    raise ValueError("unsupported dataset file: %s" % path)


def resolve_dataset_file(dataroot, env_type):
    """--dataroot may be a file (README.md:59: ./datasets/cheetah.hdf5) or a directory (README.md:33: ./datasets)."""
    if os.path.isfile(dataroot):
        return dataroot
    for ext in (".npz", ".hdf5", ".h5"):
        p = os.path.join(dataroot, env_type + ext)
        if os.path.isfile(p):
            return p
    raise FileNotFoundError("no %s.{npz,hdf5} under %s" % (env_type, dataroot))


def images_to_tensor(u8_nhwc, size=None):
    """uint8 [T,H,W,3] -> fp32 NCHW in [-1,1] (optionally nearest-resized to size x size)."""
    x = torch.from_numpy(np.ascontiguousarray(u8_nhwc)).permute(0, 3, 1, 2).float() / 127.5 - 1.0
    if size is not None and (x.shape[2] != size or x.shape[3] != size):
        x = torch.nn.functional.interpolate(x, size=(size, size), mode="nearest")
    return x.contiguous()


def tensor_to_images(x_nchw):
    """fp32 NCHW in [-1,1] -> uint8 NHWC (the layout the RL consumer reads, rlkit/torch/slac/algo.py:189-190)."""
    y = ((x_nchw.detach().float().cpu().clamp(-1, 1) + 1.0) * 127.5).round().to(torch.uint8)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


class S2PDataset(torch.utils.data.Dataset):
    def __init__(self, opt):
        self.opt = opt
        arr = load_arrays(resolve_dataset_file(opt.dataroot, opt.env_type))
        self.images = arr["image_observations"]
        self.states = arr["observations"].astype(np.float32)
        T = len(self.images)
        if self.states.shape[1] != opt.state_dim:
            raise ValueError("dataset state dim %d != --state_dim %d" % (self.states.shape[1], opt.state_dim))
        timeouts = arr.get("timeouts")
        self.timeouts = None if timeouts is None else np.asarray(timeouts).astype(bool).reshape(-1)
        valid = np.ones(T - 1, dtype=bool)
        if timeouts is not None:
            valid &= ~self.timeouts[:-1]                          # no pair across an episode boundary
        self.index = np.nonzero(valid)[0][: opt.max_dataset_size]
        self.size = opt.crop_size

    def __len__(self):
        return len(self.index)

    def __getitem__(self, i):
        t = int(self.index[i])
        imgs = images_to_tensor(self.images[t:t + 2], self.size)
        return dict(prev_image=imgs[0], state=torch.from_numpy(self.states[t + 1]), image=imgs[1], index=t)

    def sequence(self, start, length):
        """Frames/states [start, start+length] for an autoregressive rollout."""
        if start + length >= len(self.images):
            raise IndexError("sequence [%d,%d] exceeds dataset length %d" % (start, start + length, len(self.images)))
        if self.timeouts is not None and self.timeouts[start:start + length].any():
            # frame t+1 after a timeout at t belongs to the next episode: the rollout would be scored against it
            end = start + int(np.argmax(self.timeouts[start:start + length]))
            raise IndexError("sequence [%d,%d] crosses an episode boundary (timeout at frame %d); use --seq_len <= %d"
                             % (start, start + length, end, end - start))
        imgs = images_to_tensor(self.images[start:start + length + 1], self.size)
        return imgs, torch.from_numpy(self.states[start:start + length + 1])


def _loader(ds, opt, rank, world_size, num_workers):
    """The DataLoader of both input paths: sampler, batching and drop_last are decided here and nowhere else."""
    sampler = None
    if world_size > 1:
        sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=world_size, rank=rank,
                                                                  shuffle=not opt.serial_batches)
    dl = torch.utils.data.DataLoader(ds, batch_size=opt.batchSize, shuffle=(sampler is None and not opt.serial_batches),
                                     sampler=sampler, num_workers=num_workers, drop_last=opt.isTrain)
    return dl


def create_dataloader(opt, rank=0, world_size=1):
    return _loader(S2PDataset(opt), opt, rank, world_size, int(opt.nThreads))


# ---- --device_data: the training set on the device (SPEC.md N1d) ---------------------------------------------------------------
class FrameIndexDataset(torch.utils.data.Dataset):
    """Item i is the frame number S2PDataset's item i starts at, and nothing else: the host half of the device-resident path."""

    def __init__(self, index):
        self.index = index

    def __len__(self):
        return len(self.index)

    def __getitem__(self, i):
        return int(self.index[i])


def create_index_loader(index, opt, rank=0, world_size=1):
    """A DataLoader over the pair index alone, built by the function that builds `create_dataloader`'s (same sampler, batch size
    and drop_last, no workers): its batches are the `index` entries of that loader's batches, in that order, and it draws from
    torch's global generator exactly as that loader does with --nThreads 0."""
    return _loader(FrameIndexDataset(index), opt, rank, world_size, 0)


class DeviceDataset:
    """The dataset of `S2PDataset(opt)` held once on a HIP device: `pool` uint8 [T,H,W,C] and `states` fp32 [T,S] as stored.
    `gather` turns frame numbers into the batch tensors `S2PDataset.__getitem__` + the default collate give, bit for bit, with one
    launch (`ops.frame_pair_gather`).  `index`, `timeouts`, --max_dataset_size and the state_dim check are S2PDataset's."""

    def __init__(self, opt, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("--device_data keeps the dataset on a HIP device; %s is none (no CPU fallback)" % device)
        host = S2PDataset(opt)
        if host.images.dtype != np.uint8 or host.images.ndim != 4:
            raise TypeError("--device_data needs image_observations as uint8 [T,H,W,C], got %s %s" % (host.images.dtype, host.images.shape))
        self.index, self.size, self.device = host.index, host.size, device
        self.n_frames = len(host.images)
        try:
            self.pool = torch.from_numpy(np.ascontiguousarray(host.images)).to(device)
            self.states = torch.from_numpy(np.ascontiguousarray(host.states)).to(device)
        except torch.OutOfMemoryError as e:
            raise RuntimeError("--device_data: the frame pool of %.2f GB (%d frames of %d bytes) plus %.1f MB of states does not fit on %s; "
                               "train without --device_data" % (host.images.nbytes / 1e9, self.n_frames, host.images[0].nbytes,
                                                                host.states.nbytes / 1e6, device)) from e

    def out_size(self):
        """(h, w) of a batch: --crop_size square, as `S2PDataset.__getitem__` resizes."""
        return (self.size, self.size)

    def gather(self, idx, out=None):
        """Frame numbers `idx` (host int64, [B]) -> dict(prev_image, state, image), device fp32.  With `out` (such a dict of
        caller-owned contiguous buffers, as --hip_graph keeps) the batch is written there and each buffer's version counter is
        bumped, so whatever is cached on (id, _version, data_ptr) of a buffer sees a new batch.  IndexError, before anything is
        launched, if a pair (t, t + 1) does not lie in the dataset."""
        idx = torch.as_tensor(idx, dtype=torch.int64).reshape(-1)
        if idx.is_cuda:
            raise TypeError("frame numbers are given on the host (they are range-checked there)")
        B = idx.numel()
        if B and (int(idx.min()) < 0 or int(idx.max()) + 1 >= self.n_frames):
            raise IndexError("frame pairs (t, t+1) must lie in [0, %d): got t in [%d, %d]" % (self.n_frames, int(idx.min()), int(idx.max())))
        from .. import ops
        C, (h, w) = self.pool.shape[3], self.out_size()
        if out is None:
            f = dict(dtype=torch.float32, device=self.device)
            out = dict(prev_image=torch.empty((B, C, h, w), **f), state=torch.empty((B, self.states.shape[1]), **f),
                       image=torch.empty((B, C, h, w), **f))
            reused = ()
        else:
            reused = ("prev_image", "state", "image")
        ops.frame_pair_gather(self.pool, self.states, idx.to(self.device), (h, w), out["prev_image"], out["image"], out["state"])
        for k in reused:
            torch.autograd.graph.increment_version(out[k])
        return out


class DeviceLoader:
    """Iterable over device batches in the DataLoader's order: dicts prev_image, state, image (device fp32, fresh tensors every
    batch) and index (CPU int64, as collate gives it).  `.sampler` is the index loader's, so `set_epoch` works as on a DataLoader.
    `batches()` yields the index batches alone, for a caller that gathers into buffers of its own."""

    def __init__(self, dataset, index_loader):
        self.dataset, self.index_loader = dataset, index_loader
        self.sampler = index_loader.sampler

    def __len__(self):
        return len(self.index_loader)

    def batches(self):
        return iter(self.index_loader)

    def __iter__(self):
        for idx in self.index_loader:
            batch = self.dataset.gather(idx)      # (the previous batch is still bound while this one is allocated: no address twice in a row)
            batch["index"] = idx
            yield batch


def create_device_loader(opt, device, rank=0, world_size=1):
    """--device_data: what `create_dataloader` returns, with the frames decoded on the device.  Every rank holds the whole pool."""
    ds = DeviceDataset(opt, device)
    return DeviceLoader(ds, create_index_loader(ds.index, opt, rank, world_size))
