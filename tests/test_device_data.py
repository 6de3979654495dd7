"""--device_data, host half (SPEC.md N1d): the index loader hands out the `index` entries of `create_dataloader`'s batches in that
loader's order, and draws from torch's global generator as that loader does; the flag parses; nothing of it runs on a CPU device.
The device half is tests/test_device_data_gpu.py, the kernel tests/test_frame_pair_gather_gpu.py."""
import os

import numpy as np
import pytest
import torch

from s2p_amd.data import DeviceDataset, S2PDataset, create_dataloader, create_index_loader
from s2p_amd.options.train_options import TrainOptions

N, HW, S = 23, 6, 17


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """One episode and two episodes (timeouts after frames 8 and 15) of 23 frames; the frame's number is in its pixels."""
    d = tmp_path_factory.mktemp("device_data")
    r = np.random.RandomState(3)
    arr = dict(image_observations=np.broadcast_to(np.arange(N, dtype=np.uint8).reshape(N, 1, 1, 1), (N, HW, HW, 3)).copy(),
               observations=r.randn(N, S).astype(np.float32))
    timeouts = np.zeros(N, dtype=bool)
    timeouts[[8, 15]] = True
    np.savez(os.path.join(str(d), "one.npz"), **arr)
    np.savez(os.path.join(str(d), "two.npz"), timeouts=timeouts, **arr)
    return {k: os.path.join(str(d), k + ".npz") for k in ("one", "two")}


def _opt(path, *extra):
    return TrainOptions().parse(["--env_type=cheetah", "--dataroot=" + path, "--crop_size", str(HW), "--batchSize", "4", *extra], quiet=True)


def _epochs(make, seed, epochs=2):
    """The index batches of `epochs` epochs under torch.manual_seed(seed), and the global generator's state after each epoch."""
    torch.manual_seed(seed)
    dl = make()
    batches, states = [], []
    for epoch in range(1, epochs + 1):
        if hasattr(dl.sampler, "set_epoch"):
            dl.sampler.set_epoch(epoch)
        for data in dl:
            idx = data["index"] if isinstance(data, dict) else data
            assert idx.dtype == torch.int64 and idx.device.type == "cpu" and idx.dim() == 1
            batches.append(idx.clone())
        states.append(torch.get_rng_state())
    return batches, states


CASES = {
    "shuffled": ("one", (), 0, 1),
    "serial": ("one", ("--serial_batches",), 0, 1),
    "max_dataset_size": ("one", ("--max_dataset_size", "13"), 0, 1),
    "ragged_tail": ("one", ("--batchSize", "5"), 0, 1),                  # 22 pairs: 4 batches of 5, 2 items dropped
    "two_episodes": ("two", (), 0, 1),
    "two_episodes_serial": ("two", ("--serial_batches",), 0, 1),
    "world2_rank0": ("two", (), 0, 2),
    "world2_rank1": ("two", (), 1, 2),
    "world2_rank1_serial": ("two", ("--serial_batches",), 1, 2),
}


@pytest.mark.parametrize("name", list(CASES))
def test_index_stream_and_rng_state_are_the_dataloaders(files, name):
    which, extra, rank, world = CASES[name]
    opt = _opt(files[which], *extra)
    want, want_rng = _epochs(lambda: create_dataloader(opt, rank, world), 77)
    got, got_rng = _epochs(lambda: create_index_loader(S2PDataset(opt).index, opt, rank, world), 77)
    assert len(want) == len(got) and len(want) > 0
    for a, b in zip(want, got):
        assert torch.equal(a, b), name
    for a, b in zip(want_rng, got_rng):
        assert torch.equal(a, b), name
    # the cases do what their names say
    flat = torch.cat(want).tolist()
    if which == "two":
        assert 8 not in flat and 15 not in flat and len(set(flat)) >= 8
    if name == "max_dataset_size":
        assert max(flat) == 12
    if name == "ragged_tail":
        assert len(want) == 8 and all(len(b) == 5 for b in want)
    if name == "shuffled":
        assert flat != sorted(flat) and len(create_index_loader(S2PDataset(opt).index, opt)) == len(create_dataloader(opt))
    if world == 2:
        other, _ = _epochs(lambda: create_index_loader(S2PDataset(opt).index, opt, 1 - rank, world), 77)
        assert not set(flat[:len(flat) // 2]) & set(torch.cat(other).tolist()[:len(flat) // 2])      # the ranks share no item of an epoch


def test_device_data_flag_parses_and_defaults_to_off():
    assert TrainOptions().parse(["--env_type=cheetah"], quiet=True).device_data is False
    assert TrainOptions().parse(["--env_type=cheetah", "--device_data"], quiet=True).device_data is True


def test_device_dataset_refuses_a_cpu_device(files):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceDataset(_opt(files["one"]), torch.device("cpu"))
    from s2p_amd.data import create_device_loader
    with pytest.raises(RuntimeError, match="device_data"):
        create_device_loader(_opt(files["one"]), "cpu")


def test_frame_pair_gather_refuses_bad_arguments_without_a_device():
    """Every documented refusal is made before any launch: none of them needs a device (the addresses are never looked at)."""
    from s2p_amd import _lib
    L = _lib.lib()
    assert "s2p_frame_pair_gather" in _lib.SIGNATURES and len(_lib.SIGNATURES["s2p_frame_pair_gather"]) == 15
    p = 4096

    def call(pool=p, n=10, H=8, W=8, C=3, states=p, S=17, idx=p, B=2, oh=8, ow=8, prev=p, image=p, state=p):
        return L.s2p_frame_pair_gather(pool, n, H, W, C, states, S, idx, B, oh, ow, prev, image, state, None)
    cases = {"negative n_frames": dict(n=-1), "negative H": dict(H=-1), "negative W": dict(W=-1), "negative S": dict(S=-1),
             "negative B": dict(B=-1), "negative out_h": dict(oh=-1), "negative out_w": dict(ow=-1), "C 0": dict(C=0),
             "C negative": dict(C=-3), "null pool": dict(pool=None), "null idx": dict(idx=None), "null prev": dict(prev=None),
             "null states": dict(states=None), "misaligned prev": dict(prev=p + 2), "misaligned image": dict(image=p + 1),
             "misaligned state": dict(state=p + 3), "empty frame": dict(H=0)}
    for name, kw in cases.items():
        rc = call(**kw)
        msg = L.s2p_last_error().decode()
        assert rc != 0 and msg.startswith("s2p_frame_pair_gather:"), (name, rc, msg)
    assert call(B=0, pool=None, idx=None, prev=None, states=None) == 0          # B == 0: a no-op that looks at no pointer
