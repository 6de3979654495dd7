"""--device_data on the device (SPEC.md N1d): the device loader's batches are bit for bit `create_dataloader`'s in its order, the
model's input caches see every new batch, an index out of range is refused before any launch, and train.py trains the same
weights with the flag as without it, eagerly and under --hip_graph."""
import os
import sys

import numpy as np
import pytest
import torch

from s2p_amd.data import DeviceDataset, create_dataloader, create_device_loader
from s2p_amd.options.train_options import TrainOptions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("prev_image", "state", "image")


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    """23 frames of 30x30 in two episodes (the first ends at frame 9)."""
    r = np.random.RandomState(4)
    timeouts = np.zeros(23, dtype=bool)
    timeouts[[9, 22]] = True
    path = os.path.join(str(tmp_path_factory.mktemp("device_data_gpu")), "cheetah.npz")
    np.savez(path, image_observations=r.randint(0, 256, size=(23, 30, 30, 3)).astype(np.uint8),
             observations=r.randn(23, 17).astype(np.float32), timeouts=timeouts)
    return path


def _opt(*args):
    return TrainOptions().parse(["--env_type=cheetah", "--gpu_ids=0", *args], quiet=True)


def _key(t):
    return (id(t), t._version, t.data_ptr())


def _same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _epochs(dl, seed, epochs=2):
    torch.manual_seed(seed)
    out = []
    for epoch in range(1, epochs + 1):
        for data in dl:
            out.append({k: data[k].cpu().clone() for k in KEYS + ("index",)})
    return out, torch.get_rng_state()


@pytest.mark.parametrize("order", ["shuffled", "serial"])
@pytest.mark.parametrize("which", ["shipped", "synthetic"])
def test_loader_batches_are_the_dataloaders_bit_for_bit(hip_device, synthetic, which, order):
    args = ["--dataroot=" + os.path.join(ROOT, "datasets"), "--batchSize", "2"] if which == "shipped" else \
        ["--dataroot=" + synthetic, "--batchSize", "4", "--crop_size", "20", "--max_dataset_size", "15"]
    opt = _opt(*args, *(["--serial_batches"] if order == "serial" else []))
    want, want_rng = _epochs(create_dataloader(opt), 31)
    dl = create_device_loader(opt, hip_device)
    got, got_rng = _epochs(dl, 31)
    assert len(dl) == len(want) // 2 and len(got) == len(want) > 2 and torch.equal(want_rng, got_rng)
    for a, b in zip(want, got):
        assert torch.equal(a["index"], b["index"]) and b["index"].dtype == torch.int64
        for k in KEYS:
            assert _same_bits(a[k], b[k]), (which, order, k)
    if which == "synthetic":
        flat = torch.cat([b["index"] for b in got]).tolist()
        assert 9 not in flat and max(flat) <= 15 and tuple(got[0]["image"].shape) == (4, 3, 20, 20)      # pairs 0..8, 10..15
    if order == "shuffled":
        assert not all(torch.equal(a["index"], b["index"]) for a, b in zip(got[:len(dl)], got[len(dl):]))


def test_every_batch_presents_a_new_cache_key(hip_device, synthetic):
    """Pix2PixModel.preprocess_input and autograd_nodes._dreal_key key on (id, _version, data_ptr) of the input tensors."""
    opt = _opt("--dataroot=" + synthetic, "--batchSize", "4", "--crop_size", "20")
    dl = create_device_loader(opt, hip_device)
    it = iter(dl)
    a = next(it)
    ka = {k: _key(a[k]) for k in KEYS}
    b = next(it)
    for k in KEYS:
        assert a[k].is_cuda and a[k].dtype == torch.float32 and _key(b[k]) != ka[k], k
    del a
    c = next(it)                                # a's memory may be handed out again, b's may not
    for k in KEYS:
        assert _key(c[k]) != _key(b[k]), k
    # reused buffers (--hip_graph): the launch itself bumps nothing, gather does
    ds = dl.dataset
    out = ds.gather(b["index"])
    assert all(_same_bits(out[k], b[k]) for k in KEYS)
    before = {k: _key(out[k]) for k in KEYS}
    again = ds.gather(c["index"], out=out)
    assert again is out
    for k in KEYS:
        assert _same_bits(out[k], c[k]) and _key(out[k]) != before[k] and out[k]._version > before[k][1], k
        assert (id(out[k]), out[k].data_ptr()) == (before[k][0], before[k][2])


def test_index_out_of_range_raises_before_any_launch(hip_device, synthetic):
    ds = DeviceDataset(_opt("--dataroot=" + synthetic, "--crop_size", "20"), hip_device)
    out = {k: torch.full(s, 3.25, device=hip_device) for k, s in (("prev_image", (2, 3, 20, 20)), ("image", (2, 3, 20, 20)), ("state", (2, 17)))}
    versions = {k: out[k]._version for k in KEYS}
    for bad in (-1, 22, 23, 2 ** 40):
        with pytest.raises(IndexError):
            ds.gather(torch.tensor([3, bad]), out=out)
        with pytest.raises(IndexError):
            ds.gather([bad])
    torch.cuda.synchronize()
    for k in KEYS:
        assert bool((out[k] == 3.25).all()) and out[k]._version == versions[k], k
    ds.gather([21, 0], out=out)                 # the last pair is in range
    assert float(out["image"].abs().max()) <= 1.0


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "hip_graph"])
def test_train_cli_with_device_data_matches_the_dataloader_run(hip_device, tmp_path, capsys, graph):
    """train.py on the shipped dataset under one seed, with and without --device_data: the same steps are taken and every weight
    agrees within the bound of test_train_cli_graph_replay_matches_eager.  (Whether they are bitwise equal is printed.)"""
    sys.path.insert(0, ROOT)
    import train
    out = {}
    for mode in ("loader", "device"):
        d = os.path.join(str(tmp_path), mode)
        args = ["--env_type=cheetah", "--dataroot=" + os.path.join(ROOT, "datasets"), "--netG=s2p", "--batchSize=2", "--gpu_ids=0",
                "--checkpoints_dir", d, "--save_epoch_freq", "2", "--print_freq", "100", "--no_vgg_loss", "--niter", "2"]
        torch.manual_seed(1234)
        train.main(args + (["--hip_graph"] if graph else []) + (["--device_data", "--nThreads", "3"] if mode == "device" else []))
        out[mode] = torch.load(os.path.join(d, "cheetah_2.pth"), map_location="cpu")
    assert capsys.readouterr().out.count("--nThreads 3 is ignored with --device_data") == 1
    a, b = out["loader"], out["device"]
    assert a["iters_done"] == b["iters_done"] > 0 and int(a["optG"]["step"]) == int(b["optG"]["step"]) == a["iters_done"]
    assert int(a["optD"]["step"]) == int(b["optD"]["step"])
    bitwise = True
    for net in ("netG", "netD"):
        for k in a[net]:
            x, y = a[net][k].float(), b[net][k].float()
            assert float((x - y).norm()) <= 1e-4 * float(x.norm()) + 1e-7, (net, k)
            bitwise = bitwise and torch.equal(x, y)
    with capsys.disabled():
        print("\n[device_data %s] weights bitwise equal to the DataLoader run: %s" % ("hip_graph" if graph else "eager", bitwise))
