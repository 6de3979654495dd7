"""Generates tests/golden/slac_buffer_golden_v1.npz by RUNNING THE REAL REFERENCE loader and buffer
(`rlkit/torch/slac/algo.py:154-416` SlacAlgorithm.load_data_in_buffer, `rlkit/torch/slac/buffer.py` ReplayBuffer) on the CPU over the
seeded datasets of tests/slac_buffer_ref.py.  Data only: per scenario the window frames (the reference's `state_`), `action_`,
`reward_`, `done_`, `_n`, `_p`, `_real_n`; one `random_batch(4)` under `np.random.seed(3)` for the mixed scenario; and one scenario
driven through `reset_episode` / `append` directly.

The reference loader opens its file with h5py, which is not needed here: a stand-in module named `h5py` is put into sys.modules
whose `File` returns the dict of numpy arrays registered under that name.  The algorithm object is made with `object.__new__` and
given `buffer`, `num_sequences` and `use_seperate_buffer` only, so no 100x100 model is built.
Run:  python tests/golden/make_golden_slac_buffer.py <path of the reference checkout>"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, sys.argv[1])
import slac_buffer_ref as R  # noqa: E402

FILES = {}


class _File(dict):
    def close(self):
        pass


h5py = types.ModuleType("h5py")
h5py.File = lambda name, mode="r": _File(FILES[name])
sys.modules["h5py"] = h5py

from rlkit.torch.slac.algo import SlacAlgorithm  # noqa: E402  (the real reference)
from rlkit.torch.slac.buffer import ReplayBuffer  # noqa: E402


def frames_of(buf):
    return np.stack([np.array(buf.state_[i]._frames, dtype=np.uint8) for i in range(buf._n)])


def record(out, name, buf):
    n = buf._n
    out[name + ".frames"] = frames_of(buf)
    out[name + ".action_"] = buf.action_[:n].numpy().copy()
    out[name + ".reward_"] = buf.reward_[:n].numpy().copy()
    out[name + ".done_"] = buf.done_[:n].numpy().copy()
    out[name + ".counts"] = np.array([buf._n, buf._p, buf._real_n])
    print(name, "_n", buf._n, "_p", buf._p, "_real_n", buf._real_n, "done sum", float(buf.done_[:n].sum()))


def main():
    for k, make in R.DATASETS.items():
        FILES[k] = make()
    out = {}
    for name, size, what in R.SCENARIOS:
        algo = object.__new__(SlacAlgorithm)
        algo.buffer = ReplayBuffer(size, R.S, (R.C, R.H, R.W), (R.A,), "cpu")
        algo.num_sequences, algo.use_seperate_buffer = R.S, False
        for k in what:
            algo.load_data_in_buffer(k, None, None, **R.LOAD_ARGS[k])
        record(out, name, algo.buffer)
        if name == "mixed64":
            np.random.seed(R.BATCH_SEED)
            b = algo.buffer.random_batch(R.BATCH)
            for k, v in b.items():
                out["batch." + k] = v.numpy().copy()
    buf = ReplayBuffer(R.APPEND_BUFFER, R.S, (R.C, R.H, R.W), (R.A,), "cpu")
    R.drive_append(buf)
    record(out, "append", buf)
    path = os.path.join(HERE, "slac_buffer_golden_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
