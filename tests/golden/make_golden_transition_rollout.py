"""Generates tests/golden/transition_rollout_golden_v1.npz by running tests/transition_rollout_ref.py (the restatement of
state_transition_rollout.py:105-229; that script itself needs gym / dmc2gym / h5py and cannot be imported) with the REAL reference
module `/root/reference/gaussian_ensemble.py` (importable in the build container only) on the CPU.  The model is built from the
`sd.*` arrays of ensemble_golden_v1.npz (E 7, hidden 64, 17 + 6 inputs), so this fixture holds no weights: data only -- the seeded
real dataset (`in.*`), the normalisation (`cfg.*`, computed as train_dynamics.py does), the action bounds and the seed, and the
reference's generated dataset (`out.*`) with the member indices it drew (`ensemble_idx`).
Run:  python tests/golden/make_golden_transition_rollout.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")
from gaussian_ensemble import EnsembleTransition  # noqa: E402  (the real reference)

import transition_rollout_ref as R  # noqa: E402
from train_dynamics import normalisation  # noqa: E402


def main():
    g = np.load(os.path.join(HERE, "ensemble_golden_v1.npz"))
    model = EnsembleTransition(R.OBS_DIM, R.ACT_DIM, 64, 3, ensemble_size=R.N_MEMBERS)
    missing = model.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd.")}, strict=False)
    assert all("saved" in k for k in missing.missing_keys) and not missing.unexpected_keys

    def forward(x):
        dist = model(x)
        return dist.mean, dist.stddev

    data = R.make_dataset()
    cfg = normalisation(data)
    assert all(cfg[k].dtype == np.float32 for k in ("obs_mean", "obs_std", "next_obs_mean", "next_obs_std"))
    members = []
    out = R.rollout(data, cfg, forward, R.ACT_LOW, R.ACT_HIGH, R.SEED, members_out=members)
    arrays = {"in." + k: v for k, v in data.items()}
    arrays.update({"cfg." + k: np.asarray(v) for k, v in cfg.items()})
    arrays.update({"out." + k: v for k, v in out.items()})
    arrays.update(act_low=R.ACT_LOW, act_high=R.ACT_HIGH, seed=np.int64(R.SEED),
                  ensemble_idx=np.concatenate(members).astype(np.int64))
    path = os.path.join(HERE, "transition_rollout_golden_v1.npz")
    np.savez_compressed(path, **arrays)
    for k, v in out.items():
        print(k, v.dtype, v.shape)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
