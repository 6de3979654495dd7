"""Generates tests/golden/slac_predict_golden_v1.npz by RUNNING THE REAL REFERENCE's modules (`rlkit/torch/slac/network/latent.py`:
`model.z1_prior`, `model.z2_prior`, `model.reward`, `model.decoder` of a `LatentModel` loaded with the seeded weights of
tests/slac_latent_ref.py) in fp64 and in fp32 on the seeded inputs of tests/slac_predict_ref.py.  The reference has the two prior
heads but no loop that feeds them their own samples (SPEC.md N3i); that loop is written here.  Data only: seeds, dims, a weight
checksum, and per rollout (sampled, mean) the fp64 z1_mean, z1_std, z, the reward head's mean and std, a compact image of every
decoded frame (sum, L2 norm, the strided 256-sample of R.sample), and `ref32_err`: the deviation of the reference's own fp32 run
from its fp64 run in R.rel_max's measure (the tests' tolerance is a multiple of it).
Run:  python tests/golden/make_golden_slac_predict.py REFERENCE_ROOT"""
import os
import sys

os.environ["PYTORCH_JIT"] = "0"
import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))


def run(LatentModel, dtype, sample):
    import slac_latent_ref as R
    import slac_predict_ref as P
    model = LatentModel((3, 100, 100), (P.A,), image_size=100)
    model.load_state_dict(R.full_state_dict(R.make_params(P.A)), strict=True)
    model.to(dtype)
    z0, actions, noise = [t.to(dtype) for t in P.make_inputs()]
    if not sample:
        noise = torch.zeros_like(noise)
    with torch.no_grad():
        z2, ms, ss, zs = z0[:, P.Z1:], [], [], []
        for k in range(P.H):
            m1, s1 = model.z1_prior(torch.cat([z2, actions[:, k]], dim=1))
            z1 = m1 + noise[:, k, :P.Z1] * s1
            m2, s2 = model.z2_prior(torch.cat([z1, z2, actions[:, k]], dim=1))
            z2 = m2 + noise[:, k, P.Z1:] * s2
            ms.append(m1); ss.append(s1); zs.append(torch.cat([z1, z2], dim=1))
        z = torch.stack(zs, 1)
        x = torch.cat([torch.cat([z0[:, None], z[:, :-1]], dim=1), actions, z], dim=-1)
        rm, rs = model.reward(x.view(P.B * P.H, -1))
        img, _ = model.decoder(z)
    out = (torch.stack(ms, 1), torch.stack(ss, 1), z, rm.view(P.B, P.H), rs.view(P.B, P.H)) + P.frame_measures(img)
    return dict(zip(P.QUANTITIES, out))


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from rlkit.torch.slac.network.latent import LatentModel  # (the real reference)
    import slac_latent_ref as R
    import slac_predict_ref as P
    torch.set_num_threads(8)
    out = dict(seeds=np.array([R.SEEDS["heads"], R.SEEDS["dec"]] + [P.SEEDS[k] for k in ("z0", "actions", "noise")]),
               dims=np.array([P.B, P.H, P.A]), checksum=np.float64(R.checksum(R.make_params(P.A))))
    worst = 0.0
    for name, sample in zip(P.ROLLOUTS, (True, False)):
        r64, r32 = run(LatentModel, torch.float64, sample), run(LatentModel, torch.float32, sample)
        for k in P.QUANTITIES:
            out["%s.%s" % (name, k)] = r64[k].numpy()
            e = out["%s.%s.ref32_err" % (name, k)] = np.float64(R.rel_max(r32[k], r64[k]))
            worst = max(worst, float(e))
            print("%-8s %-12s ref32_err %.3e" % (name, k, e))
    path = os.path.join(HERE, "slac_predict_golden_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; worst ref32_err %.3e" % worst)


if __name__ == "__main__":
    main()
