"""Generates tests/golden/slac_imagine_golden_v1.npz by RUNNING THE REAL REFERENCE's modules: `model.z1_prior`, `model.z2_prior` and
`model.reward` of a `rlkit/torch/slac/network/latent.py` `LatentModel` loaded with the seeded weights of tests/slac_latent_ref.py,
`MakeDeterministic(TanhGaussianPolicy)` (`rlkit/torch/sac/policies`, hidden [256, 256]) and two `Qfunction`s
(`examples/iql/custom_networks.py`) loaded with the seeded weights of tests/slac_imagine_ref.py, in fp64 and in fp32.  The reference
has no loop in which the policy acts inside the latent model (SPEC.md N3j); that loop is written here.  Data only: seeds, dims,
weight checksums (the weights themselves are functions of the seeds), the inputs z0 and eps, and per rollout (sampled, mean) the fp64
actions, z1_mean, z1_std, z, the reward head's mean and std, returns, bootstrap and value, each with `ref32_err`: the deviation of the
reference's own fp32 run from its fp64 run in R.rel_max's measure -- PER STEP [H] for the per-step quantities, one number for
returns, bootstrap and value (the tests' tolerance is a multiple of it).  Asserts that the recorded |a| spans [0.1, 0.9] and that
ref32_err of z at the last step is <= 1e-4 (the closed loop does not amplify rounding into noise).
Run:  python tests/golden/make_golden_slac_imagine.py REFERENCE_ROOT"""
import os
import sys
import types

os.environ["PYTORCH_JIT"] = "0"
import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))


def run(mods, dtype, sample):
    import slac_imagine_ref as I
    import slac_latent_ref as R
    LatentModel, TanhGaussianPolicy, MakeDeterministic, Qfunction = mods
    model = LatentModel((3, 100, 100), (I.A,), image_size=100)
    model.load_state_dict(R.full_state_dict(R.make_params(I.A)), strict=True)
    model.to(dtype)
    policy = TanhGaussianPolicy(hidden_sizes=[I.W, I.W], obs_dim=I.Z, action_dim=I.A)
    policy.load_state_dict(I.make_policy_params(), strict=True)
    agent = MakeDeterministic(policy.to(dtype))
    qfs = []
    for i in range(2):
        q = Qfunction(hidden_sizes=[I.W, I.W], output_size=1, input_size=I.Z + I.A)
        q.load_state_dict(I.make_q_params(i), strict=True)
        qfs.append(q.to(dtype))
    z0, noise = [t.to(dtype) for t in I.make_inputs()]
    if not sample:
        noise = torch.zeros_like(noise)
    with torch.no_grad():
        z, acts, ms, ss, zs = z0, [], [], [], []
        for k in range(I.H):
            a = agent(z).sample()
            z2 = z[:, I.Z1:]
            m1, s1 = model.z1_prior(torch.cat([z2, a], dim=1))
            z1 = m1 + noise[:, k, :I.Z1] * s1
            m2, s2 = model.z2_prior(torch.cat([z1, z2, a], dim=1))
            z = torch.cat([z1, m2 + noise[:, k, I.Z1:] * s2], dim=1)
            acts.append(a); ms.append(m1); ss.append(s1); zs.append(z)
        acts, zz = torch.stack(acts, 1), torch.stack(zs, 1)
        x = torch.cat([torch.cat([z0[:, None], zz[:, :-1]], dim=1), acts, zz], dim=-1)
        rm, rs = model.reward(x.view(I.B * I.H, -1))
        rm, rs = rm.view(I.B, I.H), rs.view(I.B, I.H)
        ret = (rm * I.DISCOUNT ** torch.arange(I.H, dtype=dtype)).sum(dim=1)
        zH = zz[:, -1]
        aH = agent(zH).sample()
        boot = torch.minimum(qfs[0](zH, aH)[:, 0], qfs[1](zH, aH)[:, 0])
        val = ret + I.DISCOUNT ** I.H * boot
    return dict(zip(I.QUANTITIES, (acts, torch.stack(ms, 1), torch.stack(ss, 1), zz, rm, rs, ret, boot, val)))


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = sys.argv[1]
    for name in ("torchvision", "torchvision.models", "gtimer"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    sys.modules["torchvision.models"].resnet18 = None
    sys.path.insert(0, ref)
    sys.path.insert(0, os.path.join(ref, "examples", "iql"))
    from rlkit.torch.slac.network.latent import LatentModel  # (the real reference)
    from rlkit.torch.sac.policies import MakeDeterministic, TanhGaussianPolicy
    from custom_networks import Qfunction
    import slac_imagine_ref as I
    import slac_latent_ref as R
    import slac_predict_ref as P
    torch.set_num_threads(8)
    mods = (LatentModel, TanhGaussianPolicy, MakeDeterministic, Qfunction)
    z0, noise = I.make_inputs()
    out = dict(seeds=np.array([R.SEEDS["heads"], P.SEEDS["z0"], P.SEEDS["noise"], I.SEEDS["policy"], I.SEEDS["qf"]]),
               dims=np.array([I.B, I.H, I.A, I.W]), discount=np.float64(I.DISCOUNT), z0=z0.numpy(), noise=noise.numpy(),
               checksum=np.float64(R.checksum(R.make_params(I.A))), policy_checksum=np.float64(R.checksum(I.make_policy_params())),
               qf_checksum=np.array([R.checksum(I.make_q_params(i)) for i in range(2)]))
    worst = 0.0
    for name, sample in zip(I.ROLLOUTS, (True, False)):
        r64, r32 = run(mods, torch.float64, sample), run(mods, torch.float32, sample)
        for k in I.QUANTITIES:
            out["%s.%s" % (name, k)] = r64[k].numpy()
            e = I.step_err(r32[k], r64[k]).numpy() if k in I.STEPWISE else np.float64(R.rel_max(r32[k], r64[k]))
            out["%s.%s.ref32_err" % (name, k)] = e
            worst = max(worst, float(np.max(e)))
            print("%-8s %-12s ref32_err max %.3e  last %.3e" % (name, k, np.max(e), np.ravel(e)[-1]))
        a = np.abs(out[name + ".actions"])
        print("%-8s |a| min %.4f max %.4f" % (name, a.min(), a.max()))
        assert a.min() <= 0.1 and a.max() >= 0.9, "(a) the recorded |a| must span [0.1, 0.9]: change the policy's seed or scale"
        assert out[name + ".z.ref32_err"][-1] <= 1e-4, "(b) ref32_err of z at the last step must stay <= 1e-4: change the seed or scale"
    path = os.path.join(HERE, "slac_imagine_golden_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; worst ref32_err %.3e" % worst)


if __name__ == "__main__":
    main()
