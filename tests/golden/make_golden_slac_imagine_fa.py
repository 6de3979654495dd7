"""Generates tests/golden/slac_imagine_fa_golden_v1.npz by RUNNING THE REAL REFERENCE's modules: `model.encoder`, `model.decoder`,
`model.z1_prior` and `model.z2_prior` of a `rlkit/torch/slac/network/latent.py` `LatentModel` loaded with the seeded weights of
tests/slac_latent_ref.py, `create_feature_actions` (`rlkit/torch/slac/utils.py`) for the window's layout and
`MakeDeterministic(TanhGaussianPolicy)` (`rlkit/torch/sac/policies`, hidden [128, 128], obs_dim 2090) loaded with the seeded weights
of tests/slac_imagine_fa_ref.py, in fp64 and in fp32.  The reference has no loop in which a `feature_action` policy acts inside the
latent model (SPEC.md N3o); that loop is written here: act on the window, step the two priors, decode z, clamp the frame to [0,1]
(clamp-only mode, the smooth one), encode it, shift it and the action into the window.  B 2, H 3, context 8: window(0) is
`create_feature_actions`' next_fa of the fp32 encoder's features of the 9 context frames and the 8 context actions, recorded and fed
to both runs.  Data only: seeds, dims, weight checksums, the inputs z0, eps and window, and per rollout (sampled, mean) the fp64
actions, z1_mean, z1_std, z, obs (the H + 1 windows) and the sum, L2 norm and strided sample of every clamped frame, each with
`ref32_err` PER STEP: the deviation of the reference's own fp32 run from its fp64 run in R.rel_max's measure.  Also the uint8 frames
of step 0 of the fp64 run, clamp(round(v * 255), 0, 255), for the quantised mode's one-level check.  Asserts, in clamp-only mode, that
the decoded frames hold values that are clamped and values inside (0, 1), and that the recorded |a| spans [0.1, 0.9].
Run:  python tests/golden/make_golden_slac_imagine_fa.py REFERENCE_ROOT"""
import os
import sys
import types

os.environ["PYTORCH_JIT"] = "0"
import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))


def build(mods, dtype):
    import slac_imagine_fa_ref as F
    import slac_latent_ref as R
    LatentModel, TanhGaussianPolicy, MakeDeterministic, _ = mods
    model = LatentModel((3, 100, 100), (F.A,), image_size=100)
    model.load_state_dict(R.full_state_dict(R.make_params(F.A)), strict=True)
    policy = TanhGaussianPolicy(hidden_sizes=[F.W, F.W], obs_dim=F.OBS, action_dim=F.A)
    policy.load_state_dict(F.make_policy_params(), strict=True)
    return model.to(dtype), MakeDeterministic(policy.to(dtype))


def first_window(mods):
    import slac_imagine_fa_ref as F
    model, _ = build(mods, torch.float32)
    u8, action = F.context_frames()
    with torch.no_grad():
        feat = model.encoder(u8.float() / 255.0)
    return mods[3](feat, action)[1].contiguous()                         # next_fa: the last S features, the S - 1 actions between them


def run(mods, dtype, sample, window):
    import slac_imagine_fa_ref as F
    model, agent = build(mods, dtype)
    z0, noise = [t.to(dtype) for t in F.make_inputs(F.B, F.H)]
    if not sample:
        noise = torch.zeros_like(noise)
    window = window.to(dtype)
    nf = F.S * F.FEAT
    with torch.no_grad():
        z, acts, ms, ss, zs, obs, frames, raws = z0, [], [], [], [], [], [], []
        for k in range(F.H):
            obs.append(window)
            a = agent(window).sample()
            z2 = z[:, F.Z1:]
            m1, s1 = model.z1_prior(torch.cat([z2, a], dim=1))
            z1 = m1 + noise[:, k, :F.Z1] * s1
            m2, s2 = model.z2_prior(torch.cat([z1, z2, a], dim=1))
            z = torch.cat([z1, m2 + noise[:, k, F.Z1:] * s2], dim=1)
            acts.append(a); ms.append(m1); ss.append(s1); zs.append(z)
            raw = model.decoder(z[:, None])[0]                           # [b,1,3,100,100]
            img = raw.clamp(0.0, 1.0)
            f = model.encoder(img)[:, 0]
            window = torch.cat([window[:, F.FEAT:nf], f, window[:, nf + F.A:], a], dim=1)
            frames.append(img[:, 0]); raws.append(raw[:, 0])
        obs.append(window)
    st = lambda xs: torch.stack(xs, 1)
    out = F.measures(dict(actions=st(acts), z1_mean=st(ms), z1_std=st(ss), z=st(zs), obs=st(obs), frames=st(frames)))
    return out, st(raws)


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = sys.argv[1]
    for name in ("torchvision", "torchvision.models", "gtimer"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    sys.modules["torchvision.models"].resnet18 = None
    sys.path.insert(0, ref)
    from rlkit.torch.slac.network.latent import LatentModel  # (the real reference)
    from rlkit.torch.slac.utils import create_feature_actions
    from rlkit.torch.sac.policies import MakeDeterministic, TanhGaussianPolicy
    import slac_imagine_fa_ref as F
    import slac_latent_ref as R
    import slac_predict_ref as P
    torch.set_num_threads(8)
    mods = (LatentModel, TanhGaussianPolicy, MakeDeterministic, create_feature_actions)
    window = first_window(mods)
    assert tuple(window.shape) == (F.B, F.OBS)
    z0, noise = F.make_inputs(F.B, F.H)
    out = dict(seeds=np.array([R.SEEDS["heads"], R.SEEDS["enc"], R.SEEDS["dec"], R.SEEDS["inputs"], P.SEEDS["z0"], P.SEEDS["noise"],
                               F.SEEDS["policy"]]),
               dims=np.array([F.B, F.H, F.A, F.W, F.S, F.CONTEXT]), z0=z0.numpy(), noise=noise.numpy(), window=window.numpy(),
               checksum=np.float64(R.checksum(R.make_params(F.A))), policy_checksum=np.float64(R.checksum(F.make_policy_params())))
    worst = 0.0
    for name, sample in zip(F.ROLLOUTS, (True, False)):
        (r64, raw64), (r32, _) = run(mods, torch.float64, sample, window), run(mods, torch.float32, sample, window)
        for k in F.QUANTITIES:
            out["%s.%s" % (name, k)] = r64[k].numpy()
            e = F.step_err(r32[k], r64[k]).numpy()
            out["%s.%s.ref32_err" % (name, k)] = e
            worst = max(worst, float(np.max(e)))
            print("%-8s %-12s ref32_err max %.3e  last %.3e" % (name, k, np.max(e), np.ravel(e)[-1]))
        q = torch.round(raw64[:, 0] * 255.0).clamp(0.0, 255.0).to(torch.uint8)          # [b,3,100,100]
        out[name + ".frames_u8_step0"] = q.permute(0, 2, 3, 1).contiguous().numpy()      # NHWC, as frames_u8 is
        a = np.abs(out[name + ".actions"])
        clamped, inside = float(((raw64 <= 0) | (raw64 >= 1)).double().mean()), float(((raw64 > 0) & (raw64 < 1)).double().mean())
        out[name + ".frame_shares"] = np.array([clamped, inside])
        print("%-8s |a| min %.4f max %.4f; decoded values clamped %.3f, inside (0,1) %.3f; raw range [%.3f, %.3f]; levels at step 0: %d"
              % (name, a.min(), a.max(), clamped, inside, float(raw64.min()), float(raw64.max()), len(np.unique(q.numpy()))))
        assert clamped >= 0.05 and inside >= 0.05, "(a) the decoded frames must hold clamped values and values inside (0, 1)"
        assert a.min() <= 0.1 and a.max() >= 0.9, "(b) the recorded |a| must span [0.1, 0.9]: change the policy's seed or scale"
    path = os.path.join(HERE, "slac_imagine_fa_golden_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; worst ref32_err %.3e" % worst)


if __name__ == "__main__":
    main()
