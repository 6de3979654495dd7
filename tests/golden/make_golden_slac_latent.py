"""Generates tests/golden/slac_latent_golden_v1.npz by RUNNING THE REAL REFERENCE LatentModel
(`/root/reference/rlkit/torch/slac/network/latent.py`, importable in the build container only) in fp64 and in fp32 with the
seeded weights, inputs and noise of tests/slac_latent_ref.py.  Data only: seeds, a weight checksum, the fp64 losses, posterior /
prior samples, a compact image of every parameter gradient (sum, L2 norm, a strided sample), and `ref32_err`: the deviation of
the reference's own fp32 run from its fp64 run in the measure the tests use (the tests' tolerance is a multiple of it).
PYTORCH_JIT=0 makes the reference's script methods plain Python, so torch.randn_like can be replaced, for the duration of a call,
by a function that hands out the recorded eps (draw order z1(0), z2(0), z1(1), z2(1), ...).
Run:  python tests/golden/make_golden_slac_latent.py"""
import os
import sys

os.environ["PYTORCH_JIT"] = "0"
import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, "/root/reference")
import slac_latent_ref as R  # noqa: E402
from rlkit.torch.slac.network.latent import LatentModel  # noqa: E402  (the real reference)


def run(dtype):
    p = R.make_params()
    model = LatentModel((3, 100, 100), (R.A,), image_size=100)
    model.load_state_dict(R.full_state_dict(p), strict=True)
    model.to(dtype)
    state_u8, action, reward, done, noise = R.make_inputs()
    state = (state_u8.to(torch.float64) / 255.0).to(dtype)
    action, reward, done, noise = action.to(dtype), reward.to(dtype), done.to(dtype), noise.to(dtype)
    draws = []
    for t in range(R.S + 1):
        draws += [noise[:, t, :R.Z1], noise[:, t, R.Z1:]]
    it = iter(draws)
    orig = torch.randn_like

    def recorded(x, **kw):
        e = next(it)
        assert e.shape == x.shape
        return e

    torch.randn_like = recorded
    try:
        losses = model.calculate_loss(state, action, reward, done)
        assert next(it, None) is None
        sum(losses).backward()
        it = iter(draws)
        with torch.no_grad():
            feat = model.encoder(state)
            pm, ps, z1, z2 = model.sample_posterior(feat, action)
            qm, qs = model.sample_prior(action, z2)
    finally:
        torch.randn_like = orig
    grads = {k: dict(model.named_parameters())[k].grad for k in p}
    mid = dict(post_mean=pm, post_std=ps, z1=z1, z2=z2, prior_mean=qm, prior_std=qs)
    return [float(v) for v in losses], mid, grads, p, model


def main():
    torch.set_num_threads(8)
    l64, m64, g64, p, model = run(torch.float64)
    l32, m32, g32, _, _ = run(torch.float32)
    sd = model.state_dict()
    out = dict(seeds=np.array([R.SEEDS[k] for k in ("enc", "dec", "heads", "inputs", "noise")]), dims=np.array([R.B, R.S, R.A]),
               checksum=np.float64(R.checksum(p)), losses=np.array(l64),
               losses_ref32_err=np.array([abs(a - b) / abs(b) for a, b in zip(l32, l64)]),
               state_dict_keys=np.array(list(sd.keys())), state_dict_shapes=np.array([",".join(map(str, v.shape)) for v in sd.values()]),
               param_names=np.array(list(p.keys())))
    for k, v in m64.items():
        out["mid." + k] = v.numpy()
        out["mid." + k + ".ref32_err"] = np.float64(R.rel_max(m32[k], v))
    for k in p:
        g = g64[k]
        assert g is not None and float(g.abs().sum()) > 0, k               # no gradient of the fixture is zero
        s, l2, samp = float(g.double().sum()), float(g.double().norm()), R.sample(g)
        out[f"grad.{k}.sum"], out[f"grad.{k}.l2"], out[f"grad.{k}.samp"] = np.float64(s), np.float64(l2), samp.numpy()
        out[f"grad.{k}.ref32_err"] = np.array(R.grad_measures(g32[k], s, l2, samp))
    path = os.path.join(HERE, "slac_latent_golden_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; losses", l64, "fp32 dev", out["losses_ref32_err"])
    print("worst grad ref32_err", max(float(out[f"grad.{k}.ref32_err"].max()) for k in p),
          "smallest", min(float(out[f"grad.{k}.ref32_err"].min()) for k in p))


if __name__ == "__main__":
    main()
