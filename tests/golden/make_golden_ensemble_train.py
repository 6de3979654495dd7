"""Generates tests/golden/ensemble_train_golden_v1.npz by RUNNING THE REAL REFERENCE (`/root/reference/gaussian_ensemble.py`,
importable in the build container only) under autograd.  The fixture holds data only: a small seeded reference model's live
parameters (hidden 32, 3 layers, E 7, obs 17, act 6), inputs and targets, and for three cases -- a per-member 3-D batch, a shared
2-D batch, a 5-member selection -- the float64 loss, per-member nll / mse and every parameter gradient (stored as fp32) of the
real module, each with `ref32_err`, the deviation of the module's own fp32 run from its fp64 run (relative to the fp64 maximum).
The loss / diagnostics on top of the module's distribution are the unpinned half of SPEC.md N2b.  It also stores the final loss of
the fp64 Adam trajectory of tests/ensemble_train_ref.py on its seeded synthetic system, with that restatement's own fp32 deviation.
Run:  python tests/golden/make_golden_ensemble_train.py"""
import copy
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
from gaussian_ensemble import EnsembleTransition  # noqa: E402  (the real reference)
import ensemble_train_ref as R  # noqa: E402

SELECT = [0, 2, 3, 5, 6]


def run(model, x, y, dtype):
    m = copy.deepcopy(model).to(dtype)
    dist = m(x.to(dtype))
    y = y.to(dtype)
    nll = -dist.log_prob(y)
    assert torch.allclose(nll, 0.5 * ((y - dist.mean) / dist.stddev) ** 2 + dist.stddev.log() + 0.5 * math.log(2 * math.pi))
    loss = nll.mean() + 0.01 * m.max_logstd.mean() - 0.01 * m.min_logstd.mean()
    loss.backward()
    out = {"loss": loss.detach(), "nll": nll.mean((1, 2)).detach(), "mse": ((dist.mean - y) ** 2).mean((1, 2)).detach()}
    for n, p in m.named_parameters():
        if "saved" in n:
            assert p.grad is None
        else:
            assert p.grad is not None and float(p.grad.abs().max()) > 0, n      # every live gradient is non-zero
            out["grad." + n] = p.grad.detach()
    return out


def main():
    torch.manual_seed(20261017)
    obs_dim, act_dim, E, B = 17, 6, 7, 37
    model = EnsembleTransition(obs_dim, act_dim, 32, 3, ensemble_size=E)
    with torch.no_grad():       # non-trivial biases / clamps so every term is exercised
        for n, p in model.named_parameters():
            if n.endswith("bias") and "saved" not in n:
                p.copy_(torch.randn_like(p) * 0.1)
        model.max_logstd.copy_(torch.rand(obs_dim + 1) * 1.5 - 0.5)
        model.min_logstd.copy_(-torch.rand(obs_dim + 1) * 3 - 2)
    model.update_save(list(range(E)))            # saved_* = the live parameters: set_select below restores exactly these
    x3 = torch.randn(E, B, obs_dim + act_dim)
    x3[..., obs_dim:] = torch.rand(E, B, act_dim) * 2 - 1
    x3[:, 0] *= 30.0            # drive some logstd values into both soft-clamp regimes
    y3 = x3[..., :obs_dim + 1] * 0.9 + 0.3 * torch.randn(E, B, obs_dim + 1)
    out = {"sd." + k: v.detach().numpy() for k, v in model.state_dict().items() if "saved" not in k}
    out["state_dict_names"] = np.array(list(model.state_dict().keys()))
    out["state_dict_shapes"] = np.array([",".join(map(str, v.shape)) for v in model.state_dict().values()])
    out.update(x3=x3.numpy(), y3=y3.numpy(), select=np.array(SELECT, np.int32))
    cases = {"c3": (model, x3, y3), "c2": (model, x3[1], y3[1])}
    sel_model = copy.deepcopy(model)
    sel_model.set_select(SELECT)
    cases["sel"] = (sel_model, x3[SELECT], y3[SELECT])
    for tag, (m, x, y) in cases.items():
        r64, r32 = run(m, x, y, torch.float64), run(m, x, y, torch.float32)
        for k in r64:
            out[f"{tag}.{k}"] = r64[k].numpy().astype(np.float64 if k in ("loss", "nll", "mse") else np.float32)
            out[f"{tag}.{k}.ref32_err"] = np.float64(R.rel_max(r32[k], r64[k]))
        with torch.no_grad():
            d = copy.deepcopy(m).double()(x.double())
            out[f"{tag}.mean"], out[f"{tag}.std"] = d.mean.numpy().astype(np.float32), d.stddev.numpy().astype(np.float32)
        print(tag, "loss", float(r64["loss"]), "ref32_err", {k: float(out[f"{tag}.{k}.ref32_err"]) for k in r64})
    g = out["sel.grad.backbones.0.weight"]
    assert np.abs(g[[1, 4]]).max() == 0 and np.abs(g[SELECT]).min(axis=(1, 2)).max() > 0     # unselected members: exactly zero
    assert float(out["c3.std"].max()) > 1.0 and float(out["c3.std"].min()) < 0.3                # both soft-clamp regimes occur

    # the Adam trajectory of the restatement on its seeded synthetic system
    p, xs, ys, xh, yh = R.training_problem()
    l64, p64 = R.adam_trajectory(p, xs, ys, torch.float64)
    l32, _ = R.adam_trajectory(p, xs, ys, torch.float32)
    drift = abs(l32[-1] - l64[-1]) / abs(l64[-1])
    assert drift < 1e-3, drift                   # the fp32 restatement stays on the fp64 trajectory over all the steps
    out["traj.checksum"] = np.float64(float(xs.double().sum() + ys.double().sum() + sum(v.double().sum() for v in p.values())))
    out["traj.losses"] = np.array(l64)
    out["traj.final_loss.ref32_err"] = np.float64(drift)
    out["traj.holdout_mse_initial"] = R.holdout_mse({k: v.double() for k, v in p.items()}, xh, yh).numpy()
    out["traj.holdout_mse_final"] = R.holdout_mse(p64, xh, yh).numpy()
    print("trajectory: loss", l64[0], "->", l64[-1], "fp32 drift", drift, "holdout", out["traj.holdout_mse_initial"], "->",
          out["traj.holdout_mse_final"])
    path = os.path.join(HERE, "ensemble_train_golden_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
