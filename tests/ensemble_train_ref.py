"""Plain-torch, float64-capable restatement of SPEC.md N2b (ensemble dynamics training) -- TEST INFRASTRUCTURE ONLY.

Pinned half (gaussian_ensemble.py:13-19, 37-48, 83-96): the grouped linear chain for 2-D and 3-D input, soft_clamp, the 'local'
residual and the elementwise Gaussian NLL; tests/test_ensemble_train.py checks it against the real module's autograd results in
tests/golden/ensemble_train_golden_v1.npz.  Unpinned half (the lineage's trainer): the loss, the per-member diagnostics, the
seeded synthetic system and the Adam trajectory the fixture stores."""
import math

import torch
import torch.nn.functional as F

LIVE = ("weight", "bias")


def layer_names(n_hidden):
    return [f"backbones.{i}" for i in range(n_hidden)] + ["output_layer"]


def live_names(n_hidden):
    return ["max_logstd", "min_logstd"] + [f"{n}.{k}" for n in layer_names(n_hidden) for k in LIVE]


def state_dict_names(n_hidden):
    return ["max_logstd", "min_logstd"] + [f"{n}.{k}" for n in layer_names(n_hidden)
                                           for k in ("weight", "bias", "saved_weight", "saved_bias")]


def make_params(seed, E, n_in, hidden, n_hidden, D, rand_bias=True, rand_bounds=True):
    """Seeded parameters in the reference layout (weight [E,in,out], bias [E,1,out]), fp32."""
    g = torch.Generator().manual_seed(seed)
    p = {}
    dims = [(n_in if i == 0 else hidden, hidden) for i in range(n_hidden)] + [(hidden, 2 * D)]
    p["max_logstd"] = torch.rand(D, generator=g) * 1.5 - 0.5 if rand_bounds else torch.ones(D)
    p["min_logstd"] = -torch.rand(D, generator=g) * 3 - 2 if rand_bounds else -5 * torch.ones(D)
    for name, (a, b) in zip(layer_names(n_hidden), dims):
        p[name + ".weight"] = torch.randn(E, a, b, generator=g) / (2 * a ** 0.5)
        p[name + ".bias"] = torch.randn(E, 1, b, generator=g) * 0.1 if rand_bias else torch.zeros(E, 1, b)
    return p


def forward(p, x, select=None):
    """-> (mu, logstd) [G,B,D] over the selected members; x [B,in] or [G,B,in]."""
    n_hidden = len([k for k in p if k.startswith("backbones.") and k.endswith(".weight") and "saved" not in k])
    sel = list(range(p["output_layer.weight"].shape[0])) if select is None else list(select)
    h = x
    for name in layer_names(n_hidden):
        w, b = p[name + ".weight"][sel], p[name + ".bias"][sel]
        h = (torch.einsum("ij,bjk->bik", h, w) if h.dim() == 2 else torch.einsum("bij,bjk->bik", h, w)) + b
        if name != "output_layer":
            h = h * torch.sigmoid(h)
    mu, ls = torch.chunk(h, 2, dim=-1)
    ls = p["max_logstd"] - F.softplus(p["max_logstd"] - ls)
    ls = p["min_logstd"] + F.softplus(ls - p["min_logstd"])
    obs_dim = mu.shape[-1] - 1
    mu = torch.cat([mu[..., :obs_dim] + x[..., :obs_dim], mu[..., obs_dim:]], dim=-1)
    return mu, ls


def loss_terms(p, x, y, select=None):
    """-> (loss, nll_per_member [G], mse_per_member [G])"""
    mu, ls = forward(p, x, select)
    nll = 0.5 * ((y - mu) / torch.exp(ls)) ** 2 + ls + 0.5 * math.log(2 * math.pi)
    loss = nll.mean() + 0.01 * p["max_logstd"].mean() - 0.01 * p["min_logstd"].mean()
    return loss, nll.mean((1, 2)), ((mu - y) ** 2).mean((1, 2))


def loss_and_grad(p32, x, y, select=None, dtype=torch.float64):
    """Runs loss_terms in `dtype` under autograd.  -> (loss, nll, mse, grads: name -> tensor), all in `dtype`."""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in p32.items() if "saved" not in k}
    loss, nll, mse = loss_terms(p, x.to(dtype), y.to(dtype), select)
    loss.backward()
    return loss.detach(), nll.detach(), mse.detach(), {k: v.grad for k, v in p.items()}


def rel_max(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


# ---- the seeded synthetic linear-Gaussian system and the Adam trajectory of the fixture ---------------------------------------------
SYS = dict(obs=5, act=2, hidden=32, n_hidden=3, E=7, B=64, steps=30, n_hold=96, seed=11)


def synthetic_system(n, seed, obs, act):
    """s' = s + 0.1 (A s + C a) + 0.02 noise, r = w . s + 0.02 noise; already 'normalised'.  -> (inputs [n,in], targets [n,obs+1])"""
    g = torch.Generator().manual_seed(seed)
    A, C, w = torch.randn(obs, obs, generator=g) * 0.5, torch.randn(obs, act, generator=g), torch.randn(obs, generator=g)
    s, a = torch.randn(n, obs, generator=g), torch.rand(n, act, generator=g) * 2 - 1
    s2 = s + 0.1 * (s @ A.T + a @ C.T) + 0.02 * torch.randn(n, obs, generator=g)
    r = s @ w + 0.02 * torch.randn(n, generator=g)
    return torch.cat([s, a], 1), torch.cat([s2, r[:, None]], 1)


def training_problem():
    """-> (params fp32, batches x [steps,E,B,in], y [steps,E,B,D], holdout x [n,in], y [n,D])"""
    c = SYS
    n_in, D = c["obs"] + c["act"], c["obs"] + 1
    p = make_params(c["seed"], c["E"], n_in, c["hidden"], c["n_hidden"], D, rand_bias=False, rand_bounds=False)
    X, Y = synthetic_system(2048 + c["n_hold"], c["seed"] + 1, c["obs"], c["act"])
    g = torch.Generator().manual_seed(c["seed"] + 2)
    idx = torch.randint(2048, (c["steps"], c["E"], c["B"]), generator=g)
    return p, X[idx], Y[idx], X[2048:], Y[2048:]


def adam_trajectory(p32, xs, ys, dtype, lr=1e-3):
    """torch.optim.Adam (defaults) on loss_terms over the given batches.  -> (losses per step [steps], final params)"""
    p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in p32.items()}
    opt = torch.optim.Adam(list(p.values()), lr=lr)
    losses = []
    for x, y in zip(xs, ys):
        opt.zero_grad()
        loss = loss_terms(p, x.to(dtype), y.to(dtype))[0]
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, {k: v.detach() for k, v in p.items()}


def holdout_mse(p, x, y):
    with torch.no_grad():
        return loss_terms(p, x.to(p["max_logstd"].dtype), y.to(p["max_logstd"].dtype))[2]
