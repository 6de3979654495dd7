"""Plain-torch restatement of the closed-loop imagination rollout (SPEC.md N3j) and the seeded inputs of its fixture -- TEST
INFRASTRUCTURE ONLY.  Builds on the latent weights of tests/slac_latent_ref.py and the input pools of tests/slac_predict_ref.py.
Shared by tests/golden/make_golden_slac_imagine.py (which runs the real reference's modules with these weights and inputs) and
tests/test_latent_imagine*.py (which check this restatement, then the HIP model, against the recorded fp64 results)."""
import torch
import torch.nn.functional as F

import slac_latent_ref as R
import slac_predict_ref as P

Z1, Z2, Z = P.Z1, P.Z2, P.Z
B, H, A = 4, 12, 6
W = 256                                                     # hidden width of the fixture's policy and Q functions
DISCOUNT = 0.99
SEEDS = dict(policy=941, qf=942)
ROLLOUTS = ("sampled", "mean")
STEPWISE = ("actions", "z1_mean", "z1_std", "z", "reward_mean", "reward_std")       # [b,h,...]: one ref32_err per step
SCALARS = ("returns", "bootstrap", "value")                                          # [b]: one ref32_err
QUANTITIES = STEPWISE + SCALARS


def make_policy_params(w=W, a=A, seed=None):
    """Seeded weights of TanhGaussianPolicy(hidden [w, w], 288, a) under the reference's keys.  The reference's +-1e-3 `last_fc` would
    leave every action near 0 and the action path untested: it is drawn wide enough that tanh(mean) spreads over (-1, 1)."""
    g = torch.Generator().manual_seed((SEEDS["policy"] if seed is None else seed) + 7 * w + a)
    p, n_in = {}, Z
    for i in range(2):
        p["fc%d.weight" % i] = (torch.rand(w, n_in, generator=g) * 2 - 1) / n_in ** 0.5
        p["fc%d.bias" % i] = torch.randn(w, generator=g) * 0.05
        n_in = w
    p["last_fc.weight"] = (torch.rand(a, w, generator=g) * 2 - 1) * 7.0 / w ** 0.5
    p["last_fc.bias"] = torch.randn(a, generator=g) * 0.05
    p["last_fc_log_std.weight"] = (torch.rand(a, w, generator=g) * 2 - 1) * 1e-3
    p["last_fc_log_std.bias"] = (torch.rand(a, generator=g) * 2 - 1) * 1e-3
    return p


def make_q_params(i, w=W, a=A):
    """Seeded weights of Qfunction number i (hidden [w, w], input 288 + a, output 1) under the reference's keys."""
    g = torch.Generator().manual_seed(SEEDS["qf"] + i)
    p, n_in = {}, Z + a
    for k in range(2):
        p["fc%d.weight" % k] = (torch.rand(w, n_in, generator=g) * 2 - 1) / n_in ** 0.5
        p["fc%d.bias" % k] = torch.randn(w, generator=g) * 0.05
        n_in = w
    p["last_fc.weight"] = (torch.rand(1, w, generator=g) * 2 - 1) / w ** 0.5
    p["last_fc.bias"] = torch.randn(1, generator=g) * 0.05
    return p


def make_inputs(b=B, h=H):
    """z0 [b,288] and eps [b,h,288]: the pools of tests/slac_predict_ref.py (row b and step k do not depend on b and h)."""
    z0, _, noise = P.make_inputs(b, h, A)
    return z0, noise


def mlp(p, x):
    h = F.relu(F.linear(x, p["fc0.weight"], p["fc0.bias"]))
    h = F.relu(F.linear(h, p["fc1.weight"], p["fc1.bias"]))
    return F.linear(h, p["last_fc.weight"], p["last_fc.bias"])


def act(pol, z):
    """tanh(mean): MakeDeterministic(TanhGaussianPolicy)."""
    return torch.tanh(mlp(pol, z))


def imagine(p, pol, z0, noise):
    """-> actions [b,h,A], z1_mean [b,h,32], z1_std [b,h,32], z [b,h,288]; slot k holds a(k) and z(k+1)."""
    z = z0
    acts, ms, ss, zs = [], [], [], []
    for k in range(noise.shape[1]):
        a = act(pol, z)
        z2 = z[:, Z1:]
        m1, s1 = R.gaussian(p, "z1_prior", torch.cat([z2, a], dim=1))
        z1 = m1 + noise[:, k, :Z1] * s1
        m2, s2 = R.gaussian(p, "z2_prior", torch.cat([z1, z2, a], dim=1))
        z = torch.cat([z1, m2 + noise[:, k, Z1:] * s2], dim=1)
        acts.append(a); ms.append(m1); ss.append(s1); zs.append(z)
    return torch.stack(acts, 1), torch.stack(ms, 1), torch.stack(ss, 1), torch.stack(zs, 1)


def discounted(r, discount=DISCOUNT):
    g = discount ** torch.arange(r.shape[1], dtype=r.dtype)
    return (r * g).sum(dim=1)


def q_min(qs, z, a):
    x = torch.cat([z, a], dim=1)
    return torch.minimum(mlp(qs[0], x)[:, 0], mlp(qs[1], x)[:, 0])


def run_all(p, pol, qs, z0, noise, sample=True, discount=DISCOUNT):
    """The nine QUANTITIES of one rollout of the restatement, in the dtype of its arguments."""
    if not sample:
        noise = torch.zeros_like(noise)
    a, m, s, z = imagine(p, pol, z0, noise)
    rm, rs = P.predict_reward(p, z0, z, a)
    ret = discounted(rm, discount)
    zH = z[:, -1]
    boot = q_min(qs, zH, act(pol, zH))
    return dict(zip(QUANTITIES, (a, m, s, z, rm, rs, ret, boot, ret + discount ** noise.shape[1] * boot)))


def step_err(got, ref):
    """R.rel_max per step: [h] for a [b,h,...] quantity."""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double().cpu()
    return torch.tensor([R.rel_max(got[:, k], ref[:, k]) for k in range(ref.shape[1])], dtype=torch.float64)
