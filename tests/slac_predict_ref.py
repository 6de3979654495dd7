"""Plain-torch restatement of the open-loop prior rollout (SPEC.md N3i) and the seeded inputs of its fixture -- TEST
INFRASTRUCTURE ONLY.  Builds on the weights of tests/slac_latent_ref.py.  Shared by tests/golden/make_golden_slac_predict.py (which
runs the real reference's modules with these inputs) and tests/test_latent_predict*.py (which check this restatement, then the HIP
model, against the recorded fp64 results)."""
import torch

import slac_latent_ref as R
import slac_oracle as SO

Z1, Z2, Z = R.Z1, R.Z2, R.Z1 + R.Z2
B, H, A = 4, 12, 6
POOL = 33
SEEDS = dict(z0=931, actions=932, noise=933)
ROLLOUTS = ("sampled", "mean")
QUANTITIES = ("z1_mean", "z1_std", "z", "reward_mean", "reward_std", "frame_sum", "frame_l2", "frame_samp")


def make_inputs(b=B, h=H, a=A):
    """z0 [b,288] ~ N(0,1), actions [b,h,a] ~ U(-1,1), eps [b,h,288] ~ N(0,1), b <= 33, h <= 12: slices of one seeded pool each, so
    row b and step k are the same whatever b and h are (the fixture is the first 4 rows)."""
    assert b <= POOL and h <= H
    z0 = torch.randn(POOL, Z, generator=torch.Generator().manual_seed(SEEDS["z0"]))[:b]
    actions = torch.rand(POOL, H, a, generator=torch.Generator().manual_seed(SEEDS["actions"] + a))[:b, :h] * 2 - 1
    noise = torch.randn(POOL, H, Z, generator=torch.Generator().manual_seed(SEEDS["noise"]))[:b, :h]
    return z0.contiguous(), actions.contiguous(), noise.contiguous()


def predict(p, z0, actions, noise):
    """-> z1_mean [b,h,32], z1_std [b,h,32], z [b,h,288]; step k + 1 in slot k.  z1(0) = z0[:, :32] is not read."""
    z2 = z0[:, Z1:]
    ms, ss, zs = [], [], []
    for k in range(actions.shape[1]):
        m1, s1 = R.gaussian(p, "z1_prior", torch.cat([z2, actions[:, k]], dim=1))
        z1 = m1 + noise[:, k, :Z1] * s1
        m2, s2 = R.gaussian(p, "z2_prior", torch.cat([z1, z2, actions[:, k]], dim=1))
        z2 = m2 + noise[:, k, Z1:] * s2
        ms.append(m1); ss.append(s1); zs.append(torch.cat([z1, z2], dim=1))
    return torch.stack(ms, 1), torch.stack(ss, 1), torch.stack(zs, 1)


def predict_reward(p, z0, z, actions):
    """Reward head on [z(k) | a(k) | z(k+1)], z(0) = z0 -> mean, std [b,h]."""
    prev = torch.cat([z0[:, None], z[:, :-1]], dim=1)
    m, s = R.gaussian(p, "reward", torch.cat([prev, actions, z], dim=-1))
    return m[..., 0], s[..., 0]


def decode(p, z):
    return SO.decoder_forward({k[len("decoder."):]: v for k, v in p.items() if k.startswith("decoder.")}, z)


def frame_measures(img):
    """Per frame of img [b,h,3,100,100]: sum [b,h], L2 norm [b,h] and the strided 256-sample of R.sample [b,h,256], in fp64."""
    f = torch.as_tensor(img).detach().double().cpu()
    b, h = f.shape[:2]
    f = f.reshape(b, h, -1)
    samp = torch.stack([torch.stack([R.sample(f[i, k]) for k in range(h)]) for i in range(b)])
    return f.sum(-1), f.norm(dim=-1), samp


def run_all(p, z0, actions, noise, sample=True):
    """The eight QUANTITIES of one rollout of the restatement, in the dtype of its arguments."""
    if not sample:
        noise = torch.zeros_like(noise)
    m, s, z = predict(p, z0, actions, noise)
    rm, rs = predict_reward(p, z0, z, actions)
    return dict(zip(QUANTITIES, (m, s, z, rm, rs) + frame_measures(decode(p, z))))
