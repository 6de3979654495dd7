"""Plain-torch restatement of the SLAC latent model (SPEC.md N3b) and the seeded weights / inputs of its fixture -- TEST
INFRASTRUCTURE ONLY.  Shared by tests/golden/make_golden_slac_latent.py (which runs the real reference with these weights)
and tests/test_slac_latent.py (which checks this restatement, then the HIP model, against the recorded fp64 results)."""
import math

import torch
import torch.nn.functional as F

import slac_oracle as SO

Z1, Z2, FEAT, HID = 32, 256, 256, 256
B, S, A = 4, 8, 6
SEEDS = dict(enc=911, dec=912, heads=913, inputs=914, noise=915)
NSAMP = 256


def head_dims(a=A):
    """name -> (input_dim, output_dim) of the six distinct Gaussian heads, in the reference's registration order."""
    return {"z2_prior_init": (Z1, Z2), "z1_prior": (Z2 + a, Z1), "z2_prior": (Z1 + Z2 + a, Z2), "z1_posterior_init": (FEAT, Z1),
            "z1_posterior": (FEAT + Z2 + a, Z1), "reward": (2 * (Z1 + Z2) + a, 1)}


ALIASES = {"z2_posterior_init": "z2_prior_init", "z2_posterior": "z2_prior"}
KEY_ORDER = ["z2_prior_init", "z1_prior", "z2_prior", "z1_posterior_init", "z2_posterior_init", "z1_posterior", "z2_posterior",
             "reward"]


def make_head_params(seed, a=A):
    """Seeded xavier-uniform weights and NON-ZERO biases (the reference's initialiser zeroes them, which would leave every
    bias path untested) for the six distinct heads, keys `<head>.net.{0,2,4}.{weight,bias}`."""
    g = torch.Generator().manual_seed(seed)
    p = {}
    for name, (din, dout) in head_dims(a).items():
        dims = [(din, HID), (HID, HID), (HID, 2 * dout)]
        for i, (ci, co) in zip((0, 2, 4), dims):
            bound = (6.0 / (ci + co)) ** 0.5
            p[f"{name}.net.{i}.weight"] = (torch.rand((co, ci), generator=g) * 2 - 1) * bound
            p[f"{name}.net.{i}.bias"] = torch.randn(co, generator=g) * 0.05
    return p


def make_params(a=A):
    """The 60 distinct parameters (36 of the heads, 24 of the conv stacks)."""
    p = make_head_params(SEEDS["heads"], a)
    p.update({"encoder." + k: v for k, v in SO.make_params(SO.ENCODER_100, SEEDS["enc"]).items()})
    p.update({"decoder." + k: v for k, v in SO.make_params(SO.DECODER_100, SEEDS["dec"]).items()})
    return p


def full_state_dict(p):
    """The reference's 72-key state_dict (aliases included), in its key order."""
    sd = {}
    for name in KEY_ORDER:
        src = ALIASES.get(name, name)
        for i in (0, 2, 4):
            for wb in ("weight", "bias"):
                sd[f"{name}.net.{i}.{wb}"] = p[f"{src}.net.{i}.{wb}"]
    sd.update({k: v for k, v in p.items() if k.startswith(("encoder.", "decoder."))})
    return sd


def checksum(p):
    return float(sum(v.double().abs().sum() for v in p.values()))


def make_inputs(b=B, s=S, a=A):
    """state [b,s+1,3,100,100] in [0,1] on the uint8 grid, action, reward ~ N(0,1), done with some ones, eps [b,s+1,288]."""
    g = torch.Generator().manual_seed(SEEDS["inputs"])
    state_u8 = (torch.rand(b, s + 1, 3, 100, 100, generator=g) * 255).round().to(torch.uint8)
    action = torch.randn(b, s, a, generator=g)
    reward = torch.randn(b, s, 1, generator=g)
    done = (torch.rand(b, s, 1, generator=g) < 0.25).float()
    done[0, 0, 0], done[0, 1, 0] = 1.0, 0.0
    g = torch.Generator().manual_seed(SEEDS["noise"])
    noise = torch.randn(b, s + 1, Z1 + Z2, generator=g)
    return state_u8, action, reward, done, noise


def gaussian(p, name, x):
    h = F.leaky_relu(F.linear(x, p[f"{name}.net.0.weight"], p[f"{name}.net.0.bias"]), 0.2)
    h = F.leaky_relu(F.linear(h, p[f"{name}.net.2.weight"], p[f"{name}.net.2.bias"]), 0.2)
    out = F.linear(h, p[f"{name}.net.4.weight"], p[f"{name}.net.4.bias"])
    mean, raw = torch.chunk(out, 2, dim=-1)
    return mean, F.softplus(raw) + 1e-5


def sample_posterior(p, feat, action, noise):
    m, s = gaussian(p, "z1_posterior_init", feat[:, 0])
    z1 = m + noise[:, 0, :Z1] * s
    m2, s2 = gaussian(p, "z2_prior_init", z1)
    z2 = m2 + noise[:, 0, Z1:] * s2
    ms, ss, z1s, z2s = [m], [s], [z1], [z2]
    for t in range(1, action.shape[1] + 1):
        m, s = gaussian(p, "z1_posterior", torch.cat([feat[:, t], z2, action[:, t - 1]], dim=1))
        z1 = m + noise[:, t, :Z1] * s
        m2, s2 = gaussian(p, "z2_prior", torch.cat([z1, z2, action[:, t - 1]], dim=1))
        z2 = m2 + noise[:, t, Z1:] * s2
        ms.append(m); ss.append(s); z1s.append(z1); z2s.append(z2)
    return torch.stack(ms, 1), torch.stack(ss, 1), torch.stack(z1s, 1), torch.stack(z2s, 1)


def sample_prior(p, action, z2_post):
    m, s = gaussian(p, "z1_prior", torch.cat([z2_post[:, :action.shape[1]], action], dim=-1))
    m0, s0 = torch.zeros_like(m[:, :1]), torch.ones_like(s[:, :1])
    return torch.cat([m0, m], dim=1), torch.cat([s0, s], dim=1)


def kl(pm, ps, qm, qs):
    vr = (ps / qs) ** 2
    return 0.5 * (vr + ((pm - qm) / qs) ** 2 - 1 - vr.log())


def nll(x, mean, std):
    return 0.5 * ((x - mean) / (std + 1e-8)) ** 2 + std.log() + 0.5 * math.log(2 * math.pi)


def calculate_loss(p, state, action, reward, done, noise):
    """-> (loss_kld, loss_image, loss_reward), dict of the intermediate samples."""
    enc = {k[len("encoder."):]: v for k, v in p.items() if k.startswith("encoder.")}
    dec = {k[len("decoder."):]: v for k, v in p.items() if k.startswith("decoder.")}
    feat = SO.encoder_forward(enc, state)
    pm, ps, z1, z2 = sample_posterior(p, feat, action, noise)
    qm, qs = sample_prior(p, action, z2)
    loss_kld = kl(pm, ps, qm, qs).mean(0).sum()
    z = torch.cat([z1, z2], dim=-1)
    img = SO.decoder_forward(dec, z)
    loss_image = nll(state, img, torch.full_like(img, 0.1 ** 0.5)).mean(0).sum()
    rm, rs = gaussian(p, "reward", torch.cat([z[:, :-1], action, z[:, 1:]], dim=-1))
    loss_reward = (nll(reward, rm, rs) * (1 - done)).mean(0).sum()
    mid = dict(post_mean=pm, post_std=ps, z1=z1, z2=z2, prior_mean=qm, prior_std=qs)
    return (loss_kld, loss_image, loss_reward), mid


def sample(g):
    f = torch.as_tensor(g).detach().double().flatten().cpu()
    stride = max(1, f.numel() // NSAMP)
    return f[::stride][:NSAMP]


def grad_measures(g, ref_sum, ref_l2, ref_samp):
    """The three deviations `_check_grads` of tests/test_slac.py bounds, as numbers: L2 norm, sum, strided sample."""
    got = torch.as_tensor(g).detach().double().cpu()
    ref_samp = torch.as_tensor(ref_samp).double()
    e_l2 = abs(float(got.norm()) - ref_l2) / ref_l2
    e_sum = abs(float(got.sum()) - ref_sum) / (ref_l2 * got.numel() ** 0.5)
    e_samp = float((sample(got) - ref_samp).norm()) / max(float(ref_samp.norm()), 1e-3 * ref_l2)
    return e_l2, e_sum, e_samp


def rel_max(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))
