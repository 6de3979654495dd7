"""Plain-torch restatement of the closed-loop rollout of a `feature_action` policy (SPEC.md N3o) and the seeded inputs of its
fixture -- TEST INFRASTRUCTURE ONLY.  Builds on the latent weights of tests/slac_latent_ref.py, the z0 / eps pools of
tests/slac_predict_ref.py and the conv stacks of oracle/slac_oracle.py.  Shared by tests/golden/make_golden_slac_imagine_fa.py (which
runs the real reference's modules with these weights and inputs) and tests/test_imagine_feature_action*.py."""
import torch

import slac_imagine_ref as IR
import slac_latent_ref as R
import slac_predict_ref as P
import slac_oracle as SO

Z1, Z2, Z, FEAT = P.Z1, P.Z2, P.Z, R.FEAT
S, A, W = 8, 6, 128                                         # frames of the policy's window, action width, hidden width of the policy
OBS = S * FEAT + (S - 1) * A                                # 2090
B, H, CONTEXT = 2, 3, 8                                     # the fixture's batch, horizon and context
SEEDS = dict(policy=951, window=952)
ROLLOUTS = ("sampled", "mean")
QUANTITIES = ("actions", "z1_mean", "z1_std", "z", "obs", "frame_sum", "frame_l2", "frame_samp")          # [b,h,...]: one ref32_err per step


def make_policy_params(w=W, a=A, s=S, seed=None):
    """Seeded weights of TanhGaussianPolicy(hidden [w, w], s 256 + (s - 1) a, a) under the reference's keys; `last_fc` is drawn wide
    so that tanh(mean) spreads over (-1, 1), as tests/slac_imagine_ref.py does for the latent_z policy."""
    g = torch.Generator().manual_seed((SEEDS["policy"] if seed is None else seed) + 7 * w + a)
    p, n_in = {}, s * FEAT + (s - 1) * a
    for i, gain in enumerate((4.0, 1.0)):                  # (the seeded encoder's features are small, |f| ~ 0.03: fc0 is drawn wide too)
        p["fc%d.weight" % i] = (torch.rand(w, n_in, generator=g) * 2 - 1) * gain / n_in ** 0.5
        p["fc%d.bias" % i] = torch.randn(w, generator=g) * 0.05
        n_in = w
    p["last_fc.weight"] = (torch.rand(a, w, generator=g) * 2 - 1) * 14.0 / w ** 0.5
    p["last_fc.bias"] = torch.randn(a, generator=g) * 0.05
    p["last_fc_log_std.weight"] = (torch.rand(a, w, generator=g) * 2 - 1) * 1e-3
    p["last_fc_log_std.bias"] = (torch.rand(a, generator=g) * 2 - 1) * 1e-3
    return p


def make_window(b, a=A, s=S):
    """A seeded policy-input row per sample, [b, s 256 + (s - 1) a]: rows of one pool, so row i does not depend on b (b <= 33).
    Features ~ N(0, 0.5), actions ~ U(-1, 1).  (The fixture's window is the encoder's features of real context frames instead.)"""
    assert b <= P.POOL
    g = torch.Generator().manual_seed(SEEDS["window"] + a + 100 * s)
    f = torch.randn(P.POOL, s * FEAT, generator=g) * 0.5
    u = torch.rand(P.POOL, (s - 1) * a, generator=g) * 2 - 1
    return torch.cat([f, u], dim=1)[:b].contiguous()


def make_inputs(b, h):
    """z0 [b,288] and eps [b,h,288] of tests/slac_predict_ref.py's pools."""
    z0, _, noise = P.make_inputs(b, h, A)
    return z0, noise


def context_frames(b=B, context=CONTEXT):
    """The fixture's context: uint8 frames [b,context+1,3,100,100] and actions [b,context,A] of tests/slac_latent_ref.py's inputs."""
    state_u8, action, _, _, _ = R.make_inputs(b, context, A)
    return state_u8, action


def window_of(feat, action, s=S):
    """`create_feature_actions`' next_fa of the last s + 1 frames: the last s features and the s - 1 actions between them."""
    n = feat.shape[0]
    return torch.cat([feat[:, -s:].reshape(n, -1), action[:, -(s - 1):].reshape(n, -1)], dim=-1)


def push(window, feat, action, a=A, s=S):
    """window(h+1) from window(h): features and actions shifted left by one, the new ones last."""
    f, u = window[:, :s * FEAT], window[:, s * FEAT:]
    return torch.cat([f[:, FEAT:], feat, u[:, a:], action], dim=1)


def quantise(img):
    """clamp(round(v * 255), 0, 255) / 255 in the dtype of img."""
    return torch.round(img * 255.0).clamp(0.0, 255.0) / 255.0


def rollout(p, pol, z0, window, noise, quantize=False, final_obs=True):
    """The loop of SPEC.md N3o on the restated modules -> dict: actions [b,h,A], z1_mean, z1_std [b,h,32], z [b,h,288], obs
    [b,h(+1),OBS], frames [b,h(-1 without final_obs),3,100,100]: what the encoder saw."""
    enc = {k[len("encoder."):]: v for k, v in p.items() if k.startswith("encoder.")}
    z, acts, ms, ss, zs, obs, frames = z0, [], [], [], [], [], []
    Hn = noise.shape[1]
    for k in range(Hn):
        obs.append(window)
        a = IR.act(pol, window)
        z2 = z[:, Z1:]
        m1, s1 = R.gaussian(p, "z1_prior", torch.cat([z2, a], dim=1))
        z1 = m1 + noise[:, k, :Z1] * s1
        m2, s2 = R.gaussian(p, "z2_prior", torch.cat([z1, z2, a], dim=1))
        z = torch.cat([z1, m2 + noise[:, k, Z1:] * s2], dim=1)
        acts.append(a); ms.append(m1); ss.append(s1); zs.append(z)
        if k == Hn - 1 and not final_obs:
            break
        img = P.decode(p, z[:, None])                                     # [b,1,3,100,100]
        img = quantise(img) if quantize else img.clamp(0.0, 1.0)
        frames.append(img[:, 0])
        window = push(window, SO.encoder_forward(enc, img)[:, 0], a)
    if final_obs:
        obs.append(window)
    st = lambda xs: torch.stack(xs, 1)
    return dict(actions=st(acts), z1_mean=st(ms), z1_std=st(ss), z=st(zs), obs=st(obs), frames=st(frames))


def measures(out):
    """The eight QUANTITIES of a rollout dict: its per-step tensors and the three frame measures of tests/slac_predict_ref.py."""
    fs, fl, fsamp = P.frame_measures(out["frames"])
    return dict(actions=out["actions"], z1_mean=out["z1_mean"], z1_std=out["z1_std"], z=out["z"], obs=out["obs"], frame_sum=fs,
                frame_l2=fl, frame_samp=fsamp)


step_err = IR.step_err
