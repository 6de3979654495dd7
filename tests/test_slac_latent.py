"""N3b -- the SLAC latent model (posterior / prior heads, KL, image and reward likelihoods).  PINNED parity:
tests/golden/slac_latent_golden_v1.npz holds fp64 results of the REAL reference LatentModel (rlkit/torch/slac/network/
latent.py:174-311) run with the seeded weights, inputs and noise of tests/slac_latent_ref.py, and `ref32_err`, the deviation of
the reference's own fp32 run from them.  (The reference's state_dict has 72 keys for 60 distinct parameters: 12 keys are the
aliases z2_posterior_init / z2_posterior.)

fp32 tolerance of every quantity: K_TOL x max(ref32_err of that quantity, 1e-6).  The HIP path is the same arithmetic in the same
precision in another summation order (MFMA K-chunks, the split first layer, fixed-order block reductions).  Worst observed
ratios (deviation / max(ref32_err, 1e-6)) on an MI355X, per group: losses 0.29, samples 0.71, head gradients 1.90, conv
gradients 1.19; K_TOL is the round number above them."""
import os

import numpy as np
import pytest
import torch

import slac_latent_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "slac_latent_golden_v1.npz"))
K_TOL = 4.0
FLOOR = 1e-6
NAMES = [str(k) for k in G["param_names"]]
MID = ("post_mean", "post_std", "z1", "z2", "prior_mean", "prior_std")
WORST = {}


def _note(group, ratio):
    WORST[group] = max(WORST.get(group, 0.0), ratio)


def _params():
    p = R.make_params()
    assert np.isclose(R.checksum(p), float(G["checksum"]), rtol=1e-9)       # identical weights to the ones the reference ran with
    assert NAMES == list(p.keys()) and len(NAMES) == 60
    assert [int(v) for v in G["dims"]] == [R.B, R.S, R.A]
    return p


def _check(group, err, ref_err, k=K_TOL, what=""):
    tol = k * max(float(ref_err), FLOOR)
    _note(group, err / max(float(ref_err), FLOOR))
    assert err <= tol, (group, what, err, tol)


def _check_all(losses, mid, grads, bound=None, prefix=""):
    """bound None: K_TOL x ref32_err per quantity; else (forward bound, gradient bound) as fixed relative tolerances."""
    for i, name in enumerate(("kld", "image", "reward")):
        err = abs(float(losses[i]) - float(G["losses"][i])) / abs(float(G["losses"][i]))
        if bound is None:
            _check(prefix + "losses", err, G["losses_ref32_err"][i], what=name)
        else:
            assert err <= bound[0], (name, err)
    for k in MID:
        err = R.rel_max(mid[k], G["mid." + k])
        if bound is None:
            _check(prefix + "samples", err, G[f"mid.{k}.ref32_err"], what=k)
        else:
            assert err <= bound[1], (k, err)          # downstream of the (bf16) encoder
    compared = 0
    for k in NAMES:
        assert float(G[f"grad.{k}.l2"]) > 0 and np.abs(G[f"grad.{k}.samp"]).sum() > 0     # no reference gradient is zero
        assert grads[k] is not None, k
        errs = R.grad_measures(grads[k], float(G[f"grad.{k}.sum"]), float(G[f"grad.{k}.l2"]), G[f"grad.{k}.samp"])
        group = prefix + ("conv gradients" if k.startswith(("encoder.", "decoder.")) else "head gradients")
        for e, r, m in zip(errs, G[f"grad.{k}.ref32_err"], ("l2", "sum", "samp")):
            if bound is None:
                _check(group, e, r, what=k + ":" + m)
            else:
                assert e <= bound[1], (k, m, e)
        compared += 1
    assert compared == 60                                                    # no gradient is skipped


def _inputs(dtype=torch.float64):
    state_u8, action, reward, done, noise = R.make_inputs()
    state = (state_u8.double() / 255.0).to(dtype)
    return state_u8, state, action.to(dtype), reward.to(dtype), done.to(dtype), noise.to(dtype)


# ---- CPU -------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("s2p_gauss_head_fwd", "s2p_gauss_head_bwd", "s2p_linear_add_fwd", "s2p_linear_add_bwd", "s2p_gauss_kl",
               "s2p_gauss_ll", "s2p_gauss_ll_image")


def test_library_exports_the_latent_entry_points():
    from s2p_amd import _lib
    L = _lib.lib()
    assert L.s2p_version() == 125
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in _lib.SIGNATURES, name


def test_latent_entry_points_refuse_bad_arguments_without_a_device():
    from s2p_amd import _lib
    L = _lib.lib()
    p = 4096                                        # a non-NULL, 16-byte aligned address: refusals happen before any launch
    calls = {
        "head_fwd null raw": lambda: L.s2p_gauss_head_fwd(None, 64, 4, 32, None, 0, p, 32, None, 0, None, 0, None, 0, None),
        "head_fwd negative": lambda: L.s2p_gauss_head_fwd(p, 64, -1, 32, None, 0, p, 32, None, 0, None, 0, None, 0, None),
        "head_fwd short pitch": lambda: L.s2p_gauss_head_fwd(p, 63, 4, 32, None, 0, p, 32, None, 0, None, 0, None, 0, None),
        "head_fwd sample without eps": lambda: L.s2p_gauss_head_fwd(p, 64, 4, 32, None, 0, None, 0, None, 0, p, 32, None, 0, None),
        "head_fwd no output": lambda: L.s2p_gauss_head_fwd(p, 64, 4, 32, None, 0, None, 0, None, 0, None, 0, None, 0, None),
        "head_bwd null draw": lambda: L.s2p_gauss_head_bwd(p, 64, 4, 32, None, 0, p, 32, None, 0, None, 0, None, 0, None, 64, None),
        "head_bwd dz without eps": lambda: L.s2p_gauss_head_bwd(p, 64, 4, 32, None, 0, None, 0, None, 0, p, 32, None, 0, p, 64, None),
        "lin_add_fwd K % 4": lambda: L.s2p_linear_add_fwd(p, 4, 6, 8, p, 8, None, 16, None, 0, 0, 0.2, p, 16, 16, None),
        "lin_add_fwd misaligned": lambda: L.s2p_linear_add_fwd(p + 4, 4, 8, 8, p, 8, None, 16, None, 0, 0, 0.2, p, 16, 16, None),
        "lin_add_fwd null": lambda: L.s2p_linear_add_fwd(None, 4, 8, 8, p, 8, None, 16, None, 0, 0, 0.2, p, 16, 16, None),
        "lin_add_fwd short add": lambda: L.s2p_linear_add_fwd(p, 4, 8, 8, p, 8, None, 16, p, 8, 0, 0.2, p, 16, 16, None),
        "lin_add_fwd n_store": lambda: L.s2p_linear_add_fwd(p, 4, 8, 8, p, 8, None, 16, None, 0, 0, 0.2, p, 16, 32, None),
        "lin_add_bwd no output": lambda: L.s2p_linear_add_bwd(p, 8, p, 16, None, 0, 4, 8, 8, 16, None, 0, 0, 0.2, None, 0, None, None, 0, 0, None, 0, None),
        "lin_add_bwd tanh": lambda: L.s2p_linear_add_bwd(p, 8, p, 16, p, 16, 4, 8, 8, 16, None, 0, 3, 0.2, None, 0, None, None, 0, 0, p, 16, None),
        "lin_add_bwd act without y": lambda: L.s2p_linear_add_bwd(p, 8, p, 16, None, 0, 4, 8, 8, 16, None, 0, 2, 0.2, None, 0, None, None, 0, 0, p, 16, None),
        "lin_add_bwd dx without w": lambda: L.s2p_linear_add_bwd(p, 8, p, 16, None, 0, 4, 8, 8, 16, None, 0, 0, 0.2, None, 0, None, p, 8, 0, None, 0, None),
        "kl null": lambda: L.s2p_gauss_kl(None, p, 32, p, p, 32, 2, 3, 32, 1, 0.5, p, None, None, 0, None, None, 0, None),
        "kl negative": lambda: L.s2p_gauss_kl(p, p, 32, p, p, 32, 2, -3, 32, 1, 0.5, p, None, None, 0, None, None, 0, None),
        "kl short pitch": lambda: L.s2p_gauss_kl(p, p, 31, p, p, 32, 2, 3, 32, 1, 0.5, p, None, None, 0, None, None, 0, None),
        "ll null": lambda: L.s2p_gauss_ll(p, 1, None, 1, p, None, 8, 1.0, p, None, None, None),
        "ll negative": lambda: L.s2p_gauss_ll(p, 1, p, 1, p, None, -8, 1.0, p, None, None, None),
        "ll_image dtype": lambda: L.s2p_gauss_ll_image(7, p, 4, p, 0, 1, 3, 16, 0.3, 1.0, p, None, None),
        "ll_image pitch": lambda: L.s2p_gauss_ll_image(1, p, 4, p, 0, 1, 3, 16, 0.3, 1.0, p, None, None),
        "ll_image misaligned": lambda: L.s2p_gauss_ll_image(0, p + 4, 4, p, 0, 1, 3, 16, 0.3, 1.0, p, None, None),
        "ll_image sigma": lambda: L.s2p_gauss_ll_image(0, p, 4, p, 0, 1, 3, 16, 0.0, 1.0, p, None, None),
    }
    for what, call in calls.items():
        assert call() != 0 and L.s2p_last_error(), what
    # a size of 0 is a no-op that looks at no pointer
    assert L.s2p_gauss_head_fwd(None, 0, 0, 32, None, 0, None, 0, None, 0, None, 0, None, 0, None) == 0
    assert L.s2p_gauss_head_bwd(None, 0, 4, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None) == 0
    assert L.s2p_linear_add_fwd(None, 0, 8, 8, None, 8, None, 16, None, 0, 0, 0.2, None, 16, 16, None) == 0
    assert L.s2p_linear_add_bwd(None, 8, None, 16, None, 0, 0, 8, 8, 16, None, 0, 0, 0.2, None, 0, None, None, 0, 0, None, 0, None) == 0
    assert L.s2p_gauss_kl(None, None, 0, None, None, 0, 0, 3, 32, 1, 0.5, None, None, None, 0, None, None, 0, None) == 0
    assert L.s2p_gauss_ll(None, 1, None, 1, None, None, 0, 1.0, None, None, None, None) == 0
    assert L.s2p_gauss_ll_image(0, None, 4, None, 0, 0, 3, 16, 0.3, 1.0, None, None, None) == 0


def test_torch_restatement_reproduces_the_reference_in_fp64():
    """Proves the fixture, the seeded weights and the eps order are what the GPU tests assume."""
    p = {k: v.double().requires_grad_(True) for k, v in _params().items()}
    _, state, action, reward, done, noise = _inputs(torch.float64)
    losses, mid = R.calculate_loss(p, state, action, reward, done, noise)
    sum(losses).backward()
    for i in range(3):
        assert abs(float(losses[i]) - float(G["losses"][i])) <= 1e-9 * abs(float(G["losses"][i]))
    for k in MID:
        assert R.rel_max(mid[k], G["mid." + k]) <= 1e-9, k
    for k in NAMES:
        errs = R.grad_measures(p[k].grad, float(G[f"grad.{k}.sum"]), float(G[f"grad.{k}.l2"]), G[f"grad.{k}.samp"])
        assert max(errs) <= 1e-9, (k, errs)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _model(dtype):
    from s2p_amd.slac import LatentModel
    m = LatentModel((3, 100, 100), (R.A,), image_size=100, dtype=dtype)
    m.load_state_dict(R.full_state_dict(_params()), strict=True)
    return m


def _grads(m):
    named = dict(m.named_parameters())
    assert set(named) == set(NAMES)
    return {k: named[k].grad for k in NAMES}


@pytest.mark.gpu
def test_state_dict_keys_shapes_and_aliasing(hip_device, tmp_path):
    m = _model(torch.float32)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in G["state_dict_keys"]] and len(sd) == 72
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in G["state_dict_shapes"]]
    assert m.z2_posterior_init is m.z2_prior_init and m.z2_posterior is m.z2_prior
    assert sd["z2_posterior.net.0.weight"].data_ptr() == sd["z2_prior.net.0.weight"].data_ptr()
    assert len(list(m.parameters())) == 60 and sum(p.numel() for p in m.parameters()) == 5395525
    m.save_model(str(tmp_path))
    from s2p_amd.slac import Encoder, LatentModel
    m2 = LatentModel((3, 100, 100), (R.A,), image_size=100)
    m2.load_state_dict(torch.load(os.path.join(tmp_path, "latent.pth")), strict=True)
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    enc_sd = torch.load(os.path.join(tmp_path, "encoder.pth"))
    assert set(enc_sd) == set(Encoder(3, 256, 100).state_dict())
    with pytest.raises(NotImplementedError):
        LatentModel((3, 64, 64), (R.A,), image_size=64)


@pytest.mark.gpu
def test_fp32_matches_the_real_reference(hip_device, capsys):
    m = _model(torch.float32)
    _, state, action, reward, done, noise = _inputs(torch.float32)
    with torch.no_grad():
        feat = m.encoder(state)
        pm, ps, z1, z2 = m.sample_posterior(feat, action, noise)
        qm, qs = m.sample_prior(action, z2)
    assert pm.shape == (R.B, R.S + 1, 32) and z2.shape == (R.B, R.S + 1, 256) and qm.shape == (R.B, R.S + 1, 32)
    mid = dict(post_mean=pm, post_std=ps, z1=z1, z2=z2, prior_mean=qm, prior_std=qs)
    losses = m.calculate_loss(state, action, reward, done, noise)
    sum(losses).backward()
    torch.cuda.synchronize()
    try:
        _check_all(losses, mid, _grads(m))
    finally:
        with capsys.disabled():
            print("\nworst deviation / max(ref32_err, 1e-6) per group:", {k: round(v, 3) for k, v in WORST.items()})


@pytest.mark.gpu
def test_fp32_uint8_frames_give_the_same_losses(hip_device):
    """uint8 NHWC frames (what Encoder.forward already accepts): same pixels, so the same losses within the fp32 bound."""
    m = _model(torch.float32)
    state_u8, _, action, reward, done, noise = _inputs(torch.float32)
    frames = state_u8.permute(0, 1, 3, 4, 2).contiguous()
    losses = m.calculate_loss(frames, action, reward, done, noise)
    for i in range(3):
        err = abs(float(losses[i]) - float(G["losses"][i])) / abs(float(G["losses"][i]))
        assert err <= K_TOL * max(float(G["losses_ref32_err"][i]), FLOOR), (i, err)


@pytest.mark.gpu
def test_bf16_stacks_match_the_real_reference(hip_device):
    """bf16 conv stacks, fp32 heads: the bounds tests/test_slac.py uses for these stacks in bf16 (4e-2 forward quantities and
    losses, 1e-1 for gradients and for anything downstream of the encoder)."""
    m = _model(torch.bfloat16)
    _, state, action, reward, done, noise = _inputs(torch.float32)
    with torch.no_grad():
        feat = m.encoder(state)
        pm, ps, z1, z2 = m.sample_posterior(feat, action, noise)
        qm, qs = m.sample_prior(action, z2)
    mid = dict(post_mean=pm, post_std=ps, z1=z1, z2=z2, prior_mean=qm, prior_std=qs)
    losses = m.calculate_loss(state, action, reward, done, noise)
    sum(losses).backward()
    torch.cuda.synchronize()
    _check_all(losses, mid, _grads(m), bound=(4e-2, 1e-1))


def _two_runs(m):
    _, state, action, reward, done, noise = _inputs(torch.float32)
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        sum(m.calculate_loss(state, action, reward, done, noise)).backward()
        runs.append({k: g.clone() for k, g in _grads(m).items()})
    torch.cuda.synchronize()
    diff = {}
    for k in NAMES:
        if not torch.equal(runs[0][k], runs[1][k]):
            diff[k] = float((runs[0][k] - runs[1][k]).abs().max() / runs[0][k].abs().max())
    return diff


@pytest.mark.gpu
def test_gradients_are_bitwise_reproducible(hip_device):
    """Two identical calculate_loss + backward calls give bitwise identical gradients for all 60 parameters: the heads and the
    chain sum in a fixed order, and the conv stacks' backward takes the atomics-free weight-gradient / channel-sum route
    (s2p_conv2d_wgrad_det_workspace, s2p_channel_sum_ws) in fp32 as well."""
    diff = _two_runs(_model(torch.float32))
    print("parameters whose gradient differs between two identical calls (max abs difference / max abs):", diff)
    assert not diff, diff


@pytest.mark.gpu
def test_head_gradients_are_bitwise_reproducible(hip_device):
    """The 36 parameters of the Gaussian heads: the chain, its batched weight gradients, KL and both likelihood seeds."""
    diff = _two_runs(_model(torch.float32))
    assert not [k for k in diff if not k.startswith(("encoder.", "decoder."))], diff


@pytest.mark.gpu
def test_noise_is_drawn_on_the_device(hip_device):
    m = _model(torch.float32)
    _, state, action, reward, done, noise = _inputs(torch.float32)
    losses = m.calculate_loss(state, action, reward, done)                    # noise=None: drawn on the device
    assert all(bool(torch.isfinite(v)) for v in losses)
    with torch.no_grad():
        feat = m.encoder(state)
        a, b = m.sample_posterior(feat, action), m.sample_posterior(feat, action)
    assert float((a[2] - b[2]).abs().max()) > 0 and float((a[3] - b[3]).abs().max()) > 0


@pytest.mark.gpu
def test_no_grad_posterior_keeps_no_backward_state(hip_device):
    """prepare_batch use (slac/algo.py:127-141): encoder + sample_posterior under no_grad."""
    from s2p_amd.slac import create_feature_actions
    m = _model(torch.float32)
    _, state, action, _, _, noise = _inputs(torch.float32)
    with torch.no_grad():
        feat = m.encoder(state)
        out = m.sample_posterior(feat, action, noise)
    assert m.chain_state_bytes == 0 and all(t.grad_fn is None and not t.requires_grad for t in out) and feat.grad_fn is None
    ref = m.sample_posterior(m.encoder(state), action, noise)                # the same values with the backward state kept
    assert m.chain_state_bytes > 0 and ref[2].grad_fn is not None
    for a, b in zip(out, ref):
        assert torch.equal(a, b.detach())
    fa, n_fa = create_feature_actions(feat, action.cuda())
    assert fa.shape == (R.B, R.S * 256 + (R.S - 1) * R.A) and n_fa.shape == fa.shape
    assert torch.equal(fa[:, :256], feat[:, 0]) and torch.equal(n_fa[:, :256], feat[:, 1])


@pytest.mark.gpu
def test_adam_step_changes_the_next_loss(hip_device):
    m = _model(torch.float32)
    _, state, action, reward, done, noise = _inputs(torch.float32)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    before = [float(v) for v in m.calculate_loss(state, action, reward, done, noise)]
    opt.zero_grad()
    sum(m.calculate_loss(state, action, reward, done, noise)).backward()
    opt.step()
    after = [float(v) for v in m.calculate_loss(state, action, reward, done, noise)]
    assert all(a != b for a, b in zip(after, before))                        # packed operands were refreshed
