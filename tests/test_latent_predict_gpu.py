"""N3i -- open-loop prediction from the SLAC latent model: `LatentModel.predict` on its per-layer path and as one launch
(csrc/gauss_chain.hip: s2p_prior_chain_fwd, `LatentModel.fused_chain`), `predict_reward`, `slac_predict.open_loop`, predict_latent.py.

The acceptance between the two paths is BITWISE (torch.equal): both run the same MFMA sequence per output element over the chain
columns, then (acc + add) + bias and the same epilogues, at the smallest shapes that reach every code path (a partial 16-row tile,
exactly one tile, one row more, three workgroups; one step, one loop turn, the workload's nine; action widths 6 and 1 for both
paddings of the hoisted K).  The toleranced checks -- against the recorded run of the reference's modules
(tests/golden/slac_predict_golden_v1.npz) and against `sample_prior`, whose first layer is ONE K = 256 + A sum -- use the project's
rule: err <= K_TOL x max(ref32_err, 1e-6), K_TOL = 4, with ref32_err the deviation of the reference's own fp32 run from its fp64 run
(1e-7 .. 1.4e-6 here, no growth over the 12 steps: all but one quantity sit on the 1e-6 floor).
Measured on an MI355X: see test_pinned_parity's docstring."""
import os

import numpy as np
import pytest
import torch

import slac_buffer_ref as SB
import slac_latent_ref as R
import slac_predict_ref as PR
from guard_region import Region
from slac_chain_util import build_model, count_calls, model_cache

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
K_TOL, FLOOR = 4.0, 1e-6
Z1, Z2, Z = 32, 256, 288
BS, HS, AS = (1, 15, 16, 17, 33), (1, 2, 9), (6, 1)
NAME = "s2p_prior_chain_fwd"
LN2 = 0.6931472
OUT = ("mean", "std", "z")


@pytest.fixture(scope="module")
def models(hip_device):
    """action width -> a LatentModel with the seeded weights of tests/slac_latent_ref.py; built once, left with fused_chain False."""
    return model_cache()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "slac_predict_golden_v1.npz"))


def _inputs(B, H, A):
    return [t.cuda() for t in PR.make_inputs(B, H, A)]                 # row b, step k are the same whatever B and H are


def _predict(m, fused, z0, actions, noise=None, sample=True):
    m.fused_chain = fused
    try:
        with torch.enable_grad():                                      # predict itself must switch grad off
            out = m.predict(z0, actions, noise, sample)
        torch.cuda.synchronize()
        assert all(t.grad_fn is None and not t.requires_grad for t in out)
        return [t.clone() for t in out]
    finally:
        m.fused_chain = False


# ---- 1. bitwise against the per-layer path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("A", AS)
def test_fused_equals_per_layer_bitwise(models, A, H):
    m = models(A)
    for B in BS:
        args = _inputs(B, H, A)
        want, got = _predict(m, False, *args), _predict(m, True, *args)
        for name, a, b in zip(OUT, got, want):
            assert a.shape == b.shape == (B, H, Z if name == "z" else Z1)
            assert bool(torch.isfinite(b).all()) and float(b.abs().max()) > 0
            diff = int((a.view(torch.int32) != b.view(torch.int32)).sum())
            print("A %d H %d B %2d %-4s elements that differ: %d of %d" % (A, H, B, name, diff, a.numel()))
            assert torch.equal(a, b), (A, H, B, name, diff)


def test_the_mean_rollout_and_the_drawn_noise(models):
    m = models(6)
    z0, actions, noise = _inputs(17, 9, 6)
    for fused in (False, True):
        zero = _predict(m, fused, z0, actions, torch.zeros_like(noise))
        mean = _predict(m, fused, z0, actions, noise, sample=False)           # the noise argument is not used
        assert all(torch.equal(a, b) for a, b in zip(mean, zero))
        assert torch.equal(mean[2][:, 0, :Z1], mean[0][:, 0])                # z1 = its mean when eps = 0
        torch.manual_seed(5)
        d1 = _predict(m, fused, z0, actions)
        torch.manual_seed(5)
        d2 = _predict(m, fused, z0, actions)
        assert all(torch.equal(a, b) for a, b in zip(d1, d2)) and not torch.equal(d1[2], mean[2])
    with pytest.raises(ValueError):
        m.predict(z0[:, :Z2], actions)
    with pytest.raises(ValueError):
        m.predict(z0, actions[:5])
    with pytest.raises(ValueError):
        m.predict(z0, actions[..., :3])
    with pytest.raises(ValueError):
        m.predict(z0, actions, noise[:, :4])


# ---- 2. Markov restart ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
def test_markov_restart(models, fused):
    m = models(6)
    z0, actions, noise = _inputs(17, 9, 6)
    full = _predict(m, fused, z0, actions, noise)
    tail = _predict(m, fused, full[2][:, 3], actions[:, 4:], noise[:, 4:])
    for name, a, b in zip(OUT, tail, full):
        assert a.shape[1] == 5 and torch.equal(a, b[:, 4:]), name
    other = z0.clone()
    other[:, :Z1] = torch.randn(17, Z1, generator=torch.Generator().manual_seed(3)).cuda() * 10
    again = _predict(m, fused, other, actions, noise)                          # z1(0) is not an input of the chain
    assert all(torch.equal(a, b) for a, b in zip(again, full))


# ---- 3. rows do not meet ---------------------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_their_tile(models):
    A, H = 6, 9
    m = models(A)
    z0, actions, noise = _inputs(33, H, A)
    full = _predict(m, True, z0, actions, noise)
    for row in (0, 32):                                      # the first row of the first tile, the only row of the last one
        alone = _predict(m, True, z0[row:row + 1], actions[row:row + 1], noise[row:row + 1])
        for name, a, b in zip(OUT, alone, full):
            assert torch.equal(a[0], b[row]), (row, name)
    bad = 16                                                 # the first row of the second tile; rows 17..31 share its tile
    z0_nan = z0.clone()
    z0_nan[bad] = float("nan")
    got = _predict(m, True, z0_nan, actions, noise)
    others = [r for r in range(33) if r != bad]
    for name, a, b in zip(OUT, got, full):
        assert bool(torch.isnan(a[bad]).all()), name
        assert torch.equal(a[others], b[others]), name


# ---- 4. nothing else is written ----------------------------------------------------------------------------------------------------------
def _terms(m, actions):
    from s2p_amd.slac import _action_term
    A = actions.shape[2]
    return _action_term(actions, m.z1_prior.packed_cols(Z2, Z2 + A))[1], _action_term(actions, m.z2_prior.packed()["g1"][1][0])[1]


def _direct(m, z2_0, rc, rb, B, H, eps_view, mean, std, z):
    """The entry point itself on [B*H, C] views with any pitch."""
    from s2p_amd import ops
    v3 = lambda t: t.view(B, H, t.shape[1]) if t.is_contiguous() else t.as_strided((B, H, t.shape[1]), (H * t.stride(0), t.stride(0), 1))
    mlps = [ops.chain_mlp(m.z1_prior.packed(), k1=Z2), ops.chain_mlp(m.z2_prior.packed())]
    ops.prior_chain_fwd(z2_0, rc, rb, v3(eps_view), mlps, v3(mean), v3(std), v3(z))
    torch.cuda.synchronize()


def test_only_the_three_outputs_are_written(models):
    A, B, H = 6, 17, 9
    m = models(A)
    z0, actions, noise = _inputs(B, H, A)
    want = _predict(m, False, z0, actions, noise)
    eps = Region(B * H, Z, pitch=300, off=8, fill=noise.reshape(B * H, Z))
    mean, std = Region(B * H, Z1, pitch=40, off=4), Region(B * H, Z1, pitch=36, off=0)
    z = Region(B * H, Z, pitch=320, off=16)                  # a slice of a 320-wide buffer
    rc, rb = _terms(m, actions)
    params = m.z1_prior.layer_params() + m.z2_prior.layer_params()
    assert m.z1_prior.packed()["g1"][0][0].shape == (256, 264) and len(m.z1_prior.packed()["g1"]) == 1     # packed() is what it was
    z00, eps0, rc0, rb0 = z0.clone(), eps.buf.clone(), rc.clone(), rb.clone()
    weights0 = [p.detach().clone() for p in params]
    packs0 = [t.clone() for g in (m.z1_prior, m.z2_prior) for t in (g.packed()["g1"][0][0], g.packed()["w2"], g.packed()["w3"])]
    _direct(m, z0[:, Z1:], rc, rb, B, H, eps.v, mean.v, std.v, z.v)             # z2(0): a column slice of z0, read in place
    assert torch.equal(z0, z00) and torch.equal(eps.buf, eps0) and torch.equal(rc, rc0) and torch.equal(rb, rb0)
    assert all(torch.equal(p.detach(), w) for p, w in zip(params, weights0))
    packs = [t for g in (m.z1_prior, m.z2_prior) for t in (g.packed()["g1"][0][0], g.packed()["w2"], g.packed()["w3"])]
    assert all(torch.equal(a, b) for a, b in zip(packs, packs0))
    got = [mean.bits("mean"), std.bits("std"), z.bits("z")]
    for name, a, b, w in zip(OUT, got, want, (Z1, Z1, Z)):
        assert torch.equal(a.view(B, H, w), b.cpu()), name


# ---- 5. both softplus branches -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head,D", [("z1_prior", Z1), ("z2_prior", Z2)])
@pytest.mark.parametrize("bias", [30.0, -30.0])
def test_both_softplus_branches(hip_device, bias, head, D):
    """raw_std = +-30 + O(1): softplus is r + log1p(exp(-r)) on one side and log1p(exp(r)) ~ 1e-13 on the other, where std is the
    1e-5 floor.  z1_prior's std is an output; z2_prior's shows in z2 = mean + eps * std, so eps = 1 against eps = 0 at the first
    step (the same mean in both runs).  softplus(0) = ln 2 separates the branches."""
    A, B, H = 6, 17, 2
    m = build_model(A)
    with torch.no_grad():
        getattr(m, head).net._modules["4"].bias[D:] = bias
    z0, actions, noise = _inputs(B, H, A)
    rc, rb = _terms(m, actions)
    outs = {}
    for e in (None, 0.0, 1.0):
        eps = noise.clone()
        if e is not None:
            lo, hi = (Z1, Z) if D == Z2 else (0, Z1)
            eps[..., lo:hi] = e
        want = _predict(m, False, z0, actions, eps)             # the composition of the existing entry points
        mean, std, z = (torch.full((B, H, c), float("nan"), device=hip_device) for c in (Z1, Z1, Z))
        _direct(m, z0[:, Z1:], rc, rb, B, H, eps.view(B * H, Z), mean.view(B * H, Z1), std.view(B * H, Z1), z.view(B * H, Z))
        got = [mean, std, z]
        for name, a, b in zip(OUT, got, want):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all()), (name, e)
        assert float(std.min()) > 0
        outs[e] = got
    if D == Z1:
        sd = outs[None][1]
        print("bias %+.0f: z1 std in [%.6e, %.6e]" % (bias, float(sd.min()), float(sd.max())))
        assert (float(sd.min()) > LN2) if bias > 0 else (float(np.float32(1e-5)) <= float(sd.min()) and float(sd.max()) < LN2)
    else:
        step = outs[1.0][2][:, 0, Z1:] - outs[0.0][2][:, 0, Z1:]
        print("bias %+.0f: z2(eps 1) - z2(eps 0) in [%.6e, %.6e]" % (bias, float(step.min()), float(step.max())))
        assert float(step.min()) > 0 and ((float(step.min()) > LN2) if bias > 0 else float(step.max()) < LN2)


# ---- 6. tied to the existing module path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", AS)
def test_one_step_matches_sample_prior(models, golden, A):
    """sample_prior's first layer is ONE sum over K = 256 + A; predict's is (sum over 256) + action term: equal within the rule, not
    bitwise.  A wrong column split (z2 columns read at the wrong offset or pitch, action columns from the wrong place) is O(1)."""
    m = models(A)
    z0, actions, noise = _inputs(33, 1, A)
    with torch.no_grad():
        pm, ps = m.sample_prior(actions, z0[:, None, Z1:])
    for fused in (False, True):
        mean, std, _ = _predict(m, fused, z0, actions, noise)
        for name, got, want in (("z1_mean", mean[:, 0], pm[:, 1]), ("z1_std", std[:, 0], ps[:, 1])):
            err, ref = R.rel_max(got, want), max(float(golden["sampled.%s.ref32_err" % name]), FLOOR)
            print("A %d fused %d %s: deviation from sample_prior %.3e (%.3f of max(ref32_err, 1e-6))" % (A, fused, name, err, err / ref))
            assert err <= K_TOL * ref, (name, err)


# ---- 7. pinned parity ------------------------------------------------------------------------------------------------------------------------
def test_pinned_parity(models, golden, capsys):
    """Both rollouts, the reward head and the fp32-decoded frames against the recorded fp64 run of the reference's modules.
    Measured on an MI355X (worst deviation / max(ref32_err, 1e-6) over all 16 quantities; the bound is K_TOL = 4):
    0.854751 on both paths (sampled z1_mean; sampled z 0.420, mean z 0.458, reward_mean 0.684 / 0.688, frame sample 0.392 / 0.456,
    frame sum 0.049, frame L2 0.005), identical between the per-layer and the fused path in every quantity.  The H = 1 comparison
    with sample_prior (test_one_step_matches_sample_prior) measured 0.297 at most."""
    m = models(PR.A)
    z0, actions, noise = [t.cuda() for t in PR.make_inputs()]
    worst = {}
    for fused in (False, True):
        ratios = {}
        for rollout, sample in zip(PR.ROLLOUTS, (True, False)):
            mean, std, z = _predict(m, fused, z0, actions, noise, sample)
            with torch.no_grad():
                rm, rs = m.predict_reward(z0, z, actions)
                img = m.decoder(z)[0]
            assert rm.shape == rs.shape == (PR.B, PR.H) and img.shape == (PR.B, PR.H, 3, 100, 100)
            got = dict(zip(PR.QUANTITIES, (mean, std, z, rm, rs) + PR.frame_measures(img)))
            for k in PR.QUANTITIES:
                key = "%s.%s" % (rollout, k)
                ratios[key] = R.rel_max(got[k], golden[key]) / max(float(golden[key + ".ref32_err"]), FLOOR)
        worst[fused] = ratios
    with capsys.disabled():
        for key in worst[True]:
            print("\n%-22s deviation / max(ref32_err, 1e-6): per-layer %.6f, fused %.6f" % (key, worst[False][key], worst[True][key]), end="")
        print("\nworst: per-layer %.6f, fused %.6f" % (max(worst[False].values()), max(worst[True].values())))
    for fused in (False, True):
        for key, r in worst[fused].items():
            assert r <= K_TOL, (fused, key, r)
    assert worst[True] == worst[False]


# ---- 8. call counts --------------------------------------------------------------------------------------------------------------------------
def test_call_counts(models):
    m = models(6)
    args = _inputs(17, 9, 6)
    per_layer, fused = count_calls(lambda: _predict(m, False, *args)), count_calls(lambda: _predict(m, True, *args))
    print("library calls, per-layer:", per_layer, " fused:", fused)
    assert fused == {NAME: 1, "s2p_linear_fwd": 2}
    assert per_layer == {"s2p_linear_add_fwd": 18, "s2p_gauss_head_fwd": 18, "s2p_linear_fwd": 2 + 36}
    assert "s2p_posterior_chain_fwd" not in fused and "s2p_posterior_chain_fwd" not in per_layer


# ---- 9. open_loop and the command line -------------------------------------------------------------------------------------------------------
CONTEXT, HORIZON = 8, 3
MODEL = {"z0", "z1_mean", "z1_std", "z", "frames", "reward_mean", "reward_std", "reward_abs_err"}          # bitwise reproducible
METRICS = {"psnr", "ssim", "baseline_psnr", "baseline_ssim"}       # s2p_image_metrics sums with fp32 atomics: equal to ~1e-6, not bitwise
KEYS = MODEL | METRICS


def _same(a, b, k):
    """Bitwise for what the model computes; the metrics' per-image sums are fp32 atomic adds of a few hundred positive partials, whose
    order changes the last bits (relative 1e-6 at most for that many terms; 1e-4 is asked)."""
    if k in MODEL:
        return torch.equal(a, b)
    return bool(torch.allclose(a, b, rtol=1e-4, atol=0.0))


@pytest.fixture(scope="module")
def real_windows():
    from s2p_amd.slac_predict import gather, windows
    data = SB.real_dataset(2, 12, 100, 100)
    starts = windows(data, CONTEXT + HORIZON, stride=1)
    assert starts.tolist() == [0, 1, 12, 13]
    frames, actions, rewards = gather(data, starts, CONTEXT + HORIZON)
    frames[0, CONTEXT + 1] = frames[0, CONTEXT]              # window 0: the first future frame IS the last context frame
    return data, frames, actions, rewards


def _noises(B):
    g = torch.Generator().manual_seed(77)
    return torch.randn(B, CONTEXT + 1, Z, generator=g).cuda(), torch.randn(B, HORIZON, Z, generator=g).cuda()


def test_open_loop(models, real_windows):
    from s2p_amd.slac_predict import open_loop
    m = models(SB.A)
    _, frames, actions, rewards = real_windows
    B = frames.shape[0]
    pn, n = _noises(B)
    outs = {}
    try:
        for fused in (False, True):
            m.fused_chain = fused
            outs[fused] = open_loop(m, frames, actions, rewards, context=CONTEXT, noise=n, posterior_noise=pn)
            torch.cuda.synchronize()
    finally:
        m.fused_chain = False
    o = outs[True]
    assert set(o) == KEYS and all(v.is_cuda and v.grad_fn is None for v in o.values())
    assert o["z0"].shape == (B, Z) and o["z"].shape == (B, HORIZON, Z) and o["z1_mean"].shape == o["z1_std"].shape == (B, HORIZON, Z1)
    assert o["frames"].shape == (B, HORIZON, 3, 100, 100) and 0.0 <= float(o["frames"].min()) and float(o["frames"].max()) <= 1.0
    for k in ("psnr", "ssim", "baseline_psnr", "baseline_ssim", "reward_mean", "reward_std", "reward_abs_err"):
        assert o[k].shape == (B, HORIZON), k
    for k in ("psnr", "ssim", "baseline_ssim", "reward_mean", "reward_std", "reward_abs_err", "z"):
        assert bool(torch.isfinite(o[k]).all()), k
    bp = o["baseline_psnr"]
    assert float(bp[0, 0]) == float("inf") and float(o["baseline_ssim"][0, 0]) == pytest.approx(1.0, abs=1e-5)
    rest = torch.ones_like(bp, dtype=torch.bool)
    rest[0, 0] = False
    assert bool(torch.isfinite(bp[rest]).all()) and float(bp[rest].max()) < 20.0          # independent uniform noise frames: ~7.8 dB
    assert float(o["reward_std"].min()) > 0
    want = (o["reward_mean"] - torch.as_tensor(rewards[:, CONTEXT:]).cuda()).abs()
    assert torch.equal(o["reward_abs_err"], want)
    for k in KEYS:
        assert _same(outs[True][k], outs[False][k], k), k
    # the mean rollout is a function of its inputs alone, and no rewards -> no error column
    a = open_loop(m, frames, actions, context=CONTEXT, sample=False)
    b = open_loop(m, frames, actions, context=CONTEXT, sample=False)
    assert set(a) == KEYS - {"reward_abs_err"} and all(_same(a[k], b[k], k) for k in a)
    with pytest.raises(ValueError):
        open_loop(m, frames[:, :CONTEXT + 1], actions[:, :CONTEXT], context=CONTEXT)          # no step left to predict


def test_open_loop_bf16_stacks(models, real_windows):
    """bf16 conv stacks, fp32 heads: z of the rollout within the bound tests/test_slac_latent.py uses for anything downstream of the
    bf16 encoder (1e-1, R.rel_max) of the fp32 model's."""
    from s2p_amd.slac_predict import open_loop
    _, frames, actions, rewards = real_windows
    pn, n = _noises(frames.shape[0])
    ref = open_loop(models(SB.A), frames, actions, rewards, context=CONTEXT, noise=n, posterior_noise=pn)
    got = open_loop(build_model(SB.A, torch.bfloat16), frames, actions, rewards, context=CONTEXT, noise=n, posterior_noise=pn)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for k, v in got.items() if k != "baseline_psnr")
    err = R.rel_max(got["z"], ref["z"])
    print("bf16 stacks: z deviates from the fp32 model's by %.3e" % err)
    assert err <= 1e-1
    assert _same(got["baseline_psnr"], ref["baseline_psnr"], "baseline_psnr")             # the baseline does not touch the model


def test_command_line(models, real_windows, tmp_path, capsys):
    import predict_latent
    data = real_windows[0]
    path, ldir = str(tmp_path / "real.npz"), str(tmp_path / "latent")
    np.savez(path, **data)
    models(SB.A).save_model(ldir)
    res = {}
    for fused in (False, True):
        out = str(tmp_path / ("pred%d.npz" % fused))
        argv = ["--data", path, "--latent_dir", ldir, "--out", out, "--context", str(CONTEXT), "--horizon", str(HORIZON), "--windows", "3",
                "--stride", "1", "--batch", "2", "--seed", "4", "--frames"] + (["--fused_chain"] if fused else [])
        predict_latent.main(argv)
        with np.load(out) as f:
            res[fused] = {k: f[k] for k in f.files}
    text = capsys.readouterr().out
    assert "baseline_psnr" in text and "|reward error|" in text and text.count("wrote") == 2
    r = res[True]
    cols = set(predict_latent.COLUMNS)
    assert set(r) == cols | {"window_" + k for k in cols} | {"starts", "z", "reward_mean", "reward_std", "frames"}
    assert r["starts"].tolist() == [0, 12, 13]                                            # 3 of the 4 windows, evenly spread
    assert all(r[k].shape == (HORIZON,) and r["window_" + k].shape == (3, HORIZON) for k in cols)
    assert r["z"].shape == (3, HORIZON, Z) and r["frames"].shape == (3, HORIZON, 100, 100, 3) and r["frames"].dtype == np.uint8
    assert all(np.isfinite(r[k]).all() for k in r)
    assert np.allclose(r["psnr"], r["window_psnr"].astype(np.float64).mean(0))
    for k in r:
        metric = k.replace("window_", "") in METRICS
        assert np.allclose(res[True][k], res[False][k], rtol=1e-4, atol=0.0) if metric else np.array_equal(res[True][k], res[False][k]), k
    with pytest.raises(SystemExit, match="no trajectory"):
        predict_latent.main(["--data", path, "--latent_dir", ldir, "--out", str(tmp_path / "x.npz"), "--horizon", "5"])
