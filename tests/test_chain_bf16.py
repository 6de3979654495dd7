"""N3m on the host: the helper tests/chain_bf16_ref.py holds what tests/test_chain_bf16_gpu.py relies on (its exact data really is
exact in any summation order and really is rounded; its own fp32 runs leave at most HALF the rows non-tight that the GPU test lets a
kernel leave), the two bf16 entry points are exported, declared and refuse bad arguments before any launch, and the four command
lines take --bf16_chain only with --fused_chain."""
import ctypes
import os

import pytest
import torch

import chain_bf16_ref as C
import slac_latent_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POST, PRIOR = "s2p_posterior_chain_fwd_bf16", "s2p_prior_chain_fwd_bf16"
K1 = (256, 32, 256, 288)
P = 4096                                               # a non-NULL, 16-byte aligned address: refusals happen before any launch
TIGHT, CAP = 4e-6, 0.05                                # the GPU test's row bound (K_TOL x floor) and its cap on rows that miss it
SEEDS = (0, 1, 2)


def _f32(ts):
    return [t.float() for t in ts]


# ---- the exact data of the GPU test -------------------------------------------------------------------------------------------------
def test_exact_data_is_exact_in_any_order_and_is_rounded():
    A, B, T = 6, 33, 9
    p = C.exact_params(A)
    feat, action, noise = C.exact_inputs(B, T, A)
    m64, s64, z64 = C.posterior(p, feat, action, noise, torch.float64)
    m32, s32, z32 = C.posterior(p, feat, action, noise, torch.float32)
    mp, sp, zp = C.posterior(p, feat, action, noise, torch.float32, gen=torch.Generator().manual_seed(5))
    assert torch.equal(m64.float(), m32) and torch.equal(z64.float(), z32) and torch.equal(m32, mp) and torch.equal(z32, zp)
    assert torch.equal(z64[..., :C.Z1], m64)                                        # eps = 0
    _, _, z1u, z2u = R.sample_posterior(p, feat, action, noise)                     # the unrounded fp32 chain
    differ = float((torch.cat([z1u, z2u], -1) != z32).float().mean())
    print("exact data: %.1f %% of z differs from the unrounded chain; z in [%.3f, %.3f]" % (100 * differ, float(z32.min()), float(z32.max())))
    assert differ > 0.9 and float(z32.min()) > 0
    # the prior chain on the same heads
    H = 8
    z0, act = z32[:, 0], torch.cat([action, action[:, :1]], 1)[:, :H]
    eps = torch.zeros(B, H, C.Z)
    a, b, c = (C.prior(p, z0, act, eps, dt, gen=g) for dt, g in ((torch.float64, None), (torch.float32, None),
                                                                 (torch.float32, torch.Generator().manual_seed(6))))
    assert torch.equal(a[0].float(), b[0]) and torch.equal(a[2].float(), b[2]) and torch.equal(b[0], c[0]) and torch.equal(b[2], c[2])


# ---- the cap of the teacher-forced test ----------------------------------------------------------------------------------------------
def test_helper_fp32_runs_leave_at_most_half_the_cap_non_tight():
    """On exactly the inputs of the GPU test (B 33, T 3, A 6, three seeds; 594 (row, MLP) pairs): the helper's fp32 runs in two
    summation orders, teacher-forced on a free fp32 run's z, against its fp64 run on the same z."""
    A, B, T = 6, 33, 3
    p = R.make_params(A)
    loose, miss, n = 0.0, 0, 0
    for seed in SEEDS:
        feat, action, noise = C.random_inputs(B, T, A, seed)
        z = C.posterior(p, feat, action, noise, torch.float32)[2]
        ra, rb = C.hoisted_posterior(p, feat, action, torch.float32)
        ref = C.posterior(p, feat, action, noise, torch.float64, ra=ra, rb=rb, z_given=z)
        for gen in (None, torch.Generator().manual_seed(9 + seed)):
            dev = C.row_deviation(C.posterior(p, feat, action, noise, torch.float32, gen=gen, ra=ra, rb=rb, z_given=z), ref)
            assert dev.numel() == 2 * T * B
            loose, miss, n = max(loose, float(dev.max())), miss + int((dev > TIGHT).sum()), n + dev.numel()
            print("seed %d order %s: %d of %d rows not tight, worst %.3e" % (seed, "permuted" if gen else "plain", int((dev > TIGHT).sum()),
                                                                            dev.numel(), float(dev.max())))
    print("pooled: %.2f %% not tight; the loose bound would be 4 x %.3e" % (100.0 * miss / n, loose))
    assert miss / n <= CAP / 2
    assert 4 * loose < 2e-3                                # below the distance of the bf16 mode from the fp32 chain (2 to 5e-3)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_versioned():
    from s2p_amd import _lib
    header = open(os.path.join(ROOT, "include", "s2p_hip.h")).read()
    for name in (POST, PRIOR):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == 16
        assert _lib.SIGNATURES[name][:6] + _lib.SIGNATURES[name][7:] == _lib.SIGNATURES[name[:-5]][:6] + _lib.SIGNATURES[name[:-5]][7:]
        assert "int %s(" % name in header
    assert "} s2p_chain_mlp_bf16;" in header
    assert "gauss_chain_bf16.hip" in open(os.path.join(ROOT, "s2p_amd", "csrc", "build.sh")).read()
    L = _lib.lib()
    assert hasattr(L, POST) and hasattr(L, PRIOR) and L.s2p_version() == 125
    assert ctypes.sizeof(_lib.ChainMlpBf16) == 6 * 8 + 2 * 4


def _mlps(_lib, k1s, edit=None):
    arr = (_lib.ChainMlpBf16 * len(k1s))(*[_lib.ChainMlpBf16(P, P, P, P, P, P, k, k) for k in k1s])
    if edit is not None:
        g, field, value = edit
        setattr(arr[g], field, value)
    return arr


@pytest.mark.parametrize("name", [POST, PRIOR])
def test_refusals_and_no_ops_without_a_device(name):
    from s2p_amd import _lib
    L = _lib.lib()
    fn, k1s = getattr(L, name), K1 if name == POST else (256, 288)
    last = len(k1s) - 1

    def call(src=P, src_pitch=9 * 256, ra=P, rb=P, eps=P, eps_pitch=288, mlps="ok", mean=P, mean_pitch=32, std=P, std_pitch=32, z=P,
             z_pitch=288, B=4, T=9, edit=None):
        return fn(src, src_pitch, ra, rb, eps, eps_pitch, _mlps(_lib, k1s, edit) if mlps == "ok" else mlps, mean, mean_pitch, std,
                  std_pitch, z, z_pitch, B, T, None)

    assert fn(None, 0, None, None, None, 0, None, None, 0, None, 0, None, 0, 0, 9, None) == 0      # B == 0, T == 0: no pointer is looked at
    assert fn(None, 0, None, None, None, 0, None, None, 0, None, 0, None, 0, 4, 0, None) == 0
    bad = dict(negative_B=dict(B=-1), negative_T=dict(T=-1), null_src=dict(src=None), null_eps=dict(eps=None), null_mlps=dict(mlps=None),
               null_mean=dict(mean=None), null_std=dict(std=None), null_z=dict(z=None), null_ra=dict(ra=None), null_rb=dict(rb=None),
               src_pitch_short=dict(src_pitch=252), eps_pitch_short=dict(eps_pitch=287), mean_pitch_short=dict(mean_pitch=31),
               std_pitch_short=dict(std_pitch=16), z_pitch_short=dict(z_pitch=256), src_misaligned=dict(src=P + 4),
               src_pitch_not_4=dict(src_pitch=9 * 256 + 2), w1_misaligned=dict(edit=(0, "w1", P + 8)), w2_misaligned=dict(edit=(last, "w2", P + 8)),
               w3_misaligned=dict(edit=(last, "w3", P + 2)), w1_row_short=dict(edit=(last, "w1_row", 280)),
               w1_row_not_8=dict(edit=(0, "w1_row", 260)), k1_of_another_head=dict(edit=(last, "k1", 256)), other_k1=dict(edit=(0, "k1", 264)),
               null_bias=dict(edit=(1, "b2", None)), null_weight=dict(edit=(last, "w3", None)))
    for what, kw in bad.items():
        assert call(**kw) != 0, what
        assert name.encode() in L.s2p_last_error(), what
    if name == POST:                                       # T == 1 runs the two init MLPs only: ra / rb and the chain MLPs are not required
        assert call(T=1, ra=None, rb=None, eps=None) != 0 and b"null" in L.s2p_last_error()
        assert call(T=1, ra=None, rb=None, edit=(2, "w1", None), z_pitch=100) != 0 and b"pitch" in L.s2p_last_error()
        assert call(T=1, ra=None, rb=None, edit=(0, "w1", None)) != 0 and b"z1_posterior_init" in L.s2p_last_error()


# ---- the command lines and the keyword ---------------------------------------------------------------------------------------------------
BASES = dict(train_iql=["--real", "r.npz", "--latent_dir", "d", "--steps", "1", "--out", "o"],
             train_cql=["--real", "r.npz", "--latent_dir", "d", "--steps", "1", "--out", "o"],
             evaluate_policy=["--latent_dir", "d", "--policy_dir", "p", "--env", "replay:x.npz"],
             predict_latent=["--data", "x.npz", "--latent_dir", "d", "--out", "o.npz"])


@pytest.mark.parametrize("script", sorted(BASES))
def test_bf16_chain_flag_needs_fused_chain(script, capsys):
    mod, base = __import__(script), BASES[script]
    assert mod.parse_args(base).bf16_chain is False and mod.parse_args(base + ["--fused_chain"]).bf16_chain is False
    a = mod.parse_args(base + ["--fused_chain", "--bf16_chain"])
    assert a.bf16_chain is True and a.fused_chain is True and a.bf16 is False
    if script.startswith("train"):
        assert a.bf16_mlp is False and mod.parse_args(base + ["--fused_chain", "--bf16_chain", "--bf16_mlp"]).bf16_mlp is True
    with pytest.raises(SystemExit):
        mod.parse_args(base + ["--bf16_chain"])
    assert "only in the fused chain kernels" in capsys.readouterr().err


def test_the_attribute_and_the_keyword_default_to_fp32():
    import inspect
    from s2p_amd.slac import LatentModel
    from s2p_amd.slac_algo import SlacAlgorithm
    assert inspect.signature(SlacAlgorithm.__init__).parameters["chain_compute"].default == "fp32"
    assert "chain_compute" not in inspect.signature(LatentModel.__init__).parameters    # the reference's constructor stays
    assert 'self.chain_compute = "fp32"' in inspect.getsource(LatentModel.__init__)
