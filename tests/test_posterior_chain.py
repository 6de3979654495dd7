"""N3h on the host: the fused posterior chain's entry point is exported and declared, refuses bad arguments before any launch
(so without a device), treats B == 0 as a no-op that looks at no pointer, and the three command lines take --fused_chain."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "s2p_posterior_chain_fwd"
K1 = (256, 32, 256, 288)                               # chain columns of the four first layers
P = 4096                                               # a non-NULL, 16-byte aligned address: refusals happen before any launch


def test_symbol_is_exported_declared_and_versioned():
    from s2p_amd import _lib
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME]) == 16
    header = open(os.path.join(ROOT, "include", "s2p_hip.h")).read()
    assert "int %s(" % NAME in header and "} s2p_chain_mlp;" in header
    assert "gauss_chain.hip" in open(os.path.join(ROOT, "s2p_amd", "csrc", "build.sh")).read()
    L = _lib.lib()
    assert hasattr(L, NAME) and L.s2p_version() == 125
    assert ctypes.sizeof(_lib.ChainMlp) == 6 * 8 + 2 * 4


def _mlps(_lib, edit=None):
    arr = (_lib.ChainMlp * 4)(*[_lib.ChainMlp(P, P, P, P, P, P, k, k) for k in K1])
    if edit is not None:
        g, field, value = edit
        setattr(arr[g], field, value)
    return arr


def test_refusals_and_the_empty_batch_without_a_device():
    from s2p_amd import _lib
    L = _lib.lib()

    def call(feat=P, feat_pitch=9 * 256, ra=P, rb=P, eps=P, eps_pitch=288, mlps="ok", mean=P, mean_pitch=32, std=P, std_pitch=32, z=P,
             z_pitch=288, B=4, T=9, edit=None):
        return L.s2p_posterior_chain_fwd(feat, feat_pitch, ra, rb, eps, eps_pitch, _mlps(_lib, edit) if mlps == "ok" else mlps, mean,
                                         mean_pitch, std, std_pitch, z, z_pitch, B, T, None)

    # B == 0 (and T == 0): a successful no-op that looks at no pointer
    assert L.s2p_posterior_chain_fwd(None, 0, None, None, None, 0, None, None, 0, None, 0, None, 0, 0, 9, None) == 0
    assert L.s2p_posterior_chain_fwd(None, 0, None, None, None, 0, None, None, 0, None, 0, None, 0, 4, 0, None) == 0
    bad = dict(negative_B=dict(B=-1), negative_T=dict(T=-1), null_feat=dict(feat=None), null_eps=dict(eps=None), null_mlps=dict(mlps=None),
               null_mean=dict(mean=None), null_std=dict(std=None), null_z=dict(z=None), null_ra=dict(ra=None), null_rb=dict(rb=None),
               feat_pitch_short=dict(feat_pitch=252), eps_pitch_short=dict(eps_pitch=287), mean_pitch_short=dict(mean_pitch=31),
               std_pitch_short=dict(std_pitch=16), z_pitch_short=dict(z_pitch=256), feat_misaligned=dict(feat=P + 4),
               feat_pitch_not_4=dict(feat_pitch=9 * 256 + 2), w1_misaligned=dict(edit=(0, "w1", P + 4)), w2_misaligned=dict(edit=(2, "w2", P + 8)),
               w3_misaligned=dict(edit=(3, "w3", P + 4)), w1_row_short=dict(edit=(3, "w1_row", 284)), w1_row_not_4=dict(edit=(1, "w1_row", 34)),
               k1_of_another_head=dict(edit=(3, "k1", 256)),
               other_k1=dict(edit=(2, "k1", 260)), null_bias=dict(edit=(1, "b2", None)), null_chain_weight=dict(edit=(3, "w3", None)))
    for name, kw in bad.items():
        assert call(**kw) != 0, name
        assert NAME.encode() in L.s2p_last_error(), name
    # T == 1 runs the two init MLPs only: ra / rb and the two chain MLPs are not required -- what is refused then is still refused
    assert call(T=1, ra=None, rb=None, eps=None) != 0 and b"null" in L.s2p_last_error()
    assert call(T=1, ra=None, rb=None, edit=(2, "w1", None), z_pitch=100) != 0 and b"pitch" in L.s2p_last_error()
    assert call(T=1, ra=None, rb=None, edit=(0, "w1", None)) != 0 and b"z1_posterior_init" in L.s2p_last_error()


@pytest.mark.parametrize("script", ["train_iql", "train_cql"])
def test_fused_chain_flag_of_the_trainers(script):
    mod = __import__(script)
    base = ["--real", "r.npz", "--latent_dir", "d", "--steps", "1", "--out", "o"]
    assert mod.parse_args(base).fused_chain is False
    assert mod.parse_args(base + ["--fused_chain"]).fused_chain is True
    a = mod.parse_args(base + ["--fused_chain", "--freeze_slac", "--cache_features"])
    assert a.fused_chain and a.freeze_slac and a.cache_features
    assert mod.parse_args(base + ["--freeze_slac"]).fused_chain is False


def test_fused_chain_flag_of_evaluate_policy():
    import evaluate_policy
    base = ["--latent_dir", "d", "--policy_dir", "p", "--env", "replay:x.npz"]
    assert evaluate_policy.parse_args(base).fused_chain is False
    assert evaluate_policy.parse_args(base + ["--fused_chain", "--slac_policy_input_type", "latent_z"]).fused_chain is True


def test_the_attribute_and_the_keyword_default_to_off():
    import inspect
    from s2p_amd.slac import LatentModel
    from s2p_amd.slac_algo import SlacAlgorithm
    assert inspect.signature(SlacAlgorithm.__init__).parameters["fused_chain"].default is False
    assert "fused_chain" not in inspect.signature(LatentModel.__init__).parameters      # the reference's constructor stays
    src = inspect.getsource(LatentModel.__init__)
    assert "self.fused_chain = False" in src
