"""N3k on the host: the two entry points of the posterior chain under grad are exported and declared, refuse bad arguments before any
launch (so without a device), treat B == 0, T == 0 (and, for the backward, T == 1) as no-ops that look at no pointer, and the three
training command lines take --fused_chain_grad."""
import ctypes
import inspect
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, BWD = "s2p_posterior_chain_fwd_save", "s2p_posterior_chain_bwd"
K1 = (256, 32, 256, 288)                               # chain columns of the four first layers
P = 4096                                               # a non-NULL, 16-byte aligned address: refusals happen before any launch
STATE = ("a0_h1", "a0_h2", "a0_raw", "b0_h1", "b0_h2", "b0_raw", "h1a", "h2a", "rawa", "h1b", "h2b", "rawb", "xz")
GRADS = ("drawa", "dh2a", "dh1a", "drawb", "dh2b", "dh1b", "dxz")


def test_symbols_are_exported_declared_and_versioned():
    from s2p_amd import _lib
    assert len(_lib.SIGNATURES[FWD]) == 17 and len(_lib.SIGNATURES[BWD]) == 14
    header = open(os.path.join(ROOT, "include", "s2p_hip.h")).read()
    for text in ("int %s(" % FWD, "int %s(" % BWD, "} s2p_chain_state;", "} s2p_chain_grads;", "} s2p_chain_mlp_bwd;"):
        assert text in header, text
    L = _lib.lib()
    assert hasattr(L, FWD) and hasattr(L, BWD) and L.s2p_version() == 125


def test_struct_sizes_and_fields():
    from s2p_amd import _lib
    assert ctypes.sizeof(_lib.ChainState) == 13 * 8 and tuple(n for n, _ in _lib.ChainState._fields_) == STATE
    assert ctypes.sizeof(_lib.ChainGrads) == 7 * 8 and tuple(n for n, _ in _lib.ChainGrads._fields_) == GRADS
    assert ctypes.sizeof(_lib.ChainMlpBwd) == 3 * 8 + 2 * 4
    assert ctypes.sizeof(_lib.ChainMlp) == 6 * 8 + 2 * 4


def _struct(cls, edit):
    s = cls(*([P] * len(cls._fields_)))
    if edit is not None and edit[0] is cls:
        setattr(s, edit[1], edit[2])
    return s


def test_forward_refusals_and_no_ops_without_a_device():
    from s2p_amd import _lib
    L = _lib.lib()

    def call(feat=P, feat_pitch=9 * 256, ra=P, rb=P, eps=P, eps_pitch=288, mlps="ok", mean=P, mean_pitch=32, std=P, std_pitch=32, z=P,
             z_pitch=288, state="ok", B=4, T=9, edit=None):
        arr = (_lib.ChainMlp * 4)(*[_lib.ChainMlp(P, P, P, P, P, P, k, k) for k in K1])
        if edit is not None and isinstance(edit[0], int):
            setattr(arr[edit[0]], edit[1], edit[2])
        st = ctypes.byref(_struct(_lib.ChainState, edit)) if state == "ok" else state
        return L.s2p_posterior_chain_fwd_save(feat, feat_pitch, ra, rb, eps, eps_pitch, arr if mlps == "ok" else mlps, mean, mean_pitch,
                                              std, std_pitch, z, z_pitch, st, B, T, None)

    none = (None, 0, None, None, None, 0, None, None, 0, None, 0, None, 0, None)
    assert L.s2p_posterior_chain_fwd_save(*none, 0, 9, None) == 0           # B == 0, T == 0: no pointer is looked at
    assert L.s2p_posterior_chain_fwd_save(*none, 4, 0, None) == 0
    S = _lib.ChainState
    bad = dict(negative_B=dict(B=-1), negative_T=dict(T=-1), null_feat=dict(feat=None), null_eps=dict(eps=None), null_mlps=dict(mlps=None),
               null_mean=dict(mean=None), null_std=dict(std=None), null_z=dict(z=None), null_ra=dict(ra=None), null_rb=dict(rb=None),
               feat_pitch_short=dict(feat_pitch=252), eps_pitch_short=dict(eps_pitch=287), mean_pitch_short=dict(mean_pitch=31),
               std_pitch_short=dict(std_pitch=16), z_pitch_short=dict(z_pitch=256), feat_misaligned=dict(feat=P + 4),
               feat_pitch_not_4=dict(feat_pitch=9 * 256 + 2), w1_misaligned=dict(edit=(0, "w1", P + 4)),
               w3_misaligned=dict(edit=(3, "w3", P + 4)), w1_row_short=dict(edit=(3, "w1_row", 284)),
               w1_row_not_4=dict(edit=(1, "w1_row", 34)), other_k1=dict(edit=(2, "k1", 260)), null_bias=dict(edit=(1, "b2", None)),
               null_state=dict(state=None), null_t0_buffer=dict(edit=(S, "b0_raw", None)), null_chain_buffer=dict(edit=(S, "rawb", None)),
               null_xz=dict(edit=(S, "xz", None)), misaligned_t0_buffer=dict(edit=(S, "a0_h1", P + 4)),
               misaligned_chain_buffer=dict(edit=(S, "h2a", P + 8)))
    for name, kw in bad.items():
        assert call(**kw) != 0, name
        assert FWD.encode() in L.s2p_last_error(), name
    # T == 1 saves the two init MLPs only: the chain buffers may be absent, the t = 0 ones may not
    assert call(T=1, ra=None, rb=None, edit=(S, "a0_raw", None)) != 0 and b"state" in L.s2p_last_error()
    assert call(T=1, ra=None, rb=None, eps=None, edit=(S, "rawb", None)) != 0 and b"null" in L.s2p_last_error()


def test_backward_refusals_and_no_ops_without_a_device():
    from s2p_amd import _lib
    L = _lib.lib()

    def call(eps=P, eps_pitch=288, dmean=P, dmean_pitch=32, dstd=P, dstd_pitch=32, dz=P, dz_pitch=288, mlps="ok", state="ok", grads="ok",
             B=4, T=9, edit=None):
        arr = (_lib.ChainMlpBwd * 2)(_lib.ChainMlpBwd(P, P, P, 256, 256), _lib.ChainMlpBwd(P, P, P, 288, 256))
        if edit is not None and isinstance(edit[0], int):
            setattr(arr[edit[0]], edit[1], edit[2])
        st = ctypes.byref(_struct(_lib.ChainState, edit)) if state == "ok" else state
        gr = ctypes.byref(_struct(_lib.ChainGrads, edit)) if grads == "ok" else grads
        return L.s2p_posterior_chain_bwd(eps, eps_pitch, dmean, dmean_pitch, dstd, dstd_pitch, dz, dz_pitch, arr if mlps == "ok" else mlps,
                                         st, gr, B, T, None)

    none = (None, 0, None, 0, None, 0, None, 0, None, None, None)
    for B, T in ((0, 9), (4, 0), (4, 1)):                                   # no batch, no time, no chain step: no pointer is looked at
        assert L.s2p_posterior_chain_bwd(*none, B, T, None) == 0, (B, T)
    S, G = _lib.ChainState, _lib.ChainGrads
    bad = dict(negative_B=dict(B=-1), negative_T=dict(T=-1), null_eps=dict(eps=None), null_dmean=dict(dmean=None),
               null_dstd=dict(dstd=None), null_dz=dict(dz=None), null_mlps=dict(mlps=None), null_state=dict(state=None),
               null_grads=dict(grads=None), eps_pitch_short=dict(eps_pitch=287), dz_pitch_short=dict(dz_pitch=256),
               dmean_pitch_short=dict(dmean_pitch=31), dstd_pitch_short=dict(dstd_pitch=16), k1_of_the_other_head=dict(edit=(0, "k1", 288)),
               other_k1=dict(edit=(1, "k1", 292)), w1t_row_short=dict(edit=(1, "w1t_row", 252)), w1t_row_not_4=dict(edit=(0, "w1t_row", 258)),
               null_w2t=dict(edit=(0, "w2t", None)), w1t_misaligned=dict(edit=(1, "w1t", P + 4)), w3t_misaligned=dict(edit=(0, "w3t", P + 8)),
               null_saved=dict(edit=(S, "rawa", None)), misaligned_saved=dict(edit=(S, "h1b", P + 4)),
               null_output=dict(edit=(G, "dxz", None)), misaligned_output=dict(edit=(G, "drawb", P + 4)))
    for name, kw in bad.items():
        assert call(**kw) != 0, name
        assert BWD.encode() in L.s2p_last_error(), name
    # the t = 0 buffers and xz belong to the launches around the chain: the backward chain does not look at them
    assert call(edit=(S, "a0_h1", None), B=-1) != 0 and b"negative" in L.s2p_last_error()


@pytest.mark.parametrize("script", ["train_latent", "train_iql", "train_cql"])
def test_fused_chain_grad_flag(script):
    mod = __import__(script)
    base = ["--real", "r.npz", "--steps", "1", "--out", "o"] + ([] if script == "train_latent" else ["--latent_dir", "d"])
    assert mod.parse_args(base).fused_chain_grad is False
    assert mod.parse_args(base + ["--fused_chain_grad"]).fused_chain_grad is True
    if script != "train_latent":
        a = mod.parse_args(base + ["--fused_chain_grad"])
        assert not a.fused_chain and not a.freeze_slac and not a.cache_features
        a = mod.parse_args(base + ["--fused_chain", "--freeze_slac", "--cache_features"])
        assert a.fused_chain and a.freeze_slac and a.cache_features and a.fused_chain_grad is False
        a = mod.parse_args(base + ["--fused_chain_grad", "--fused_chain", "--freeze_slac", "--cache_features"])
        assert a.fused_chain_grad and a.fused_chain and a.freeze_slac and a.cache_features


def test_the_attribute_and_the_keyword_default_to_off():
    from s2p_amd.slac import LatentModel
    from s2p_amd.slac_algo import SlacAlgorithm
    assert inspect.signature(SlacAlgorithm.__init__).parameters["fused_chain_grad"].default is False
    assert inspect.signature(SlacAlgorithm.__init__).parameters["fused_chain"].default is False
    names = list(inspect.signature(LatentModel.__init__).parameters)
    assert names == ["self", "state_shape", "action_shape", "feature_dim", "z1_dim", "z2_dim", "hidden_units", "image_size", "dtype",
                     "device"]                                               # the reference's constructor stays
    src = inspect.getsource(LatentModel.__init__)
    assert "self.fused_chain_grad = False" in src and "self.fused_chain = False" in src
