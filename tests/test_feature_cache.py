"""N3g on the host: the command-line flag, the refusals of `frames="features"`, the pending-frame bookkeeping of the feature table
on a device="cpu" buffer (the encode step replaced by a recorder), and the new entry point's declaration and argument checks, which
refuse before any launch."""
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, A, CAP = 2, 2, 10
BASE = ["--real", "r.npz", "--latent_dir", "d", "--steps", "1", "--out", "o"]


@pytest.mark.parametrize("script", ["train_iql", "train_cql"])
def test_cache_features_needs_freeze_slac(script, capsys):
    mod = __import__(script)
    with pytest.raises(SystemExit) as e:
        mod.parse_args(BASE + ["--cache_features"])
    assert e.value.code == 2 and "--freeze_slac" in capsys.readouterr().err
    a = mod.parse_args(BASE + ["--cache_features", "--freeze_slac"])
    assert a.cache_features and a.freeze_slac
    assert not mod.parse_args(BASE + ["--freeze_slac"]).cache_features


def _frame(r):
    return r.randint(0, 256, size=(3, 4, 4)).astype(np.uint8)


def _buffer():
    from s2p_amd.slac_buffer import ReplayBuffer
    return ReplayBuffer(4, S, (3, 4, 4), (A,), "cpu", frame_capacity=CAP)


def _episode(buf, r, steps):
    buf.reset_episode(_frame(r))
    for t in range(steps):
        buf.append(r.uniform(-1, 1, A).astype(np.float32), 0.0, False, _frame(r), t == steps - 1)


def _recorded(buf):
    calls = []
    buf._encode_slots = lambda slots: calls.append([int(s) for s in slots])
    return calls


def test_features_without_a_table_and_for_the_latent_loss_are_refused():
    buf = _buffer()
    _episode(buf, np.random.RandomState(0), 3)
    with pytest.raises(RuntimeError, match="attach_features"):
        buf.random_batch(2, frames="features")
    with pytest.raises(RuntimeError, match="attach_features"):
        buf.sample_sac(2, frames="features")
    with pytest.raises(RuntimeError, match="attach_features"):
        buf.refresh_features()
    with pytest.raises(ValueError, match="image loss"):
        buf.sample_latent(2, frames="features")
    calls = _recorded(buf)
    buf.attach_features(types.SimpleNamespace(parameters=lambda: []))
    with pytest.raises(ValueError, match="image loss"):
        buf.sample_latent(2, frames="features")
    buf.detach_features()
    assert buf.features is None and calls == [[0, 1, 2, 3]]
    with pytest.raises(RuntimeError, match="attach_features"):
        buf.random_batch(2, frames="features")


def test_pending_frames_across_a_ring_wrap_and_a_bulk_load():
    """Frame k lives in slot k % frame_capacity; the build encodes [_tail, _head), a feature sample first encodes what was stored
    since, [_fhead, _head), `chunk` frames a call -- slots the ring has reused included."""
    r = np.random.RandomState(1)
    buf = _buffer()
    _episode(buf, r, 3)                                              # frames 0..3
    calls = _recorded(buf)
    enc = torch.nn.Linear(2, 2)
    buf.attach_features(enc, chunk=3)
    assert calls == [[0, 1, 2], [3]] and buf._fhead == buf._head == 4
    assert tuple(buf.features.shape) == (CAP, 256) and buf.features.dtype == torch.float32
    del calls[:]
    _episode(buf, r, 7)                                              # frames 4..11: 10 and 11 reuse the slots 0 and 1
    assert buf._head == 12 and buf._fhead == 4 and calls == []       # lazily: nothing is encoded before a feature sample
    with pytest.raises(RuntimeError, match="HIP device"):            # (the pending frames are encoded, then the launch needs a device)
        buf.random_batch(2, frames="features")
    assert calls == [[4, 5, 6], [7, 8, 9], [0, 1]] and buf._fhead == 12
    del calls[:]
    with pytest.raises(RuntimeError, match="HIP device"):
        buf.random_batch(2, frames="features")
    assert calls == []                                               # nothing pending: nothing encoded again
    frames = r.randint(0, 256, size=(6, 4, 4, 3)).astype(np.uint8)
    buf.load_windows(frames, np.array([[0, 1, 2], [2, 3, 5]]), r.randn(2, S, A), r.randn(2, S), np.zeros((2, S)))
    assert buf._head == 17 and calls == []                           # five referenced frames stored: 12..16
    with pytest.raises(RuntimeError, match="HIP device"):
        buf.sample_sac(2, frames="features")
    assert calls == [[2, 3, 4], [5, 6]] and buf._fhead == 17
    # staleness is host bookkeeping too: a changed encoder parameter is refused before anything is encoded or returned
    del calls[:]
    with torch.no_grad():
        enc.weight.add_(1.0)
    buf.reset_episode(_frame(r))                                     # one pending frame, 17
    with pytest.raises(RuntimeError, match=r"refresh_features\(\)"):
        buf.random_batch(2, frames="features")
    assert calls == []
    buf.refresh_features()                                           # every live frame again, ring-clipped
    assert [s for c in calls for s in c] == [k % CAP for k in range(max(buf._tail, buf._head - CAP), buf._head)] and buf._fhead == buf._head


def test_entry_point_is_declared_and_refuses_bad_arguments_without_a_device():
    from s2p_amd import _lib
    assert "s2p_feature_window_gather" in _lib.SIGNATURES and len(_lib.SIGNATURES["s2p_feature_window_gather"]) == 22
    assert "int s2p_feature_window_gather(" in open(os.path.join(ROOT, "include", "s2p_hip.h")).read()
    L = _lib.lib()
    p = 4096                                        # a non-NULL, 16-byte aligned address: refusals happen before any launch

    def call(feat=p, F=8, feat_pitch=8, T=3, B=2, A=2, feature_=p, fa=p, next_fa=p, fa_pitch=20, action_=p, alp=2, action_last=p):
        return L.s2p_feature_window_gather(feat, 5, feat_pitch, F, p, T, p, B, action_, p, p, A, feature_, fa, next_fa, fa_pitch, p,
                                           action_last, alp, p, p, None)
    assert call(B=0) == 0 and call(T=0) == 0                         # B * T == 0: a successful no-op, no pointer is looked at
    bad = dict(F_not_4=dict(F=6), feat_pitch_not_4=dict(feat_pitch=10), feat_pitch_below_F=dict(feat_pitch=4), T_1=dict(T=1),
               fa_pitch_small=dict(fa_pitch=16), fa_pitch_not_4=dict(fa_pitch=22), feat_misaligned=dict(feat=p + 4),
               feature_misaligned=dict(feature_=p + 8), fa_misaligned=dict(fa=p + 4), next_fa_misaligned=dict(next_fa=p + 4),
               null_feat=dict(feat=None), null_action=dict(action_=None), action_last_pitch_small=dict(alp=1), negative=dict(A=-1))
    for name, kw in bad.items():
        assert call(**kw) != 0, name
        assert b"s2p_feature_window_gather" in L.s2p_last_error(), name
    assert L.s2p_feature_window_gather(p, 5, 8, 8, p, 3, p, 2, p, p, p, 2, None, None, None, 20, None, None, 2, None, None, None) != 0
    assert b"null" in L.s2p_last_error()
