"""Device-resident SLAC sequence replay buffer (SPEC.md N3c; reference `rlkit/torch/slac/buffer.py:71-206`).

The reference keeps every window's S+1 frames as LazyFrames on the host and assembles a batch with a Python loop, one host array and
one host-to-device copy.  Here every frame is stored ONCE, uint8 NHWC, in a pool on the device; a window is a row of S+1 pool slots
in an int32 table; and one HIP kernel (`ops.window_gather_u8`, csrc/replay.hip) turns sampled window ids straight into what the
latent model reads: the encoder's NHWC input in the compute dtype and the uint8 target of the image loss.

Call surface, return tuples / dict keys, `_n` / `_p` / `_real_n` and the host-side `np.random.randint` draw are the reference's, so
the same `np.random.seed` selects the same windows.  The bookkeeping is host Python and works with device="cpu"; only the `sample_*`
methods in "packed" / "u8" / "float" form need a HIP device (`window_frames` is the plain-torch accessor for any device).

With a frozen encoder a frame's feature is a constant of the run (SPEC.md N3g): `attach_features(encoder)` keeps one 256-float row
per pool slot beside the pool, and `random_batch` / `sample_sac` with frames="features" return a `FeatureBatch` -- features, both
policy-input rows, actions, reward and terminal out of one launch (`ops.feature_window_gather`), no frame touched."""
from collections import deque

import numpy as np
import torch

from . import ops
from ._lib import chunk_elems

_NONE = np.iinfo(np.int64).max


class FrameBatch:
    """Frames of B sampled windows in the two forms the latent model reads: `u8` uint8 [B,S+1,H,W,C] (image-loss target) and
    `nhwc` [B*(S+1),H,W,pitch] = u8 / 255 in the compute dtype, pad channels zero (encoder input).  `shape` is the reference's
    (B,S+1,C,H,W)."""

    def __init__(self, u8, nhwc):
        B, T, H, W, C = u8.shape
        self.u8, self.nhwc, self.shape = u8, nhwc, (B, T, C, H, W)

    @property
    def device(self):
        return self.u8.device

    def __len__(self):
        return self.shape[0]


class FeatureBatch:
    """B sampled windows as cached encoder features (`ReplayBuffer.attach_features`), with everything a step on a frozen latent model
    reads, written by one launch: `feature_` [B,S+1,256], `feature_action` / `next_feature_action` [B,S*256+(S-1)*A] (the two results
    of `create_feature_actions`), `action_` [B,S,A] and `action` [B,A] = action_[:, -1].  `shape` is the reference's (B,S+1,C,H,W),
    as `FrameBatch`; there are no frames in it."""

    def __init__(self, feature_, feature_action, next_feature_action, action_, action, state_shape):
        self.feature_, self.feature_action, self.next_feature_action = feature_, feature_action, next_feature_action
        self.action_, self.action = action_, action
        self.shape = tuple(feature_.shape[:2]) + tuple(state_shape)

    @property
    def device(self):
        return self.feature_.device

    def __len__(self):
        return self.shape[0]


FEATURE_DIM = 256                                 # the encoder's output width: one row of the feature table


def _take(parts, idx):
    """Rows `idx` of the virtual concatenation of the arrays `parts` (no concatenated copy is made)."""
    if len(parts) == 1:
        return np.ascontiguousarray(parts[0][idx])
    out = np.empty((len(idx),) + parts[0].shape[1:], dtype=parts[0].dtype)
    lo = 0
    for p in parts:
        m = (idx >= lo) & (idx < lo + len(p))
        if m.any():
            out[m] = p[idx[m] - lo]
        lo += len(p)
    return out


class ReplayBuffer:
    def __init__(self, buffer_size, num_sequences, state_shape, action_shape, device, dtype=torch.float32, frame_capacity=None,
                 frames="packed"):
        if frames not in ("packed", "u8", "float"):
            raise ValueError("frames is 'packed', 'u8' or 'float'")
        self._n = 0
        self._p = 0
        self._real_n = 0
        self.buffer_size = int(buffer_size)
        self.num_sequences = S = int(num_sequences)
        self.state_shape = tuple(state_shape)
        self.action_shape = tuple(action_shape)
        self.device = torch.device(device)
        self.dtype, self.frames = dtype, frames
        C, H, W = self.state_shape
        if frame_capacity is None:
            # an episode of L steps gives L+1 frames and L-S+1 windows: enough whenever episodes last at least 9*S-1 steps
            frame_capacity = self.buffer_size + self.buffer_size // 8 + (S + 1)
        self.frame_capacity = int(frame_capacity)
        self.pool = torch.empty((self.frame_capacity, H, W, C), dtype=torch.uint8, device=self.device)
        self.table = torch.zeros((self.buffer_size, S + 1), dtype=torch.int32, device=self.device)
        self.action_ = torch.empty(self.buffer_size, S, *self.action_shape, device=self.device)
        self.reward_ = torch.empty(self.buffer_size, S, 1, device=self.device)
        self.done_ = torch.empty(self.buffer_size, S, 1, device=self.device)
        # The pool is a FIFO ring over a running frame count: frame k lives in slot k % frame_capacity, _head counts the frames
        # stored so far, _tail is a lower bound of the oldest frame still referenced, _wmin[i] the oldest frame of window i.
        self._head = 0
        self._tail = 0
        self._wmin = np.full(self.buffer_size, _NONE, dtype=np.int64)
        self._reset_pending()
        # the feature table (attach_features): features[slot] = encoder(pool[slot]); _fhead counts the frames encoded so far, so the
        # frames stored since are [_fhead, _head)
        self.features = None
        self._fhead = 0
        self._feat_encoder, self._feat_chunk, self._feat_version = None, 1024, None

    # ---- cached encoder features (SPEC.md N3g) ---------------------------------------------------------------------------
    @staticmethod
    def _encoder_version(encoder):
        return sum(p._version for p in encoder.parameters())

    def _encode_slots(self, slots):
        """features[slots] = encoder(pool[slots]) for an int64 array of pool slots: one gather over a one-column slot table (the
        encoder's NHWC input, as a sampled FrameBatch holds it) and one run of the conv stack."""
        enc = self._feat_encoder
        where = torch.from_numpy(slots).to(self.device)
        x, _ = ops.window_gather_u8(self.pool, where.to(torch.int32).view(-1, 1), torch.arange(len(slots), device=self.device), enc.dtype,
                                    ops.pad_to(self.state_shape[0], chunk_elems(enc.dtype)), want_u8=False)
        with torch.no_grad():
            y = enc.run(x)
        self.features.index_copy_(0, where, y.reshape(len(slots), -1).float())

    def _encode_frames(self, lo, hi):
        """Encode the frames with running numbers [lo, hi), `_feat_chunk` at a time; frames the ring has overwritten are left out."""
        lo = max(lo, hi - self.frame_capacity)
        for c in range(lo, hi, self._feat_chunk):
            self._encode_slots(np.arange(c, min(c + self._feat_chunk, hi), dtype=np.int64) % self.frame_capacity)
        self._fhead = hi

    def attach_features(self, encoder, chunk=1024):
        """Build the feature table, fp32 [frame_capacity, 256], from every live frame, `chunk` frames a launch.  The table is valid
        while the encoder's parameters stay as they are (`freeze_slac`); frames stored later are encoded before the next sample."""
        if chunk < 1:
            raise ValueError("chunk >= 1")
        self._feat_encoder, self._feat_chunk = encoder, int(chunk)
        self.features = torch.zeros((self.frame_capacity, FEATURE_DIM), dtype=torch.float32, device=self.device)
        self.refresh_features()

    def refresh_features(self):
        """Re-encode every live frame with the encoder as it is now."""
        if self.features is None:
            raise RuntimeError("no feature table: call attach_features(encoder) first")
        self._feat_version = self._encoder_version(self._feat_encoder)
        self._encode_frames(self._tail, self._head)

    def detach_features(self):
        self.features, self._feat_encoder, self._feat_version = None, None, None

    def _features(self, idxes):
        """-> (FeatureBatch, action_ [B,S,A], reward [B,1], terminal [B,1]) of the windows `idxes`: one id upload, one launch."""
        if self.features is None:
            raise RuntimeError("frames='features' needs a feature table: call attach_features(encoder) first")
        if self._encoder_version(self._feat_encoder) != self._feat_version:
            raise RuntimeError("the encoder's parameters changed since the feature table was built (the cache is for a frozen latent "
                               "model): call refresh_features(), or sample frames")
        if self._fhead < self._head:
            self._encode_frames(self._fhead, self._head)
        if self.device.type != "cuda":
            raise RuntimeError("sampling features runs on a HIP device only (no CPU fallback)")
        win = torch.from_numpy(np.ascontiguousarray(idxes, dtype=np.int64)).to(self.device)
        feature_, fa, next_fa, action_, action, reward, terminal = ops.feature_window_gather(
            self.features, self.table, win, self.action_, self.reward_, self.done_)
        return FeatureBatch(feature_, fa, next_fa, action_, action, self.state_shape), action_, reward, terminal

    # ---- frame ring ------------------------------------------------------------------------------------------------------
    def _reset_pending(self):
        S = self.num_sequences
        self._in_episode = False
        self._pf = deque(maxlen=S + 1)            # running frame numbers of the pending episode's last S+1 frames
        self._pa, self._pr, self._pd = deque(maxlen=S), deque(maxlen=S), deque(maxlen=S)

    def _reserve(self, n, dying=None):
        """Room for n more frames, or RuntimeError with nothing changed.  `dying`: window positions about to be overwritten."""
        if self._head + n - self._tail > self.frame_capacity:
            m = self._wmin
            if dying is not None and len(dying):
                m = m.copy()
                m[dying] = _NONE
            tail = min(int(m.min()), self._pf[0] if self._pf else _NONE, self._head)
            if self._head + n - tail > self.frame_capacity:
                raise RuntimeError(
                    "replay frame pool exhausted: %d frames are still referenced and %d more are needed, frame_capacity=%d; pass a "
                    "larger frame_capacity (short episodes store more frames per window)" % (self._head - tail, n, self.frame_capacity))
            if dying is None or not len(dying):
                self._tail = tail                 # (with `dying`, the caller overwrites those windows next: the bound stays valid)

    def _store_frame(self, state, dying=None):
        state = np.asarray(state)
        if state.shape != self.state_shape or state.dtype != np.uint8:
            raise ValueError("a frame is uint8 %s (CHW), got %s %s" % (self.state_shape, state.dtype, state.shape))
        self._reserve(1, dying)
        k = self._head
        self.pool[k % self.frame_capacity].copy_(torch.from_numpy(np.ascontiguousarray(state.transpose(1, 2, 0))))
        self._head += 1
        return k

    # ---- the reference's step-wise surface (buffer.py:98-125) ------------------------------------------------------------
    def reset_episode(self, state):
        assert not self._in_episode
        k = self._store_frame(state)
        self._in_episode = True
        self._pf.append(k)

    def append(self, action, reward, done, next_state, episode_done):
        assert self._in_episode
        S = self.num_sequences
        completes = len(self._pr) + 1 >= S
        dying = np.array([self._p]) if completes and self._n == self.buffer_size else None
        k = self._store_frame(next_state, dying)
        self._pa.append(np.asarray(action, dtype=np.float32))
        self._pr.append([reward])
        self._pd.append([done])
        self._pf.append(k)
        if completes:
            p = self._p
            slots = np.array(self._pf, dtype=np.int64)
            self.table[p].copy_(torch.from_numpy((slots % self.frame_capacity).astype(np.int32)))
            self.action_[p].copy_(torch.from_numpy(np.array(self._pa, dtype=np.float32)))
            self.reward_[p].copy_(torch.from_numpy(np.array(self._pr, dtype=np.float32)))
            self.done_[p].copy_(torch.from_numpy(np.array(self._pd, dtype=np.float32)))
            self._wmin[p] = slots.min()
            self._n = min(self._n + 1, self.buffer_size)
            self._p = (self._p + 1) % self.buffer_size
        if episode_done:
            self._reset_pending()

    # ---- bulk loading ----------------------------------------------------------------------------------------------------
    def load_windows(self, frames_u8_nhwc, slots, actions, rewards, dones):
        """Append W windows at once.  `frames_u8_nhwc`: uint8 [F,H,W,C] (or a tuple of such arrays, read as their concatenation);
        `slots` [W,S+1] index into it.  Only the frames that a surviving window references are stored (each once, in order, in one
        copy); windows follow the ring rule of `_append` (W > buffer_size keeps the last buffer_size).  A pending episode is
        dropped, as the reference loader's `buff.reset()` does.  On any error nothing is changed."""
        parts = tuple(frames_u8_nhwc) if isinstance(frames_u8_nhwc, (tuple, list)) else (frames_u8_nhwc,)
        S, C = self.num_sequences, self.state_shape[0]
        H, W_ = self.state_shape[1:]
        for p in parts:
            if p.dtype != np.uint8 or p.shape[1:] != (H, W_, C):
                raise ValueError("frames are uint8 [F,%d,%d,%d] (NHWC), got %s %s" % (H, W_, C, p.dtype, p.shape))
        F = sum(len(p) for p in parts)
        slots = np.asarray(slots, dtype=np.int64)
        W = len(slots)
        if slots.ndim != 2 or slots.shape[1] != S + 1:
            raise ValueError("slots is [W,%d]" % (S + 1))
        if W and (slots.min() < 0 or slots.max() >= F):
            raise IndexError("window slots must lie in [0, %d): got [%d, %d]" % (F, slots.min(), slots.max()))
        actions = np.asarray(actions, dtype=np.float32).reshape(W, S, *self.action_shape)
        rewards = np.asarray(rewards, dtype=np.float32).reshape(W, S, 1)
        dones = np.asarray(dones, dtype=np.float32).reshape(W, S, 1)
        if W == 0:
            self._reset_pending()
            return
        keep = min(W, self.buffer_size)
        pos = (self._p + np.arange(W - keep, W)) % self.buffer_size          # ring positions of the surviving windows
        uniq, inv = np.unique(slots[W - keep:], return_inverse=True)
        pending, self._pf = self._pf, deque()                                 # the pending episode no longer holds frames
        try:
            self._reserve(len(uniq), pos[self._wmin[pos] != _NONE])
        except RuntimeError:
            self._pf = pending
            raise
        self._reset_pending()
        dev = self.device
        num = self._head + inv.reshape(keep, S + 1).astype(np.int64)         # running frame numbers
        where = torch.from_numpy((self._head + np.arange(len(uniq))) % self.frame_capacity).to(dev)
        self.pool.index_copy_(0, where, torch.from_numpy(_take(parts, uniq)).to(dev))
        tpos = torch.from_numpy(pos).to(dev)
        self.table.index_copy_(0, tpos, torch.from_numpy((num % self.frame_capacity).astype(np.int32)).to(dev))
        self.action_.index_copy_(0, tpos, torch.from_numpy(actions[W - keep:]).to(dev))
        self.reward_.index_copy_(0, tpos, torch.from_numpy(rewards[W - keep:]).to(dev))
        self.done_.index_copy_(0, tpos, torch.from_numpy(dones[W - keep:]).to(dev))
        self._wmin[pos] = num.min(axis=1)
        self._head += len(uniq)
        self._n = min(self._n + W, self.buffer_size)
        self._p = (self._p + W) % self.buffer_size

    # ---- sampling (buffer.py:127-167) ------------------------------------------------------------------------------------
    def _idxes(self, batch_size, idxes):
        if idxes is None:
            return np.random.randint(low=0, high=self._n, size=batch_size)
        idxes = np.asarray(idxes, dtype=np.int64).reshape(-1)
        if len(idxes) and (idxes.min() < 0 or idxes.max() >= self._n):
            raise IndexError("window ids must lie in [0, %d)" % self._n)
        return idxes

    def window_frames(self, idxes):
        """uint8 [len,S+1,H,W,C] by plain torch indexing, on any device: the debugging accessor and the kernel's oracle."""
        idxes = self._idxes(None, idxes)
        rows = self.table[torch.from_numpy(idxes).to(self.device)].long()
        return self.pool[rows]

    def _state(self, idxes, frames):
        frames = self.frames if frames is None else frames
        if self.device.type != "cuda":
            raise RuntimeError("sampling frames runs on a HIP device only (no CPU fallback); window_frames() works anywhere")
        win = torch.from_numpy(np.ascontiguousarray(idxes, dtype=np.int64)).to(self.device)
        C = self.state_shape[0]
        if frames == "packed":
            x, u8 = ops.window_gather_u8(self.pool, self.table, win, self.dtype, ops.pad_to(C, chunk_elems(self.dtype)))
            return FrameBatch(u8, x)
        if frames == "u8":
            return ops.window_gather_u8(self.pool, self.table, win, self.dtype, want_x=False)[1]
        if frames == "float":                     # the reference's fp32 [B,S+1,C,H,W] = u8 / 255
            x, _ = ops.window_gather_u8(self.pool, self.table, win, torch.float32, ops.pad_to(C, 4), want_u8=False)
            return ops.nhwc_to_nchw(x, C).reshape(len(idxes), self.num_sequences + 1, *self.state_shape)
        raise ValueError("frames is 'packed', 'u8' or 'float'")

    def sample_latent(self, batch_size, idxes=None, frames=None):
        if frames == "features":
            raise ValueError("sample_latent trains the latent model, whose image loss needs the frames: frames='features' is for "
                             "sample_sac / random_batch")
        idxes = self._idxes(batch_size, idxes)
        state_ = self._state(idxes, frames)
        return state_, self.action_[idxes], self.reward_[idxes], self.done_[idxes]

    def sample_sac(self, batch_size, idxes=None, frames=None):
        idxes = self._idxes(batch_size, idxes)
        if frames == "features":
            return self._features(idxes)
        state_ = self._state(idxes, frames)
        return state_, self.action_[idxes], self.reward_[idxes, -1], self.done_[idxes, -1]

    def random_batch(self, batch_size, idxes=None, frames=None):
        idxes = self._idxes(batch_size, idxes)
        if frames == "features":                  # the cached features of a frozen encoder: observations is a FeatureBatch
            state_, actions, rewards, terminals = self._features(idxes)
            return dict(observations=state_, actions=actions, rewards=rewards, terminals=terminals)
        state_ = self._state(idxes, frames)
        return dict(observations=state_, actions=self.action_[idxes], rewards=self.reward_[idxes, -1],
                    terminals=self.done_[idxes, -1])

    def __len__(self):
        return self._n

    def get_diagnostics(self):
        return {}

    def get_snapshot(self):
        return {}

    def end_epoch(self, epoch):
        return
