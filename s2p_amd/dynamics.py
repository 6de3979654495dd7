"""Ensemble state-dynamics forward: the step that produces the predicted next states the
generator consumes.  Mirrors the reference interface `EnsembleTransition(obs_dim, action_dim, hidden_features,
hidden_layers, ensemble_size)` / `model(obs_action) -> Normal(mean, std)` (gaussian_ensemble.py:60-96) and the
per-batch post-processing of state_transition_rollout.py:180-204, running on HIP kernels:

  * the E members are ONE grouped 1x1 "conv" per layer on the exact-fp32 MFMA path (groups = E, the first layer reads
    the same input for every group via x_gstride = 0), Swish fused in the epilogue;
  * one fused head kernel does soft-clamp + exp, the 'local'-mode residual, member pick + de-normalisation and the
    disagreement / aleatoric reductions (s2p_ensemble_head).
The rollout of a whole dataset (SPEC.md N2c) is `rollout_sweep`: one s2p_transition_pack launch for the input of every row, then the
grouped fp32 layers and the head per chunk of rows, writing into dataset-long outputs.
Training (SPEC.md N2b): the parameters live in ONE flat fp32 buffer in the packed layout the forward consumes, beside flat
gradient / Adam-moment buffers of the same layout, so an optimizer step is one s2p_adam_step_dev launch.  A train step is
4 grouped linear forwards that keep the pre-activations, 1 fused NLL head, 4 grouped linear backwards, 1 Adam
(csrc/ensemble_train.hip).  No CPU fallback.
"""
import ctypes
import math

import torch

from . import ops
from ._lib import ACT_NONE, ACT_SWISH, check, lib, ptr, stream
from .ops import ConvGeom, pad_to


class EnsembleTransition:
    def __init__(self, obs_dim, action_dim, hidden_features, hidden_layers, ensemble_size=7, device="cuda:0"):
        self.obs_dim, self.action_dim, self.hidden, self.n_hidden, self.E = obs_dim, action_dim, hidden_features, hidden_layers, ensemble_size
        self.D = obs_dim + 1
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("EnsembleTransition (HIP) needs a HIP device: there is no CPU fallback")
        self.layers = None

    # ---- parameters: one flat buffer [W0 | b0 | ... | W_out | b_out | max_logstd | min_logstd], every range a multiple of 4 floats -
    def _names(self):
        return [f"backbones.{i}" for i in range(self.n_hidden)] + ["output_layer"]

    def _allocate(self, dims):
        """dims: [(in, out)] per layer.  Builds the flat buffers and the per-layer views."""
        E, dev = self.E, self.device
        self._dims, self._off, n = dims, [], 0
        for cin, cout in dims:
            kp = pad_to(cin, 4)
            assert cout % 4 == 0, "layer widths must be multiples of 4"
            self._off.append((n, n + E * cout * kp, kp))
            n += E * cout * kp + E * cout
        self._off_bounds = (n, n + pad_to(self.D, 4))
        self._n = n + 2 * pad_to(self.D, 4)
        self._flat = torch.zeros(self._n, dtype=torch.float32, device=dev)
        self._saved = torch.zeros(self._n, dtype=torch.float32, device=dev)
        self._grad = None
        self.layers = []
        for li, ((cin, cout), (ow, ob, kp)) in enumerate(zip(dims, self._off)):
            geom = ConvGeom(cin, cout, 1, groups=E, x_gstride=0 if li == 0 else cin, y_gstride=cout)
            self.layers.append((geom, self._flat[ow:ob].view(E, cout, 1, kp), self._flat[ob:ob + E * cout], kp))
        self.max_logstd = self._flat[self._off_bounds[0]:self._off_bounds[0] + self.D]
        self.min_logstd = self._flat[self._off_bounds[1]:self._off_bounds[1] + self.D]
        self.select = list(range(E))
        self._buf = {}

    def _wb(self, flat, li):
        (cin, cout), (ow, ob, kp) = self._dims[li], self._off[li]
        return flat[ow:ob].view(self.E, cout, kp), flat[ob:ob + self.E * cout].view(self.E, cout)

    def _put(self, flat, li, w, b):
        """reference layout weight [E, in, out], bias [E, 1, out] -> packed [E][out][in_pad], [E][out]"""
        wv, bv = self._wb(flat, li)
        wv[:, :, :w.shape[1]] = w.to(self.device, torch.float32).permute(0, 2, 1)
        bv.copy_(b.to(self.device, torch.float32).reshape(self.E, -1))

    def _get(self, flat, li):
        wv, bv = self._wb(flat, li)
        return wv[:, :, :self._dims[li][0]].permute(0, 2, 1).contiguous(), bv.reshape(self.E, 1, -1).clone()

    def load_state_dict(self, sd):
        """Reference layout: weight [E, in, out], bias [E, 1, out] (gaussian_ensemble.py:27-28).  saved_* are kept when present,
        else set to copies of the live parameters."""
        names = self._names()
        dims = []
        for name in names:
            w = torch.as_tensor(sd[name + ".weight"])
            assert w.shape[0] == self.E, "ensemble size mismatch"
            dims.append((int(w.shape[1]), int(w.shape[2])))
        assert dims[-1][1] == 2 * self.D
        self._allocate(dims)
        with torch.no_grad():
            for li, name in enumerate(names):
                w, b = torch.as_tensor(sd[name + ".weight"]), torch.as_tensor(sd[name + ".bias"])
                self._put(self._flat, li, w, b)
                self._put(self._saved, li, torch.as_tensor(sd.get(name + ".saved_weight", w)), torch.as_tensor(sd.get(name + ".saved_bias", b)))
            self.max_logstd.copy_(torch.as_tensor(sd["max_logstd"], dtype=torch.float32))
            self.min_logstd.copy_(torch.as_tensor(sd["min_logstd"], dtype=torch.float32))
        return self

    def init_parameters(self, seed=0):
        """The reference init (gaussian_ensemble.py:27-33, 80-81): truncated normal (std 1 / (2 sqrt(in)), cut at +-2), zero
        biases, bounds +1 / -5, saved_* = copies."""
        g = torch.Generator().manual_seed(seed)
        n_in = self.obs_dim + self.action_dim
        dims = [(n_in if i == 0 else self.hidden, self.hidden) for i in range(self.n_hidden)] + [(self.hidden, 2 * self.D)]
        sd = {"max_logstd": torch.ones(self.D), "min_logstd": -5.0 * torch.ones(self.D)}
        for name, (cin, cout) in zip(self._names(), dims):
            w = torch.empty(self.E, cin, cout)
            torch.nn.init.trunc_normal_(w, std=1 / (2 * cin ** 0.5), generator=g)
            sd[name + ".weight"], sd[name + ".bias"] = w, torch.zeros(self.E, 1, cout)
        return self.load_state_dict(sd)

    def state_dict(self):
        """The reference's 18 keys (for 3 hidden layers), in its order and shapes, on the CPU."""
        sd = {"max_logstd": self.max_logstd.detach().cpu().clone(), "min_logstd": self.min_logstd.detach().cpu().clone()}
        for li, name in enumerate(self._names()):
            w, b = self._get(self._flat, li)
            sw, sb = self._get(self._saved, li)
            sd[name + ".weight"], sd[name + ".bias"] = w.cpu(), b.cpu()
            sd[name + ".saved_weight"], sd[name + ".saved_bias"] = sw.cpu(), sb.cpu()
        return sd

    def set_select(self, indexes):
        """gaussian_ensemble.py:50-54, 98-101: forward and training run over these members, restored from their saved copies."""
        indexes = [int(i) for i in indexes]
        assert 0 < len(indexes) <= self.E and max(indexes) < self.E and min(indexes) >= 0
        self.select = indexes
        with torch.no_grad():
            for li in range(len(self._dims)):
                for live, saved in zip(self._wb(self._flat, li), self._wb(self._saved, li)):
                    live[indexes] = saved[indexes]
            if self._grad is not None:
                self._grad.zero_()               # the backward overwrites the selected members' slots only

    def update_save(self, indexes):
        indexes = [int(i) for i in indexes]
        with torch.no_grad():
            for li in range(len(self._dims)):
                for live, saved in zip(self._wb(self._flat, li), self._wb(self._saved, li)):
                    saved[indexes] = live[indexes]

    # ---- training path (csrc/ensemble_train.hip) ----------------------------------------------------------------------------
    def _member(self):
        return (ctypes.c_int32 * len(self.select))(*self.select)

    def _pack_input(self, obs_action, target=None):
        """-> (x [B][kp] or [G][B][kp] zero-padded, its group stride, B, target, its group stride)"""
        G, kp = len(self.select), self._off[0][2]
        x = obs_action.to(self.device, torch.float32)
        assert x.dim() in (2, 3) and x.shape[-1] == self._dims[0][0], "obs_action: [B, in] or [len(select), B, in]"
        assert x.dim() == 2 or x.shape[0] == G, "a 3-D input has one batch per selected member"
        B = x.shape[-2]
        xp = torch.zeros(x.shape[:-1] + (kp,), dtype=torch.float32, device=self.device)
        xp[..., :x.shape[-1]] = x
        t, tg = None, 0
        if target is not None:
            t = target.to(self.device, torch.float32).contiguous()
            assert t.shape[-2:] == (B, self.D) and (t.dim() == 2 or t.shape[0] == G), "target: [B, D] or [len(select), B, D]"
            tg = B * self.D if t.dim() == 3 else 0
        return xp, (B * kp if x.dim() == 3 else 0), B, t, tg

    def _buffers(self, B, G):
        key = (B, G)
        if key not in self._buf:
            dev, f = self.device, torch.float32
            widths = [cout for _, cout in self._dims]
            self._buf[key] = dict(pre=[torch.empty(B, G * n, dtype=f, device=dev) for n in widths],
                                   act=[torch.empty(B, G * n, dtype=f, device=dev) for n in widths[:-1]],
                                   dpre=[torch.empty(B, G * n, dtype=f, device=dev) for n in widths],
                                   sums=torch.empty(2 * G, dtype=f, device=dev), loss=torch.empty(1, dtype=f, device=dev))
        return self._buf[key]

    def _forward_train(self, x, xg, B, keep_pre):
        """The grouped linear chain over the selected members; returns the buffers (raw = pre[-1])."""
        G, E = len(self.select), self.E
        buf, mem, L = self._buffers(B, G), self._member(), lib()
        h, hg, hp = x, xg, x.shape[-1]
        for li, ((cin, cout), (geom, w, b, kp)) in enumerate(zip(self._dims, self.layers)):
            last = li == len(self.layers) - 1
            check(L.s2p_ensemble_linear_fwd(ptr(h), hg, hp, ptr(w), ptr(b), mem, G, E, B, kp, cout,
                                            ptr(buf["pre"][li]) if (keep_pre or last) else None,
                                            None if last else ptr(buf["act"][li]), G * cout, stream()), "s2p_ensemble_linear_fwd")
            if not last:
                h, hg, hp = buf["act"][li], cout, G * cout
        return buf

    def _head(self, buf, x, xg, t, tg, B, grad, mean=None, std=None):
        G, D = len(self.select), self.D
        gb = self._grad[self._off_bounds[0]:] if grad else None
        dmax = gb[:D] if grad else None
        dmin = gb[self._off_bounds[1] - self._off_bounds[0]:][:D] if grad else None
        has_t = t is not None
        check(lib().s2p_ensemble_nll(ptr(buf["pre"][-1]), G * 2 * D, ptr(x), xg, x.shape[-1], ptr(t), tg, D, B, G, D,
                                     ptr(self.min_logstd), ptr(self.max_logstd), 1.0 / (G * B * D), 0.01 / D,
                                     ptr(buf["sums"]) if has_t else None, ptr(buf["loss"]) if has_t else None,
                                     ptr(buf["dpre"][-1]) if grad else None, G * 2 * D, ptr(dmin), ptr(dmax), ptr(mean), ptr(std),
                                     stream()), "s2p_ensemble_nll")

    def _backward(self, buf, x, xg, B):
        G, E, mem, L = len(self.select), self.E, self._member(), lib()
        for li in range(len(self.layers) - 1, -1, -1):
            (cin, cout), (ow, ob, kp) = self._dims[li], self._off[li]
            xin, xig, xip = (x, xg, x.shape[-1]) if li == 0 else (buf["act"][li - 1], kp, G * kp)
            check(L.s2p_ensemble_linear_bwd(ptr(xin), xig, xip, ptr(buf["dpre"][li]), G * cout, ptr(self.layers[li][1]), mem, G, E, B,
                                            kp, cout, ptr(self._grad[ow:ob]), ptr(self._grad[ob:ob + E * cout]),
                                            ptr(buf["pre"][li - 1]) if li else None, ptr(buf["dpre"][li - 1]) if li else None,
                                            G * kp, stream()), "s2p_ensemble_linear_bwd")

    def _loss_backward(self, obs_action, target):
        """forward + head + backward into the flat gradient buffer (9 library launches); returns the buffers."""
        if self._grad is None:
            self._grad = torch.zeros(self._n, dtype=torch.float32, device=self.device)
        x, xg, B, t, tg = self._pack_input(obs_action, target)
        buf = self._forward_train(x, xg, B, keep_pre=True)
        self._head(buf, x, xg, t, tg, B, grad=True)
        self._backward(buf, x, xg, B)
        return buf, B

    @torch.no_grad()
    def loss_and_grad(self, obs_action, target):
        """obs_action [B, in] (shared) or [len(select), B, in]; target [B, D] or [len(select), B, D].  Returns (loss,
        nll_per_member [G], mse_per_member [G], grads: reference name -> tensor in the reference layout; zero for unselected
        members, no entry for saved_*)."""
        buf, B = self._loss_backward(obs_action, target)
        G = len(self.select)
        sums = buf["sums"].clone() / (B * self.D)
        grads = {"max_logstd": self._grad[self._off_bounds[0]:][:self.D].clone(),
                 "min_logstd": self._grad[self._off_bounds[1]:][:self.D].clone()}
        for li, name in enumerate(self._names()):
            grads[name + ".weight"], grads[name + ".bias"] = self._get(self._grad, li)
        return buf["loss"][0].clone(), sums[:G], sums[G:], grads

    def _raw(self, obs_action):
        B = obs_action.shape[0]
        xin_pitch = self.layers[0][3]
        x = torch.zeros((B, 1, 1, xin_pitch), dtype=torch.float32, device=self.device)
        x[:, 0, 0, :obs_action.shape[1]] = obs_action.to(self.device, torch.float32)
        h = x
        for li, (geom, w, b, cin_pad) in enumerate(self.layers):
            last = li == len(self.layers) - 1
            h = ops.conv_fwd(geom, h, w, b, cin_pad, y_pitch=self.E * geom.cout, act=ACT_NONE if last else ACT_SWISH)
        return x, h

    @torch.no_grad()
    def forward(self, obs_action):
        """obs_action: fp32 [B, obs_dim+action_dim] (normalised), or [len(select), B, in] with one batch per selected member.
        Returns (mean [G,B,D], std [G,B,D]) over the G selected members (all E by default)."""
        if obs_action.dim() == 3 or len(self.select) != self.E:
            x, xg, B, _, _ = self._pack_input(obs_action)
            buf = self._forward_train(x, xg, B, keep_pre=False)
            mean = torch.empty((len(self.select), B, self.D), dtype=torch.float32, device=self.device)
            std = torch.empty_like(mean)
            self._head(buf, x, xg, None, 0, B, grad=False, mean=mean, std=std)
            return mean, std
        x, raw = self._raw(obs_action)
        B = x.shape[0]
        mean = torch.empty((self.E, B, self.D), dtype=torch.float32, device=self.device)
        std = torch.empty_like(mean)
        check(lib().s2p_ensemble_head(ptr(raw), raw.shape[3], ptr(x), x.shape[3], B, self.E, self.D, ptr(self.min_logstd),
                                      ptr(self.max_logstd), ptr(mean), ptr(std), None, None, None, 0.0, 1.0, None, None,
                                      None, None, stream()), "s2p_ensemble_head")
        return mean, std

    __call__ = forward

    @torch.no_grad()
    def rollout_step(self, obs_action, ensemble_idx, next_obs_mean, next_obs_std, reward_mean, reward_std):
        """One trajectory batch of state_transition_rollout.py:180-204: returns (next_obs [B,obs_dim], reward [B],
        disagreement [B,1], aleatoric [B,1]) -- de-normalised prediction of the picked member + uncertainties.  An empty batch
        gives empty outputs without a launch."""
        if obs_action.shape[0] == 0:
            f32, dev = torch.float32, self.device
            return (torch.empty((0, self.obs_dim), dtype=f32, device=dev), torch.empty((0,), dtype=f32, device=dev),
                    torch.empty((0, 1), dtype=f32, device=dev), torch.empty((0, 1), dtype=f32, device=dev))
        x, raw = self._raw(obs_action)
        B, dev = x.shape[0], self.device
        idx = torch.as_tensor(ensemble_idx).to(dev, torch.int32).contiguous()
        om = torch.as_tensor(next_obs_mean, dtype=torch.float32).to(dev).contiguous()
        os_ = torch.as_tensor(next_obs_std, dtype=torch.float32).to(dev).contiguous()
        nobs = torch.empty((B, self.obs_dim), dtype=torch.float32, device=dev)
        rew = torch.empty((B,), dtype=torch.float32, device=dev)
        dis = torch.empty((B, 1), dtype=torch.float32, device=dev)
        ale = torch.empty((B, 1), dtype=torch.float32, device=dev)
        check(lib().s2p_ensemble_head(ptr(raw), raw.shape[3], ptr(x), x.shape[3], B, self.E, self.D, ptr(self.min_logstd),
                                      ptr(self.max_logstd), None, None, ptr(idx), ptr(om), ptr(os_), float(reward_mean),
                                      float(reward_std), ptr(nobs), ptr(rew), ptr(dis), ptr(ale), stream()), "s2p_ensemble_head")
        return nobs, rew, dis, ale

    @torch.no_grad()
    def rollout_sweep(self, observations, actions, ensemble_idx, obs_mean, obs_std, next_obs_mean, next_obs_std, reward_mean,
                      reward_std, chunk=16384):
        """The whole `all_state_1step_random_action` rollout of a dataset (state_transition_rollout.py:149-204, SPEC.md N2c) on
        the device: RAW fp32 observations [N, obs_dim], actions [N, A] and member indices [N], each uploaded once -> (next_obs
        [N, obs_dim], reward [N], disagreement [N, 1], aleatoric [N, 1]) fp32 on the device.  One s2p_transition_pack launch
        normalises and packs every row; then per `chunk` rows the grouped fp32 layer chain over ALL E members (the reference
        picks among all of them, not among the elites: `select` is neither read nor changed) and one s2p_ensemble_head that
        writes straight into the dataset-long outputs.  No host synchronisation.  The sweep owns its activations: two ping-pong
        [chunk][E * width] buffers and the raw head input.  A row's result does not depend on `chunk`, bit for bit."""
        dev, E, D, f32, L = self.device, self.E, self.D, torch.float32, lib()
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError("chunk must be positive")
        obs = torch.as_tensor(observations, dtype=f32).to(dev).contiguous()
        act = torch.as_tensor(actions, dtype=f32).to(dev).contiguous()
        N = obs.shape[0]
        if obs.shape != (N, self.obs_dim) or act.shape != (N, self.action_dim):
            raise ValueError("observations [N, %d] and actions [N, %d] are needed, got %s and %s" % (
                self.obs_dim, self.action_dim, tuple(obs.shape), tuple(act.shape)))
        idx = torch.as_tensor(ensemble_idx).reshape(-1)
        if idx.numel() != N or (N and not idx.is_cuda and (int(idx.min()) < 0 or int(idx.max()) >= E)):   # (host indices only: no device sync)
            raise ValueError("ensemble_idx: %d member indices in [0, %d) are needed" % (N, E))
        idx = idx.to(dev, torch.int32).contiguous()

        def vec(v):
            v = torch.as_tensor(v, dtype=f32).reshape(-1).to(dev).contiguous()
            if v.numel() != self.obs_dim:
                raise ValueError("a normalisation vector has %d entries, obs_dim is %d" % (v.numel(), self.obs_dim))
            return v
        om, os_, nom, nos = vec(obs_mean), vec(obs_std), vec(next_obs_mean), vec(next_obs_std)
        kp = self._off[0][2]
        x = ops.transition_pack(obs, act, om, os_, torch.empty((N, kp), dtype=f32, device=dev))
        nobs = torch.empty((N, self.obs_dim), dtype=f32, device=dev)
        rew = torch.empty((N,), dtype=f32, device=dev)
        dis = torch.empty((N, 1), dtype=f32, device=dev)
        ale = torch.empty((N, 1), dtype=f32, device=dev)
        rows = min(chunk, N)
        widths = [cout for _, cout in self._dims]
        ping = [torch.empty(rows * E * max(widths[:-1]), dtype=f32, device=dev) for _ in range(min(2, len(widths) - 1))]
        raw = torch.empty((rows, E * 2 * D), dtype=f32, device=dev)
        for lo in range(0, N, chunk):
            B = min(chunk, N - lo)
            xc = x[lo:lo + B]
            h, hg, hp = xc, 0, kp
            for li, ((cin, cout), (geom, w, b, k)) in enumerate(zip(self._dims, self.layers)):
                last = li == len(self.layers) - 1
                y = raw if last else ping[li % 2]
                check(L.s2p_ensemble_linear_fwd(ptr(h), hg, hp, ptr(w), ptr(b), None, E, E, B, k, cout, ptr(y) if last else None,
                                                None if last else ptr(y), E * cout, stream()), "s2p_ensemble_linear_fwd")
                h, hg, hp = y, cout, E * cout
            check(L.s2p_ensemble_head(ptr(raw), E * 2 * D, ptr(xc), kp, B, E, D, ptr(self.min_logstd), ptr(self.max_logstd), None,
                                      None, ptr(idx[lo:]), ptr(nom), ptr(nos), float(reward_mean), float(reward_std),
                                      ptr(nobs[lo:]), ptr(rew[lo:]), ptr(dis[lo:]), ptr(ale[lo:]), stream()), "s2p_ensemble_head")
        return nobs, rew, dis, ale


class EnsembleTrainer:
    """Adam training of an EnsembleTransition (SPEC.md N2b): torch.optim.Adam semantics without weight decay, one fused launch
    over the model's flat parameter / gradient / moment buffers."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        self.model, self.lr, self.betas, self.eps = model, float(lr), (float(betas[0]), float(betas[1])), float(eps)
        dev = model.device
        self.m = torch.zeros(model._n, dtype=torch.float32, device=dev)
        self.v = torch.zeros(model._n, dtype=torch.float32, device=dev)
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)

    @torch.no_grad()
    def train_step(self, obs_action, target):
        """forward, head, backward, Adam: 4 + 1 + 4 + 1 library calls.  Returns (loss, nll_per_member, mse_per_member) as device
        tensors of this step's forward (before the update)."""
        mo = self.model
        buf, B = mo._loss_backward(obs_action, target)
        check(lib().s2p_adam_step_dev(ptr(mo._flat), ptr(mo._grad), ptr(self.m), ptr(self.v), mo._n, self.lr, self.betas[0],
                                      self.betas[1], self.eps, ptr(self.step), 1.0, stream()), "s2p_adam_step_dev")
        G = len(mo.select)
        sums = buf["sums"] / (B * mo.D)
        return buf["loss"][0].clone(), sums[:G], sums[G:]

    @torch.no_grad()
    def evaluate(self, obs_action, target):
        """obs_action [B, in], target [B, D] -> mse [len(select)] (mean over rows and outputs of (mu - target)^2)."""
        mo = self.model
        x, xg, B, t, tg = mo._pack_input(obs_action, target)
        buf = mo._forward_train(x, xg, B, keep_pre=False)
        mo._head(buf, x, xg, t, tg, B, grad=False)
        return buf["sums"][len(mo.select):].clone() / (B * mo.D)

    def fit(self, inputs, targets, epochs, batch_size=256, holdout=0.1, n_elite=5, seed=0, log=None):
        """The MOPO-lineage loop (SPEC.md N2b, unpinned): a seeded holdout split; every epoch each member draws its own
        bootstrap indices (with replacement) over the training rows; after the epoch the per-member holdout MSE is computed
        and update_save(e) is called for the members whose MSE improved on their best; at the end set_select picks the
        n_elite members with the best saved holdout MSE.  holdout: a fraction of the rows (or a row count).
        Returns {"initial_mse", "epoch_mse": [per epoch], "holdout_mse": best per member, "elites": [...], "saved": [members
        saved, per epoch]}."""
        mo = self.model
        E = mo.E
        assert len(mo.select) == E, "fit trains every member: call set_select(range(E)) first"
        inputs, targets = torch.as_tensor(inputs, dtype=torch.float32), torch.as_tensor(targets, dtype=torch.float32)
        n = inputs.shape[0]
        g = torch.Generator().manual_seed(seed)
        perm = torch.randperm(n, generator=g)
        n_hold = int(holdout) if holdout >= 1 else max(1, int(math.ceil(n * holdout)))
        hold, train = perm[:n_hold], perm[n_hold:]
        xh, th = inputs[hold].to(mo.device), targets[hold].to(mo.device)
        xt, tt = inputs[train].to(mo.device), targets[train].to(mo.device)
        nt = train.shape[0]
        best = self.evaluate(xh, th).cpu()
        initial, epoch_mse = best.clone(), []
        mo.update_save(list(range(E)))
        history = []
        for epoch in range(epochs):
            idx = torch.randint(nt, (E, nt), generator=g).to(mo.device)
            for s in range(0, nt, batch_size):
                bi = idx[:, s:s + batch_size]
                self.train_step(xt[bi], tt[bi])
            mse = self.evaluate(xh, th).cpu()
            improved = [e for e in range(E) if float(mse[e]) < float(best[e])]
            if improved:
                mo.update_save(improved)
                best[improved] = mse[improved]
            history.append(improved)
            epoch_mse.append(mse)
            if log:
                log(epoch, mse, improved)
        elites = sorted(torch.argsort(best)[:n_elite].tolist())
        mo.set_select(elites)
        return {"initial_mse": initial, "epoch_mse": epoch_mse, "holdout_mse": best, "elites": elites, "saved": history}
