"""N3g -- cached encoder features for frozen-SLAC IQL / CQL steps (s2p_amd/slac_buffer.py `attach_features`, `FeatureBatch`;
`SlacAlgorithm.prepare_batch`), on the tiny real buffer of tests/test_iql_gpu.py.

Bounds.  The table against `Encoder.forward` and the fp64 encoder of oracle/slac_oracle.py: rel_max < 1e-4 for fp32 stacks, < 4e-2 for
bf16 -- what tests/test_actor_gpu.py::test_cached_window_equals_a_full_reencode holds this same comparison to.  `prepare_batch` and
the trainers' step-0 losses: the project's rule, K_TOL x max(ref_err, 1e-6) with K_TOL = 4, where ref_err is the deviation of the
FRAMES path (the behaviour before the cache existed) from the fp64 restatement (tests/slac_latent_ref.py on the oracle encoder's
features), measured in the test, and the cached path's deviation from that same fp64 result is what is bounded."""
import copy

import numpy as np
import pytest
import torch

import iql_ref as IR
import slac_buffer_ref as SB
import slac_latent_ref as R
import slac_oracle as SO

pytestmark = pytest.mark.gpu
K_TOL, FLOOR = 4.0, 1e-6
S, A, FEAT, Z = SB.S, SB.A, 256, 288
P = S * FEAT + (S - 1) * A
DTYPES = [(torch.float32, 1e-4), (torch.bfloat16, 4e-2)]
IDXES = np.array([0, 3, 7, 8, 3])


@pytest.fixture(scope="module")
def params():
    return R.make_params(A)


@pytest.fixture(scope="module")
def algos(hip_device, params):
    """dtype -> a SlacAlgorithm with the seeded latent weights and 9 windows / 25 frames of the small real dataset; built once.
    Tests leave it without a feature table and with those weights."""
    from s2p_amd.slac_algo import SlacAlgorithm
    cache = {}

    def get(dtype=torch.float32):
        if dtype not in cache:
            algo = SlacAlgorithm((3, 100, 100), (A,), 1, hip_device, seed=0, batch_size_latent=2, buffer_size=32, num_sequences=S,
                                 frame_capacity=128, dtype=dtype)
            algo.latent.load_state_dict(R.full_state_dict(params), strict=True)
            algo.load_data_in_buffer(SB.real_dataset(2, 12, 100, 100), **dict(SB.LOAD_ARGS["real"], data_num=24))
            cache[dtype] = algo
        return cache[dtype]
    return get


def _enc64(encoder):
    return {k: v.detach().double().cpu() for k, v in encoder.state_dict().items()}


def _oracle_features(encoder, frames_u8_nhwc):
    """fp64 features [n,256] of uint8 NHWC frames [n,100,100,3] under the encoder's present weights."""
    x = frames_u8_nhwc.cpu().permute(0, 3, 1, 2).double() / 255.0
    return SO.encoder_forward(_enc64(encoder), x[None])[0]


def _live_slots(buf):
    return torch.from_numpy(np.arange(max(buf._tail, buf._head - buf.frame_capacity), buf._head) % buf.frame_capacity).to(buf.device)


def _check_table(buf, encoder, tol, oracle=None, what=""):
    slots = _live_slots(buf)
    frames = buf.pool[slots]
    got = buf.features[slots].cpu()
    full = encoder(frames[None])[0].detach().cpu()
    oracle = _oracle_features(encoder, frames) if oracle is None else oracle
    e_full, e_oracle = R.rel_max(got, full), R.rel_max(got, oracle)
    print("%s table of %d live frames: vs Encoder.forward %.3e, vs the fp64 oracle %.3e (bound %.0e)" % (what, len(slots), e_full, e_oracle, tol))
    assert got.shape == (len(slots), FEAT) and float(got.abs().max()) > 0
    assert e_full < tol and e_oracle < tol, (what, e_full, e_oracle, tol)
    return oracle


@pytest.mark.parametrize("dtype,tol", DTYPES)
def test_table_equals_the_encoder_on_every_live_frame(algos, dtype, tol):
    algo = algos(dtype)
    buf, enc = algo.buffer, algo.latent.encoder
    tables, oracle = [], None
    for chunk in (1, 5, 1024):
        buf.attach_features(enc, chunk)
        assert tuple(buf.features.shape) == (128, FEAT) and buf.features.dtype == torch.float32 and buf._fhead == buf._head == 25
        oracle = _check_table(buf, enc, tol, oracle, "chunk %d" % chunk)
        tables.append(buf.features.clone())
        buf.detach_features()
    assert buf.features is None
    print("tables of chunk 1 / 5 / 1024 bitwise equal:", torch.equal(tables[0], tables[1]), torch.equal(tables[0], tables[2]))


def _fp64_batch(algo, params, idxes, noise):
    """z, next_z, feature_action, next_feature_action of the windows `idxes` in fp64: the oracle encoder, then the restated chain."""
    from s2p_amd.slac import create_feature_actions
    buf = algo.buffer
    frames = buf.window_frames(idxes)                                                       # [B,S+1,100,100,3]
    B = len(idxes)
    feat = _oracle_features(algo.latent.encoder, frames.reshape(B * (S + 1), 100, 100, 3)).reshape(B, S + 1, FEAT)
    action_ = buf.action_[torch.from_numpy(idxes).to(buf.device)].double().cpu()
    p64 = {k: v.double() for k, v in params.items()}
    _, _, z1, z2 = R.sample_posterior(p64, feat, action_, noise.double().cpu())
    z_ = torch.cat([z1, z2], dim=-1)
    fa, nfa = create_feature_actions(feat, action_)
    return dict(z=z_[:, -2], next_z=z_[:, -1], feature_action=fa, next_feature_action=nfa)


def _rule(what, cached, frames, ref):
    ref_err, err = R.rel_max(frames, ref), R.rel_max(cached, ref)
    bound = K_TOL * max(ref_err, FLOOR)
    print("%-28s frames path ref_err %.3e  cached path err %.3e  bound %.3e  (cached vs frames bitwise: %s)"
          % (what, ref_err, err, bound, torch.equal(torch.as_tensor(cached), torch.as_tensor(frames))))
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("dtype,tol", DTYPES)
def test_prepare_batch_from_features_and_from_frames(algos, params, dtype, tol):
    from s2p_amd.slac_buffer import FeatureBatch, FrameBatch
    algo = algos(dtype)
    buf = algo.buffer
    algo.cache_features()
    noise = torch.randn(len(IDXES), S + 1, Z, generator=torch.Generator().manual_seed(41)).to(buf.device)
    b_fr, b_ft = buf.random_batch(len(IDXES), idxes=IDXES), buf.random_batch(len(IDXES), idxes=IDXES, frames="features")
    assert isinstance(b_fr["observations"], FrameBatch) and isinstance(b_ft["observations"], FeatureBatch)
    assert b_ft["observations"].shape == b_fr["observations"].shape == (len(IDXES), S + 1, 3, 100, 100) and len(b_ft["observations"]) == len(IDXES)
    names = ("z", "next_z", "action", "feature_action", "next_feature_action")
    fr = dict(zip(names, algo.prepare_batch(b_fr["observations"], b_fr["actions"], noise)))
    ft = dict(zip(names, algo.prepare_batch(b_ft["observations"], b_ft["actions"], noise)))
    buf.detach_features()
    assert all(tuple(ft[k].shape) == tuple(fr[k].shape) for k in names) and tuple(ft["feature_action"].shape) == (len(IDXES), P)
    assert torch.equal(ft["action"], fr["action"])
    for k in ("actions", "rewards", "terminals"):
        assert tuple(b_ft[k].shape) == tuple(b_fr[k].shape) and torch.equal(b_ft[k], b_fr[k]), k
    ref = _fp64_batch(algo, params, IDXES, noise)
    for k in ref:
        _rule("%s %s" % (str(dtype)[6:], k), ft[k].cpu(), fr[k].cpu(), ref[k])


def _iql(dev, algo, sd):
    from s2p_amd.iql import CriticSLAC, IQLTrainer, Qfunction, TanhGaussianPolicy, Vfunction
    q = [Qfunction(hidden_sizes=[64, 64], output_size=1, input_size=Z + A) for _ in range(4)]
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=[64, 64], output_size=1, input_size=Z), device=dev)
    policy = TanhGaussianPolicy(hidden_sizes=[64, 64], obs_dim=P, action_dim=A, device=dev)
    critic.load_state_dict(sd[0], strict=True)
    policy.load_state_dict(sd[1], strict=True)
    return IQLTrainer(None, policy, critic=critic, slac_algo=algo, freeze_slac=True, discount=0.99, policy_lr=1e-4, qf_lr=3e-4, reward_scale=1,
                      soft_target_tau=0.005, beta=0.1, quantile=0.7, clip_score=100, target_update_period=2)


def _cql(dev, algo, sd):
    from s2p_amd.cql import CQLTrainer, CriticSLAC, Qfunction, TanhGaussianPolicy, Vfunction
    q = [Qfunction(hidden_sizes=[64, 64], output_size=1, input_size=Z + A) for _ in range(4)]
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=[64, 64], output_size=1, input_size=Z), device=dev)
    policy = TanhGaussianPolicy(hidden_sizes=[64, 64], obs_dim=P, action_dim=A, device=dev)
    critic.load_state_dict(sd[0], strict=True)
    policy.load_state_dict(sd[1], strict=True)
    return CQLTrainer(None, policy, critic=critic, slac_algo=algo, freeze_slac=True, discount=0.99, soft_target_tau=5e-3, policy_lr=1e-4,
                      qf_lr=3e-4, reward_scale=1, use_automatic_entropy_tuning=True, policy_eval_start=0, temp=1.0, min_q_weight=5.0,
                      num_random=3, deterministic_backup=False, generator=torch.Generator(device=dev).manual_seed(77))


@pytest.mark.parametrize("kind", ["iql", "cql"])
def test_a_trainer_step_on_either_batch_form(hip_device, algos, params, kind):
    """Three identical trainers take step 0 on the same windows after the same torch.manual_seed (which fixes the chain's eps): one on a
    FrameBatch, one on a FeatureBatch, one through `train_from_latents` on the fp64-derived latents cast to fp32 -- the reference
    both are measured against."""
    algo = algos(torch.float32)
    buf = algo.buffer
    make = _iql if kind == "iql" else _cql
    sd = IR.init_params(Z, A, 64, P, seed=5, last_scale=30.0)
    algo.cache_features()
    B = len(IDXES)
    losses = {}
    for form in ("packed", "features"):
        tr = make(hip_device, algo, sd)
        torch.manual_seed(123)
        losses[form] = tr.train_from_torch(buf.random_batch(B, idxes=IDXES, frames=form)).double().cpu().clone()
    buf.detach_features()
    torch.manual_seed(123)
    noise = torch.randn((B, S + 1, Z), dtype=torch.float32, device=buf.device)             # what prepare_batch drew
    ref = {k: v.float() for k, v in _fp64_batch(algo, params, IDXES, noise).items()}
    win = torch.from_numpy(IDXES).to(buf.device)
    tr = make(hip_device, algo, sd)
    args = (ref["z"], ref["next_z"], buf.action_[win, -1], ref["feature_action"]) + ((ref["next_feature_action"],) if kind == "cql" else ())
    want = tr.train_from_latents(*args, buf.reward_[win, -1], buf.done_[win, -1]).double().cpu()
    assert bool(torch.isfinite(want).all()) and len(want) == 4
    for i in range(4):
        scale = abs(float(want[i])) or 1.0
        ref_err, err = abs(float(losses["packed"][i] - want[i])) / scale, abs(float(losses["features"][i] - want[i])) / scale
        bound = K_TOL * max(ref_err, FLOOR)
        print("%s loss %d: %.6f  frames path ref_err %.3e  cached path err %.3e  bound %.3e" % (kind, i, float(want[i]), ref_err, err, bound))
        assert err <= bound, (kind, i, err, bound)


def test_a_changed_encoder_is_refused_until_refresh(algos, params):
    algo = algos(torch.float32)
    buf, enc = algo.buffer, algo.latent.encoder
    algo.cache_features()
    try:
        buf.random_batch(2, frames="features")
        for p in algo.latent.parameters():
            p.grad = torch.full_like(p, 0.5)
        algo.optim_latent.step()
        algo.optim_latent.zero_grad()
        for call in (lambda: buf.random_batch(2, frames="features"), lambda: buf.sample_sac(2, frames="features")):
            with pytest.raises(RuntimeError, match=r"refresh_features\(\)"):
                call()
        buf.refresh_features()
        assert isinstance(buf.random_batch(2, frames="features"), dict)
        _check_table(buf, enc, 1e-4, what="after an optimizer step and refresh_features():")
        algo.latent.load_state_dict(R.full_state_dict(params), strict=True)
        with pytest.raises(RuntimeError, match=r"refresh_features\(\)"):
            buf.random_batch(2, frames="features")
        buf.refresh_features()
        buf.sample_sac(2, frames="features")
        _check_table(buf, enc, 1e-4, what="after load_state_dict and refresh_features():")
    finally:
        algo.latent.load_state_dict(R.full_state_dict(params), strict=True)
        algo.optim_latent.state.clear()
        buf.detach_features()


def _all_windows(buf):
    n = len(buf)
    return buf.random_batch(n, idxes=np.arange(n), frames="features")["observations"].feature_


def _afresh(buf, encoder, chunk):
    """`feature_` of every window from a table built afresh on a copy of the buffer (the copy shares the pool and the tables)."""
    other = copy.copy(buf)
    other.attach_features(encoder, chunk)
    assert other.features is not buf.features
    return _all_windows(other)


@pytest.mark.parametrize("chunk", [1, 1024])
def test_frames_stored_after_the_build_are_encoded_before_a_sample(hip_device, algos, chunk):
    """An episode, the build, then three more episodes through reset_episode / append: 52 frames through a ring of 40, so the slots
    0..11, encoded at build time, hold other frames now.  One frame a launch (chunk 1) makes the chunk boundaries of the lazy path
    and of the fresh build the same: bitwise.  Otherwise the table's bound applies."""
    from s2p_amd.slac_buffer import ReplayBuffer
    enc = algos(torch.float32).latent.encoder
    buf = ReplayBuffer(8, S, (3, 100, 100), (A,), hip_device, frame_capacity=40)
    r = np.random.RandomState(17)

    def episode(steps=12):
        buf.reset_episode(r.randint(0, 256, size=(3, 100, 100)).astype(np.uint8))
        for t in range(steps):
            buf.append(r.uniform(-1, 1, A).astype(np.float32), float(r.randn()), False, r.randint(0, 256, size=(3, 100, 100)).astype(np.uint8),
                       t == steps - 1)
    episode()
    buf.attach_features(enc, chunk)
    built = buf.features[:13].clone()
    for _ in range(3):
        episode()
    assert buf._head == 52 and buf._fhead == 13 and len(buf) == 8
    got = _all_windows(buf)
    assert buf._fhead == 52 and not torch.equal(buf.features[:12], built[:12]) and torch.equal(buf.features[12], built[12])
    want = _afresh(buf, enc, chunk)
    err = R.rel_max(got, want)
    print("chunk %d: lazily encoded vs built afresh: %.3e, bitwise %s" % (chunk, err, torch.equal(got, want)))
    assert tuple(got.shape) == (8, S + 1, FEAT) and float(got.abs().max()) > 0
    assert torch.equal(got, want) if chunk == 1 else err < 1e-4
    assert torch.equal(got.cpu(), buf.features[buf.table[:8].long()].cpu())               # and the windows do read their own slots


def test_a_second_bulk_load_after_the_build(algos):
    from s2p_amd.slac_algo import SlacAlgorithm
    base = algos(torch.float32)
    enc = base.latent.encoder
    algo = SlacAlgorithm((3, 100, 100), (A,), 1, enc.device, seed=0, batch_size_latent=2, buffer_size=32, num_sequences=S, frame_capacity=128)
    algo.latent = base.latent
    data = SB.real_dataset(2, 12, 100, 100)
    algo.load_data_in_buffer(data, **dict(SB.LOAD_ARGS["real"], data_num=24))
    buf = algo.buffer
    buf.attach_features(enc, 1)
    data2 = dict(data, image_observations=255 - data["image_observations"], image_observations_tp1=255 - data["image_observations_tp1"])
    algo.load_data_in_buffer(data2, **dict(SB.LOAD_ARGS["real"], data_num=24))
    assert len(buf) == 18 and buf._head == 50 and buf._fhead == 25
    got = _all_windows(buf)
    assert buf._fhead == 50 and torch.equal(got, _afresh(buf, enc, 1))
    assert not torch.equal(got[:9], got[9:])


def test_the_same_seed_selects_the_same_windows(algos):
    algo = algos(torch.float32)
    buf = algo.buffer
    algo.cache_features()
    np.random.seed(9)
    a = buf.random_batch(4)
    np.random.seed(9)
    b = buf.random_batch(4, frames="features")
    np.random.seed(9)
    c = buf.sample_sac(4, frames="features")
    buf.detach_features()
    for k in ("actions", "rewards", "terminals"):
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
    assert torch.equal(c[1], a["actions"]) and torch.equal(c[2], a["rewards"]) and torch.equal(c[3], a["terminals"])
    assert torch.equal(c[0].feature_, b["observations"].feature_) and torch.equal(b["observations"].action_, a["actions"])
