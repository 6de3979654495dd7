"""N3e -- the CQL step on HIP (s2p_amd/cql.py, csrc/mlp.hip, csrc/cql.hip).  PINNED parity: tests/golden/cql_golden_v1.npz holds fp64 results of
the REAL reference trainer, the noise it drew, and `ref32_err`, the deviation of the trainer's own fp32 run from them; a larger shape,
which the fixture does not hold, is checked against tests/cql_ref.py run in fp64 and fp32 on the CPU inside the test
(tests/test_cql.py pins that restatement to the fixture at 1e-9).

Tolerance: per quantity K_TOL x max(ref32_err, 1e-6), K_TOL = 4 (the rule and constants of tests/test_iql_gpu.py): the HIP path is
the same fp32 arithmetic in another summation order.  Step-2 parameters are compared through their UPDATE (final - initial),
relative to the tensor's largest update, against the fp32 reference run's own deviation of the update (`update_ref32_err`); the
fixture's maker asserts that the trainer's own fp32 run stays within 1e-3 of every update over the whole tensor, so every element
is compared.  Worst observed ratios: DESIGN.md section 6b.5."""
import os

import numpy as np
import pytest
import torch

import cql_ref as C
import iql_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "cql_golden_v1.npz"))
Z, A, H, P, B, RN, STEPS = (int(v) for v in G["sizes"])
CRITIC_SD = {k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("sd.") and not k.startswith("sd.policy.")}
POLICY_SD = {k[10:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("sd.policy.")}
BATCHES = [{k.split(".", 1)[1]: torch.from_numpy(G[k]) for k in G.files if k.startswith("batch%d." % s)} for s in range(STEPS)]
NOISES = [{k.split(".", 1)[1]: torch.from_numpy(G[k]) for k in G.files if k.startswith("noise%d." % s)} for s in range(STEPS)]
K_TOL, FLOOR = 4.0, 1e-6
WORST = {}


def _check(group, err, ref_err, what=""):
    ref = max(float(ref_err), FLOOR)
    WORST[group] = max(WORST.get(group, 0.0), err / ref)
    print("%-24s %-40s err %.3e  ref32_err %.3e  ratio %.3f" % (group, what, err, float(ref_err), err / ref))
    assert err <= K_TOL * ref, (group, what, err, K_TOL * ref)


def _trainer(critic_sd, policy_sd, dev, sizes=(Z, A, H, P), **kw):
    from s2p_amd.cql import CQLTrainer, CriticSLAC, Qfunction, TanhGaussianPolicy, Vfunction
    z, a, h, p = sizes
    q = [Qfunction(hidden_sizes=[h, h], output_size=1, input_size=z + a) for _ in range(4)]
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=[h, h], output_size=1, input_size=z), device=dev)
    policy = TanhGaussianPolicy(hidden_sizes=[h, h], obs_dim=p, action_dim=a, device=dev)
    if critic_sd is not None:
        critic.load_state_dict(critic_sd, strict=True)
        policy.load_state_dict(policy_sd, strict=True)
    cfg = dict(discount=0.99, soft_target_tau=5e-3, policy_lr=1e-4, qf_lr=3e-4, reward_scale=1, use_automatic_entropy_tuning=True,
               policy_eval_start=2, temp=1.0, min_q_weight=5.0, num_random=RN, deterministic_backup=False)
    cfg.update(kw)
    return CQLTrainer(None, policy, critic=critic, **cfg)


def _step(tr, b, noise=None):
    return tr.train_from_latents(b["z"], b["next_z"], b["action"], b["policy_input"], b["policy_next_input"], b["rewards"], b["terminals"],
                                 noise=noise)


def _grads(tr):
    g = {"grad." + k: v for k, v in tr.critic.grads().items() if not k.startswith("vf.")}
    g.update(("grad.policy." + k, v) for k, v in tr.policy.grads().items())
    return g


def _scalar_err(got, want):
    return abs(float(got) - float(want)) / (abs(float(want)) or 1.0)


def _check_step(tr, want, tag):
    """want: name -> (fp64 value, ref32_err) of a step's statistics and gradients."""
    stats = tr.last_statistics()
    for k in C.STATS:
        _check("losses and alpha", _scalar_err(stats[k], want[k][0]), want[k][1], "%s %s" % (tag, k))
    grads = _grads(tr)
    assert sorted(grads) == sorted(k for k in want if k.startswith("grad."))               # none for the targets and vf
    for k, g in grads.items():
        assert float(g.abs().max()) > 0, k
        _check("policy gradients" if ".policy." in k else "critic gradients", R.rel_max(g, want[k][0]), want[k][1], "%s %s" % (tag, k))
    assert float(tr.critic.grads()["vf.fc0.weight"].abs().max()) == 0                       # vf takes part in no loss


def test_three_steps_against_the_real_trainer(hip_device):
    tr = _trainer(CRITIC_SD, POLICY_SD, hip_device)
    for s in range(STEPS):
        losses = _step(tr, BATCHES[s], NOISES[s])
        assert bool(torch.isfinite(losses).all())
        if s < 2:
            pre = "step%d." % s
            want = {k[len(pre):-10]: (G[k[:-10]], G[k]) for k in G.files if k.startswith(pre) and k.endswith(".ref32_err")}
            assert set(C.STATS) < set(want)
            _check_step(tr, want, "step %d" % s)
    assert tr._n_train_steps_total == STEPS and tr._current_epoch == STEPS
    got = dict(tr.critic.state_dict())
    got.update(("policy." + k, v) for k, v in tr.policy.state_dict().items())
    got["log_alpha"] = tr.log_alpha.cpu()
    init = dict(CRITIC_SD)
    init.update(("policy." + k, v) for k, v in POLICY_SD.items())
    init["log_alpha"] = torch.zeros(1)
    finals = {k[6:-17]: (torch.from_numpy(G[k[:-17]]), G[k]) for k in G.files if k.startswith("final.") and k.endswith(".update_ref32_err")}
    assert sorted(got) == sorted(finals)
    for k, (ref, err) in finals.items():
        upd = float((ref - init[k].double()).abs().max())
        if k.startswith("vf."):
            assert upd == 0 and torch.equal(got[k], init[k])
            continue
        group = "log_alpha" if k == "log_alpha" else ("policy" if k.startswith("policy.") else "critic") + " step-2 updates"
        _check(group, float((got[k].double() - ref).abs().max() / upd), err, "final." + k)
    stats = tr.eval_statistics                                                            # (filled by the first step only)
    for k in ("QF1 Loss", "min QF1 Loss", "QF2 Loss", "min QF2 Loss", "Std QF1 values", "Std QF2 values", "Policy Loss", "Alpha", "Alpha Loss"):
        assert abs(stats[k] - float(G["step0." + k])) <= 1e-4 * max(1.0, abs(float(G["step0." + k]))), k
    assert stats["Num Q Updates"] == 1 and stats["Num Policy Updates"] == 1


@pytest.mark.parametrize("cloning", [True, False])
def test_a_larger_shape_against_the_restatement(hip_device, cloning):
    """Z 90, A 6, H 128, P 102, B 130, R 10: K = 96 and 102 -> 104 (padded), 130 (1 + 30) = 4030 rows through the critics (no multiple
    of the 128-row tile), one row past the tile in the policy phase; the cloning branch and the SAC branch of step 0."""
    z, a, h, p, b, rn = 90, 6, 128, 102, 130, 10
    critic, policy = R.init_params(z, a, h, p, seed=11, last_scale=30.0)
    batch, noise = C.make_batch(b, z, a, p, 500, terminals=True, scale=0.5), C.make_noise(b, a, rn, 501)
    cfg = dict(C.CFG, num_random=rn, policy_eval_start=2 if cloning else 0)
    s64, s32 = (C.train(critic, policy, [batch], [noise], dt, cfg)[0][0] for dt in (torch.float64, torch.float32))
    want = {k: (s64[k], R.rel_max(s32[k], s64[k])) for k in s64 if k != "q_target"}
    tr = _trainer(critic, policy, hip_device, (z, a, h, p), num_random=rn, policy_eval_start=cfg["policy_eval_start"])
    _step(tr, batch, noise)
    _check_step(tr, want, "cloning" if cloning else "sac")
    qt = tr._buf[b]["q_target"].cpu()
    _check("q_target", R.rel_max(qt, s64["q_target"]), R.rel_max(s32["q_target"], s64["q_target"]), "q_target")


def test_device_noise_and_the_other_options(hip_device):
    """noise=None draws on the device from the trainer's generator: the same seed gives the same step, another seed another one;
    no entropy tuning leaves alpha at 1 and log_alpha alone; the deterministic backup leaves the alpha term out of q_target."""
    def run(seed, **kw):
        gen = torch.Generator(device=hip_device).manual_seed(seed)
        tr = _trainer(CRITIC_SD, POLICY_SD, hip_device, generator=gen, policy_eval_start=0, **kw)
        losses = _step(tr, BATCHES[1]).clone()
        return tr, losses

    (t1, l1), (t2, l2), (t3, l3) = run(1), run(1), run(2)
    assert torch.equal(l1, l2) and not torch.equal(l1, l3) and bool(torch.isfinite(l1).all())
    u = t1._buf[B]["uniform"]
    assert float(u.min()) >= -1 and float(u.max()) <= 1 and abs(float(u.mean())) < 0.2 and abs(float(t1._buf[B]["eps2"].std()) - 1) < 0.2
    t4, _ = run(1, use_automatic_entropy_tuning=False)
    assert float(t4.alpha) == 1.0 and float(t4.log_alpha) == 0.0 and "Alpha" not in t4.eval_statistics
    t5, _ = run(1, deterministic_backup=True)
    b = t5._buf[B]
    tq = torch.min(b["tq"][0], b["tq"][1])
    want = b["reward"] + (1 - b["terminal"]) * 0.99 * tq
    assert R.rel_max(b["q_target"].cpu(), want.cpu()) < 1e-6
    assert t1.launches["s2p_mlp_linear_fwd"] == 12 and t1.launches["s2p_mlp_linear_dgrad"] == 3 and t1.launches["s2p_mlp_linear_bwd"] == 4
    assert t1.launches["s2p_mlp_linear_bwd_split"] == 2 and t1._buf[B]["critic_split"] == [0, 8, 8]
    assert t1.launches["s2p_tanh_gauss_rsample"] == 4 and t1.launches["s2p_cql_critic_head"] == 1 and t1.launches["s2p_sac_policy_head"] == 1


def test_state_dict_round_trip_and_strict_load(hip_device, tmp_path):
    tr = _trainer(CRITIC_SD, POLICY_SD, hip_device)
    assert list(tr.critic.state_dict()) == [str(k) for k in G["critic_keys"]] and list(tr.policy.state_dict()) == [str(k) for k in G["policy_keys"]]
    for k, v in tr.critic.state_dict().items():
        assert torch.equal(v, CRITIC_SD[k]), k                                  # a reference-layout state_dict loads strict and comes back
    for k, v in tr.policy.state_dict().items():
        assert torch.equal(v, POLICY_SD[k]), k
    with pytest.raises(RuntimeError):
        tr.critic.load_state_dict({k: v for k, v in CRITIC_SD.items() if k != "qf2.fc0.bias"}, strict=True)
    with pytest.raises(RuntimeError):
        tr.policy.load_state_dict(dict(POLICY_SD, extra=torch.zeros(1)), strict=True)
    _step(tr, BATCHES[0], NOISES[0])
    _step(tr, BATCHES[1], NOISES[1])
    torch.save(tr.get_snapshot(), tmp_path / "snap.pth")
    tr2 = _trainer(None, None, hip_device).load_state_dict(torch.load(tmp_path / "snap.pth"))
    assert tr2._n_train_steps_total == 2 and tr2._current_epoch == 2
    sd = tr.state_dict()
    osd = sd["critic_optimizer"]
    assert len(osd["param_groups"][0]["params"]) == 30 and len(osd["state"]) == 12 and float(osd["state"][0]["step"]) == 2   # none for the targets and vf
    assert float(sd["alpha_optimizer"]["state"][0]["step"]) == 2 and float(sd["log_alpha"]) != 0
    l1, l2 = _step(tr, BATCHES[2], NOISES[2]).clone(), _step(tr2, BATCHES[2], NOISES[2]).clone()
    assert torch.equal(l1, l2) and torch.equal(tr.log_alpha_state, tr2.log_alpha_state)
    for a, b in ((tr.critic.state_dict(), tr2.critic.state_dict()), (tr.policy.state_dict(), tr2.policy.state_dict())):
        assert all(torch.equal(a[k], b[k]) for k in a)                            # the restored trainer continues bit for bit


@pytest.mark.parametrize("freeze", [True, False])
def test_train_from_torch_on_a_tiny_real_buffer(hip_device, freeze):
    import slac_buffer_ref as SB
    from s2p_amd.slac_algo import SlacAlgorithm
    algo = SlacAlgorithm((3, 100, 100), (SB.A,), 1, hip_device, seed=0, batch_size_latent=2, buffer_size=32, num_sequences=SB.S, frame_capacity=128)
    algo.load_data_in_buffer(SB.real_dataset(2, 12, 100, 100), **dict(SB.LOAD_ARGS["real"], data_num=24))
    tr = _trainer(None, None, hip_device, (288, SB.A, 64, SB.S * 256 + (SB.S - 1) * SB.A), slac_algo=algo, freeze_slac=freeze, num_random=3)
    before = [p.detach().clone() for p in algo.latent.parameters()]
    c0 = tr.critic.state_dict()
    for _ in range(3):
        losses = tr.train_from_torch(algo.buffer.random_batch(4))
        assert bool(torch.isfinite(losses).all())
    assert tr._n_train_steps_total == 3 and algo.learning_steps_latent == (0 if freeze else 3)
    same = [torch.equal(p, q) for p, q in zip(algo.latent.parameters(), before)]
    assert all(same) if freeze else not any(same)
    c1 = tr.critic.state_dict()
    assert all(not torch.equal(c0[k], c1[k]) for k in c0 if k.endswith("weight") and not k.startswith("vf."))
    assert ("SLAC Loss kld" in tr.eval_statistics) == (not freeze)


def test_zz_report_worst_ratios(hip_device):
    print("\nworst deviation / max(ref32_err, 1e-6) per group:", {k: round(v, 3) for k, v in WORST.items()})
    assert WORST and max(WORST.values()) <= K_TOL
