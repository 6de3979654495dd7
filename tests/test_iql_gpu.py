"""N3d -- the IQL step on HIP (s2p_amd/iql.py, csrc/mlp.hip, csrc/iql.hip).  PINNED parity: tests/golden/iql_golden_v1.npz holds fp64 results of
the REAL reference trainer and `ref32_err`, the deviation of the trainer's own fp32 run from them; the production widths, which the
fixture does not hold, are checked against tests/iql_ref.py run in fp64 and fp32 on the CPU inside the test (tests/test_iql.py pins
that restatement to the fixture at 1e-9).

Tolerance: per quantity K_TOL x max(ref32_err, 1e-6), K_TOL = 4 (the rule and constants of tests/test_ensemble_train_gpu.py): the HIP
path is the same fp32 arithmetic in another summation order.  Step-2 parameters are compared through their UPDATE (final - initial,
what the three steps produce), relative to the tensor's largest update, against the fp32 reference run's own deviation of the update.

The one exception (the Adam steps).  The first Adam steps are about lr g / (|g| + eps) per element: they depend on an element's
gradient through ratios only, so an element whose gradient cancels to near zero can differ by up to lr -- a third of the largest
update after three steps -- between ANY two fp32 runs.  The fixture has no such element (asserted in its maker: the trainer's own
fp32 run stays within 1e-3 of every update over the whole tensor), so there EVERY element of every step-2 parameter is compared.

The production widths.  Step 0 (losses, weights, every gradient) is held to the rule above against tests/iql_ref.py in fp64.  The
step-2 parameters cannot be: with 256 x 1024 hidden units per layer and network, some pre-activation lies within fp32 rounding of 0
in almost every run, and a ReLU that falls on the other side changes the gradients of that step discontinuously.  Measured on the
CPU alone, with this test's seeds: tests/iql_ref.py in fp32 torch against ITSELF with the hidden units relabelled (the same
function, another summation order) differs from the fp64 run by 0.32 (qf1.fc0.weight; the HIP path shows the same 0.319 there),
0.56 (qf1.fc1.weight), 0.49 (vf.fc0.weight) and 1.04 (policy.fc1.weight) of the largest update, 76 % of qf1.fc0.weight's elements
lie beyond K_TOL x ref32_err, and which tensors are hit changes with the relabelling -- a gradient floor does not help (the floor
of |g| > 5e-5 of the tensor's largest, which leaves out 0.6 %, was applied in these figures).  So at these widths the steps after
the first are checked where the comparison is well posed: the three optimizer steps and the two target updates are replayed in
fp64 on the host from the HIP path's OWN gradients of each step, and every step-2 parameter must match that replay to
K_TOL x e of the tensor's largest update, e = e_store + e_adam.  e_store = 3 half-ulps of the tensor's largest parameter (its fp32
storage rounds once per step) over the largest update: 6e-6 for the critics' weights (|p| <= 1/32, update 9e-4), 1.9e-5 for the
policy's (update 3e-4).  e_adam = 2^-24 / (1 - beta2) / 2 = 3.0e-5: s2p_adam_step_dev forms the bias correction 1 - beta2^t on the
device from the fp32 beta2 = 0.999, whose half-ulp 2^-24 becomes a relative 2^-24 t beta2^t / (1 - beta2^t) <= 2^-24 / (1 - beta2)
of the correction in the first steps, and half of that after the square root (torch forms the corrections in double on the host).  Worst observed
ratios: DESIGN.md section 6b.4."""
import math
import os

import numpy as np
import pytest
import torch

import iql_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "iql_golden_v1.npz"))
Z, A, H, P, B, STEPS = (int(v) for v in G["sizes"])
CRITIC_SD = {k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("sd.") and not k.startswith("sd.policy.")}
POLICY_SD = {k[10:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("sd.policy.")}
BATCHES = [{k.split(".", 1)[1]: torch.from_numpy(G[k]) for k in G.files if k.startswith("batch%d." % s)} for s in range(STEPS)]
K_TOL, FLOOR = 4.0, 1e-6
WORST = {}
LOSSES = ("qf1_loss", "qf2_loss", "vf_loss", "policy_loss")


def _check(group, err, ref_err, what=""):
    ref = max(float(ref_err), FLOOR)
    WORST[group] = max(WORST.get(group, 0.0), err / ref)
    print("%-20s %-36s err %.3e  ref32_err %.3e  ratio %.3f" % (group, what, err, float(ref_err), err / ref))
    assert err <= K_TOL * ref, (group, what, err, K_TOL * ref)


def _trainer(critic_sd, policy_sd, dev, sizes=(Z, A, H, P), **kw):
    from s2p_amd.iql import CriticSLAC, IQLTrainer, Qfunction, TanhGaussianPolicy, Vfunction
    z, a, h, p = sizes
    q = [Qfunction(hidden_sizes=[h, h], output_size=1, input_size=z + a) for _ in range(4)]
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=[h, h], output_size=1, input_size=z), device=dev)
    policy = TanhGaussianPolicy(hidden_sizes=[h, h], obs_dim=p, action_dim=a, device=dev)
    if critic_sd is not None:
        critic.load_state_dict(critic_sd, strict=True)
        policy.load_state_dict(policy_sd, strict=True)
    cfg = dict(discount=0.99, policy_lr=1e-4, qf_lr=3e-4, reward_scale=1, soft_target_tau=0.005, beta=0.1, quantile=0.7, clip_score=100,
               target_update_period=2)
    cfg.update(kw)
    return IQLTrainer(None, policy, critic=critic, **cfg)


def _step(tr, b):
    return tr.train_from_latents(b["z"], b["next_z"], b["action"], b["policy_input"], b["rewards"], b["terminals"])


def _grads(tr):
    g = {"grad." + k: v for k, v in tr.critic.grads().items()}
    g.update(("grad.policy." + k, v) for k, v in tr.policy.grads().items())
    return g


def _group(k):
    head = "policy" if ".policy." in k else "critic"
    return "%s %s" % (head, "gradients" if k.startswith("grad.") else "step-2 updates")


def _adam_replay(init, grads_per_step, cfg=R.CFG):
    """torch.optim.Adam (eps 1e-8, betas (0.9, 0.999)) and the Polyak updates in fp64 from given per-step gradients."""
    p = {k: v.double().clone() for k, v in init.items()}
    m, v = {}, {}
    for s, grads in enumerate(grads_per_step):
        for gk, g in grads.items():
            k, g = gk[5:], g.double()
            lr = cfg["policy_lr"] if k.startswith("policy.") else cfg["qf_lr"]
            m[k] = 0.9 * m.get(k, 0.0) + 0.1 * g
            v[k] = 0.999 * v.get(k, 0.0) + 0.001 * g * g
            p[k] -= lr / (1 - 0.9 ** (s + 1)) * m[k] / (v[k].sqrt() / (1 - 0.999 ** (s + 1)) ** 0.5 + 1e-8)
        if s % cfg["target_update_period"] == 0:
            for k in [k for k in p if k.startswith(("qf1.", "qf2."))]:
                p["target_" + k] = p["target_" + k] * (1.0 - cfg["soft_target_tau"]) + p[k] * cfg["soft_target_tau"]
    return p


def _check_run(tr, batches, want0, want_final, init):
    """want0: name -> (fp64 value, ref32_err) of the step-0 losses / weights / gradients; want_final: key -> (fp64 value,
    update_ref32_err), or None: the step-2 parameters against the fp64 replay of the optimizer steps from the path's own gradients
    (module docstring); init: key -> initial value."""
    own = []
    for s, b in enumerate(batches):
        losses = _step(tr, b).cpu().double()
        if want_final is None:
            own.append(_grads(tr))
        if s == 0:
            for i, k in enumerate(LOSSES):
                _check("losses", abs(float(losses[i]) - float(want0[k][0])) / abs(float(want0[k][0])), want0[k][1], k)
            w = tr._buf[len(b["z"])]["weights"].cpu()
            _check("weights", R.rel_max(w, want0["weights"][0]), want0["weights"][1], "weights")
            grads = _grads(tr)
            assert sorted(grads) == sorted(k for k in want0 if k.startswith("grad."))       # none for the targets
            for k, g in grads.items():
                assert float(g.abs().max()) > 0, k
                _check(_group(k), R.rel_max(g, want0[k][0]), want0[k][1], k)
    assert tr._n_train_steps_total == len(batches)
    got = dict(tr.critic.state_dict())
    got.update(("policy." + k, v) for k, v in tr.policy.state_dict().items())
    if want_final is None:
        replay = _adam_replay(init, own)
        assert sorted(got) == sorted(replay)
        for k, ref in replay.items():
            upd = ref - init[k].double()
            assert float(upd.abs().max()) > 0, k
            half_ulp = 2.0 ** (math.floor(math.log2(float(ref.abs().max()))) - 24)
            _check("optimizer replay", float((got[k].double() - ref).abs().max() / upd.abs().max()),
                   len(batches) * half_ulp / float(upd.abs().max()) + 2.0 ** -24 / (1 - 0.999) / 2, "final." + k)
        return
    assert sorted(got) == sorted(want_final)
    for k, (ref, err) in want_final.items():
        upd = torch.as_tensor(ref).double() - init[k].double()
        _check(_group("final." + k), float((got[k].double() - torch.as_tensor(ref).double()).abs().max() / upd.abs().max()), err, "final." + k)


def test_three_steps_against_the_real_trainer(hip_device):
    tr = _trainer(CRITIC_SD, POLICY_SD, hip_device)
    keys = [k for k in G.files if k.endswith(".ref32_err")]
    want0 = {k[:-10]: (G[k[:-10]], G[k]) for k in keys}
    finals = {k[6:-17]: (G[k[:-17]], G[k]) for k in G.files if k.startswith("final.") and k.endswith(".update_ref32_err")}
    assert len(finals) == len(CRITIC_SD) + len(POLICY_SD) and set(LOSSES) < set(want0)
    init = dict(CRITIC_SD)
    init.update(("policy." + k, v) for k, v in POLICY_SD.items())
    _check_run(tr, BATCHES, want0, finals, init)
    stats = tr.eval_statistics
    assert list(stats) == ["QF1 Loss", "QF2 Loss", "VF Loss", "Policy Loss"] and abs(stats["QF1 Loss"] - float(G["qf1_loss"])) < 1e-4


def test_production_widths_against_the_restatement(hip_device):
    """Z 288, A 6, H 1024, P 2090, B 256: K = 294 -> 296 and 2090 -> 2092 (padded), 512 vf rows, every tile full."""
    z, a, h, p, b = 288, 6, 1024, 2090, 256
    critic, policy = R.init_params(z, a, h, p, seed=5, last_scale=30.0)
    batches = [R.make_batch(b, z, a, p, 200 + s, terminals=(s == 1), scale=0.5, extreme_rows=None) for s in range(3)]
    step64, step32 = R.train(critic, policy, batches[:1], torch.float64)[0], R.train(critic, policy, batches[:1], torch.float32)[0]
    want0 = {k: (step64[k], R.rel_max(step32[k], step64[k])) for k in step64}
    init = dict(critic)
    init.update(("policy." + k, v) for k, v in policy.items())
    _check_run(_trainer(critic, policy, hip_device, (z, a, h, p)), batches, want0, None, init)


def test_state_dict_round_trip_and_strict_load(hip_device, tmp_path):
    tr = _trainer(CRITIC_SD, POLICY_SD, hip_device)
    assert list(tr.critic.state_dict()) == [str(k) for k in G["critic_keys"]] and list(tr.policy.state_dict()) == [str(k) for k in G["policy_keys"]]
    for k, v in tr.critic.state_dict().items():
        assert torch.equal(v, CRITIC_SD[k]), k                                  # a reference-layout state_dict loads strict and comes back
    for k, v in tr.policy.state_dict().items():
        assert torch.equal(v, POLICY_SD[k]), k
    with pytest.raises(RuntimeError):
        tr.critic.load_state_dict({k: v for k, v in CRITIC_SD.items() if k != "vf.fc0.bias"}, strict=True)
    with pytest.raises(RuntimeError):
        tr.policy.load_state_dict(dict(POLICY_SD, extra=torch.zeros(1)), strict=True)
    _step(tr, BATCHES[0])
    _step(tr, BATCHES[1])
    torch.save(tr.get_snapshot(), tmp_path / "snap.pth")
    tr2 = _trainer(None, None, hip_device).load_state_dict(torch.load(tmp_path / "snap.pth"))
    assert tr2._n_train_steps_total == 2
    osd = tr.state_dict()["critic_optimizer"]
    assert len(osd["param_groups"][0]["params"]) == 30 and len(osd["state"]) == 18 and float(osd["state"][0]["step"]) == 2   # no state for the targets
    l1, l2 = _step(tr, BATCHES[2]).clone(), _step(tr2, BATCHES[2]).clone()
    assert torch.equal(l1, l2)
    for a, b in ((tr.critic.state_dict(), tr2.critic.state_dict()), (tr.policy.state_dict(), tr2.policy.state_dict())):
        assert all(torch.equal(a[k], b[k]) for k in a)                            # the restored trainer continues bit for bit
    with torch.no_grad():
        act = tr.policy.act(BATCHES[0]["policy_input"].to(hip_device))
    mean = R.mlp_forward({k: v.double() for k, v in tr.policy.state_dict().items()}, "", BATCHES[0]["policy_input"].double())[0]
    assert tuple(act.shape) == (B, A) and R.rel_max(act.cpu(), torch.tanh(mean)) < 1e-5


@pytest.mark.parametrize("freeze", [True, False])
def test_train_from_torch_on_a_tiny_real_buffer(hip_device, freeze):
    import slac_buffer_ref as SB
    from s2p_amd.slac_algo import SlacAlgorithm
    algo = SlacAlgorithm((3, 100, 100), (SB.A,), 1, hip_device, seed=0, batch_size_latent=2, buffer_size=32, num_sequences=SB.S, frame_capacity=128)
    algo.load_data_in_buffer(SB.real_dataset(2, 12, 100, 100), **dict(SB.LOAD_ARGS["real"], data_num=24))
    tr = _trainer(None, None, hip_device, (288, SB.A, 64, SB.S * 256 + (SB.S - 1) * SB.A), slac_algo=algo, freeze_slac=freeze)
    before = [p.detach().clone() for p in algo.latent.parameters()]
    c0 = tr.critic.state_dict()
    for _ in range(3):
        losses = tr.train_from_torch(algo.buffer.random_batch(4))
        assert bool(torch.isfinite(losses).all())
    assert tr._n_train_steps_total == 3 and algo.learning_steps_latent == (0 if freeze else 3)
    same = [torch.equal(p, q) for p, q in zip(algo.latent.parameters(), before)]
    assert all(same) if freeze else not any(same)
    c1 = tr.critic.state_dict()
    assert all(not torch.equal(c0[k], c1[k]) for k in c0 if k.endswith("weight"))


def test_the_step_and_act_run_the_policy_through_one_table_builder(hip_device):
    """The trainer's grouped forward (the policy as group 5 of 6, then alone on the narrow last layer) and `TanhGaussianPolicy.act`
    (one group a launch, two ping-pong buffers) build their groups in s2p_amd/mlp.py and call the same kernels on the same operands:
    the step's pre-update policy output is `act`'s, bit for bit.  Hidden widths off the 32 / 64 tile, a partial row tile."""
    from s2p_amd.iql import CriticSLAC, IQLTrainer, Qfunction, TanhGaussianPolicy, Vfunction
    z, a, p, b, hid = 10, 3, 13, 37, [20, 24]
    torch.manual_seed(11)
    q = [Qfunction(hidden_sizes=hid, output_size=1, input_size=z + a) for _ in range(4)]
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=hid, output_size=1, input_size=z), device=hip_device)
    policy = TanhGaussianPolicy(hidden_sizes=hid, obs_dim=p, action_dim=a, device=hip_device)
    before = policy.state_dict()
    tr = IQLTrainer(None, policy, critic=critic, **R.CFG)
    batch = R.make_batch(b, z, a, p, 5, terminals=True)
    _step(tr, batch)
    raw = tr._buf[b]["raw"]
    assert not torch.equal(policy.state_dict()["fc0.weight"], before["fc0.weight"])            # the step did move the policy
    other = TanhGaussianPolicy(hidden_sizes=hid, obs_dim=p, action_dim=a, device=hip_device).load_state_dict(before)
    got = other.act(batch["policy_input"])
    assert got.shape == (b, a) and float(got.abs().max()) > 0
    assert torch.equal(torch.tanh(raw[:, :a]), got)


def test_act_keeps_its_scratch_buffers_between_calls(hip_device):
    """`act` caches a table of bare addresses per batch size, so the cached entry must own every buffer the table names: tensors
    allocated between two calls (of the scratch buffers' very size, which a caching allocator would hand freed memory to first)
    keep their values, an earlier result the caller still holds keeps its own, and the second call returns the first's result."""
    from s2p_amd.iql import TanhGaussianPolicy
    p, a, b, hid = 13, 3, 37, [20, 24]
    torch.manual_seed(12)
    policy = TanhGaussianPolicy(hidden_sizes=hid, obs_dim=p, action_dim=a, device=hip_device)
    x = torch.randn(b, p, generator=torch.Generator().manual_seed(6))
    first = policy.act(x)
    kept = first.clone()
    net, table = policy._eval[b]
    owned = {t.data_ptr() for t in [net.x, net.out] + net.act}
    named = {g.x for gs, G, N, act in table for g in gs[:G]} | {g.pre or g.act for gs, G, N, act in table for g in gs[:G]}
    assert named <= owned and len(named) == 4                                                  # xp, two scratch buffers, raw
    sentinels = [torch.full((b, max(hid)), 7.0, device=hip_device) for _ in range(4)] + [torch.full((b, 2 * a), 7.0, device=hip_device)]
    assert not {t.data_ptr() for t in sentinels} & owned
    second = policy.act(x)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in sentinels)
    assert torch.equal(first, kept) and torch.equal(second, kept)


def test_zz_report_worst_ratios(hip_device):
    print("\nworst deviation / max(ref32_err, 1e-6) per group:", {k: round(v, 3) for k, v in WORST.items()})
    assert WORST and max(WORST.values()) <= K_TOL
