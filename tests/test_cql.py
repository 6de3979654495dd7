"""N3e -- CQL on SLAC latents, the host side (no device): the plain-torch restatement tests/cql_ref.py against the fixture of the
REAL reference trainer (tests/golden/cql_golden_v1.npz, made by tests/golden/make_golden_cql.py) to 1e-9 in fp64, the state_dict
layout against the key / shape lists recorded from the real modules, and the options the trainer refuses."""
import os

import numpy as np
import pytest
import torch

import cql_ref as C
import iql_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "cql_golden_v1.npz"))
Z, A, H, P, B, RN, STEPS = (int(v) for v in G["sizes"])
CRITIC_SD = {k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("sd.") and not k.startswith("sd.policy.")}
POLICY_SD = {k[10:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("sd.policy.")}
BATCHES = [{k.split(".", 1)[1]: torch.from_numpy(G[k]) for k in G.files if k.startswith("batch%d." % s)} for s in range(STEPS)]
NOISES = [{k.split(".", 1)[1]: torch.from_numpy(G[k]) for k in G.files if k.startswith("noise%d." % s)} for s in range(STEPS)]


def test_restatement_reproduces_the_real_trainer_in_fp64():
    assert C.CFG["num_random"] == RN and all(sorted(n) == sorted(C.NOISE) for n in NOISES)
    per_step, (critic, policy, log_alpha) = C.train(CRITIC_SD, POLICY_SD, BATCHES, NOISES, torch.float64)
    worst, seen = 0.0, 0
    for k in [k for k in G.files if k.startswith("step") and not k.endswith("ref32_err")]:
        s, name = int(k[4]), k[6:]
        assert s < 2 and name in per_step[s], k
        worst, seen = max(worst, R.rel_max(per_step[s][name], G[k])), seen + 1
    n_grads = sum(1 for k in CRITIC_SD if k.startswith(("qf1.", "qf2."))) + len(POLICY_SD)
    assert seen == 2 * (n_grads + len(C.STATS))                                    # steps 0 and 1: every statistic, every gradient
    finals = [k for k in G.files if k.startswith("final.") and not k.endswith("ref32_err")]
    assert len(finals) == len(critic) + len(policy) + 1
    for k in finals:
        want = torch.from_numpy(G[k])
        if k == "final.log_alpha":
            got, init = log_alpha, torch.zeros(1)
        else:
            got = policy[k[13:]] if k.startswith("final.policy.") else critic[k[6:]]
            init = POLICY_SD[k[13:]] if k.startswith("final.policy.") else CRITIC_SD[k[6:]]
        upd = float((want - init.double()).abs().max())
        if k.startswith("final.vf."):
            assert upd == 0.0 and torch.equal(got, want)                            # vf takes part in no loss
            continue
        assert upd > 0, k                                                           # every other parameter moved, the targets too
        worst = max(worst, float((got - want).abs().max() / upd))                   # relative to the UPDATE
    print("restatement vs the real trainer, fp64: worst relative deviation %.3e" % worst)
    assert worst < 1e-9


def test_fixture_exercises_every_branch():
    c, p = ({k: v.double() for k, v in sd.items()} for sd in (CRITIC_SD, POLICY_SD))
    b, n = ({k: v.double() for k, v in d.items()} for d in (BATCHES[0], NOISES[0]))
    new_a, _, _, raw_ls = C.sample(p, b["policy_input"], n["eps0"])
    q1, q2 = C.q_of(c, "qf1", b["z"], new_a), C.q_of(c, "qf2", b["z"], new_a)
    assert (q1 < q2).any() and (q2 < q1).any()
    outside = (raw_ls > 2) | (raw_ls < -20)
    assert outside.any() and (~outside).any()
    assert float(C.q_of(c, "qf1", b["z"].repeat_interleave(RN, 0), n["uniform"]).view(B, RN).std(1).min()) > 1e-3
    assert any(float(x["terminals"].sum()) > 0 for x in BATCHES)
    assert C.CFG["policy_eval_start"] == 2                                          # step 0 clones, steps 1 and 2 take the SAC loss
    assert float(G["step0.policy_loss"]) != float(G["step0.Policy Loss"])


def _nets(device=None):
    from s2p_amd.cql import CriticSLAC, Qfunction, TanhGaussianPolicy, Vfunction
    q = [Qfunction(hidden_sizes=[H, H], output_size=1, input_size=Z + A) for _ in range(4)]
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=[H, H], output_size=1, input_size=Z), device=device)
    return critic, TanhGaussianPolicy(hidden_sizes=[H, H], obs_dim=P, action_dim=A, device=device)


def test_state_dict_layout_is_the_real_modules():
    critic, policy = _nets()
    for sd, keys, shapes in ((critic.state_dict(), G["critic_keys"], G["critic_shapes"]), (policy.state_dict(), G["policy_keys"], G["policy_shapes"])):
        assert list(sd) == [str(k) for k in keys]
        assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in shapes]
    assert list(critic.keys()) == R.critic_keys(2) and list(policy.keys()) == R.policy_keys(2)


@pytest.mark.parametrize("kw", [dict(with_lagrange=True), dict(max_q_backup=True), dict(num_qs=1), dict(min_q_version=2),
                                dict(curl_learning=True), dict(image_rl=False), dict(slac_representation=False),
                                dict(policy_weight_decay=1e-4), dict(q_weight_decay=1e-4)])
def test_refused_options_raise(kw):
    from s2p_amd.cql import CQLTrainer
    critic, policy = _nets()
    with pytest.raises(NotImplementedError):
        CQLTrainer(None, policy, critic=critic, **kw)


def test_a_fixed_std_and_a_cpu_device_are_refused():
    from s2p_amd.cql import CQLTrainer, TanhGaussianPolicy
    with pytest.raises(NotImplementedError):
        TanhGaussianPolicy(hidden_sizes=[H, H], obs_dim=P, action_dim=A, std=0.5, device=None)
    critic, policy = _nets()
    with pytest.raises(ValueError):                                                 # no CPU fallback: nothing of a CPU holder can train
        CQLTrainer(None, policy, critic=critic)
    with pytest.raises(ValueError):
        CQLTrainer(None, policy, critic=critic, slac_policy_input_type="pixels")


def test_cli_arguments():
    import train_cql as T
    a = T.parse_args(["--real", "r.npz", "--latent_dir", "d", "--steps", "5", "--out", "o"])
    assert (a.num_random, a.min_q_weight, a.temp, a.policy_eval_start, a.deterministic_backup) == (10, 5.0, 1.0, 40000, False)
    assert (a.batch_size, a.hidden, a.freeze_slac, a.slac_policy_input_type) == (256, 1024, False, "feature_action")   # train_iql.py's options
    a = T.parse_args(["--real", "r.npz", "--latent_dir", "d", "--steps", "5", "--out", "o", "--num_random", "4", "--temp", "0.5",
                      "--policy_eval_start", "0", "--deterministic_backup", "--freeze_slac"])
    assert (a.num_random, a.temp, a.policy_eval_start, a.deterministic_backup, a.freeze_slac) == (4, 0.5, 0, True, True)
    for bad in (["--num_random", "0"], ["--temp", "0"], ["--steps", "-1"]):
        with pytest.raises(SystemExit):
            T.parse_args(["--real", "r.npz", "--latent_dir", "d", "--out", "o"] + (bad if bad[0] == "--steps" else ["--steps", "1"] + bad))
