"""N3d -- IQL on SLAC latents, the host side (no device): the plain-torch restatement tests/iql_ref.py against the fixture of the
REAL reference trainer (tests/golden/iql_golden_v1.npz, made by tests/golden/make_golden_iql.py) to 1e-9 in fp64, the state_dict
layout of s2p_amd/iql.py against the key / shape lists recorded from the real modules, the init bounds, the step-counter rule of
the target update, and the CLI's argument handling."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import iql_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = np.load(os.path.join(HERE, "golden", "iql_golden_v1.npz"))
Z, A, H, P, B, STEPS = (int(v) for v in G["sizes"])
CRITIC_SD = {k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("sd.") and not k.startswith("sd.policy.")}
POLICY_SD = {k[10:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("sd.policy.")}
BATCHES = [{k.split(".", 1)[1]: torch.from_numpy(G[k]) for k in G.files if k.startswith("batch%d." % s)} for s in range(STEPS)]


def test_restatement_reproduces_the_real_trainer_in_fp64():
    step0, (critic, policy), _ = R.train(CRITIC_SD, POLICY_SD, BATCHES, torch.float64)
    worst = 0.0
    for k in ("qf1_loss", "qf2_loss", "vf_loss", "policy_loss", "weights"):
        worst = max(worst, R.rel_max(step0[k], G[k]))
    grads = [k for k in G.files if k.startswith("grad.") and not k.endswith("ref32_err")]
    assert sorted(grads) == sorted(k for k in step0 if k.startswith("grad."))
    for k in grads:
        worst = max(worst, R.rel_max(step0[k], G[k]))
    finals = [k for k in G.files if k.startswith("final.") and not k.endswith("ref32_err")]
    assert len(finals) == len(critic) + len(policy)
    for k in finals:
        got = policy[k[13:]] if k.startswith("final.policy.") else critic[k[6:]]
        init = POLICY_SD[k[13:]] if k.startswith("final.policy.") else CRITIC_SD[k[6:]]
        want = torch.from_numpy(G[k])
        assert float((want - init.double()).abs().max()) > 0, k                   # every parameter moved, the targets too
        worst = max(worst, float((got - want).abs().max() / (want - init.double()).abs().max()))     # relative to the UPDATE
    print("restatement vs the real trainer, fp64: worst relative deviation %.3e" % worst)
    assert worst < 1e-9


def test_fixture_exercises_every_branch():
    c, p = ({k: v.double() for k, v in sd.items()} for sd in (CRITIC_SD, POLICY_SD))
    o = R.losses(c, p, {k: v.double() for k, v in BATCHES[0].items()})
    assert (o["vf_err"] > 0).any() and (o["vf_err"] < 0).any()
    assert (o["exp_adv_unclipped"] > 100).any() and (o["exp_adv_unclipped"] < 100).any()
    assert ((o["raw_log_std"] > 2) | (o["raw_log_std"] < -20)).any()
    assert (BATCHES[0]["action"].abs() > 0.999999).any()
    assert any(float(b["terminals"].sum()) > 0 for b in BATCHES)


def _nets(hidden=(H, H)):
    from s2p_amd.iql import CriticSLAC, Qfunction, TanhGaussianPolicy, Vfunction
    hid = list(hidden)
    q = [Qfunction(hidden_sizes=hid, output_size=1, input_size=Z + A) for _ in range(4)]
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=hid, output_size=1, input_size=Z), device=None)
    return critic, TanhGaussianPolicy(hidden_sizes=hid, obs_dim=P, action_dim=A, device=None)


def test_state_dict_keys_shapes_and_order_are_the_real_modules():
    critic, policy = _nets()
    for net, keys, shapes, ref_keys in ((critic, G["critic_keys"], G["critic_shapes"], R.critic_keys(2)),
                                        (policy, G["policy_keys"], G["policy_shapes"], R.policy_keys(2))):
        sd = net.state_dict()
        assert list(sd.keys()) == [str(k) for k in keys] == net.keys() == ref_keys
        assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in shapes]


def test_init_bounds():
    torch.manual_seed(3)
    critic, policy = _nets((256, 128))
    sd = critic.state_dict()
    for n in R.NETS:
        for i, out_w in enumerate((256, 128)):
            w, bound = sd["%s.fc%d.weight" % (n, i)], 1 / math.sqrt(out_w)       # fanin_init's quirk: the bound is from the OUT width
            assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound
            assert float(sd["%s.fc%d.bias" % (n, i)].abs().max()) == 0
        assert 0.9 * 3e-3 < float(sd[n + ".last_fc.weight"].abs().max()) <= 3e-3 and float(sd[n + ".last_fc.bias"].abs().max()) == 0
    assert not torch.equal(sd["qf1.fc0.weight"], sd["target_qf1.fc0.weight"])    # the targets are independent inits, not copies
    assert not torch.equal(sd["qf2.fc0.weight"], sd["target_qf2.fc0.weight"])
    ps = policy.state_dict()
    assert 0.8 * 1e-3 < float(ps["last_fc.weight"].abs().max()) <= 1e-3 and float(ps["last_fc.bias"].abs().max()) == 0
    assert 0.8 * 1e-3 < float(ps["last_fc_log_std.weight"].abs().max()) <= 1e-3
    assert 0 < float(ps["last_fc_log_std.bias"].abs().max()) <= 1e-3             # this head's bias is drawn too


def test_target_update_runs_on_the_steps_the_period_divides_counted_from_zero():
    from s2p_amd.iql import target_update_due
    assert [s for s in range(6) if target_update_due(s, 2)] == [0, 2, 4]
    assert all(target_update_due(s, 1) for s in range(4))
    assert [s for s in range(7) if target_update_due(s, 3)] == [0, 3, 6]


def test_no_device_means_no_run():
    from s2p_amd.iql import IQLTrainer, TanhGaussianPolicy
    with pytest.raises(RuntimeError, match="HIP device"):
        TanhGaussianPolicy(hidden_sizes=[32, 32], obs_dim=8, action_dim=2, device="cpu")
    with pytest.raises(ValueError):
        TanhGaussianPolicy(hidden_sizes=[30], obs_dim=8, action_dim=2, device=None)    # hidden widths: multiples of 4 above 16
    critic, policy = _nets()
    with pytest.raises(NotImplementedError):
        IQLTrainer(None, policy, critic=critic, q_weight_decay=0.1)


def test_cli_arguments():
    sys.path.insert(0, ROOT)
    import train_iql as T
    a = T.parse_args(["--real", "r.npz", "--latent_dir", "d", "--steps", "5", "--out", "o"])
    assert (a.freeze_slac, a.slac_policy_input_type, a.bf16, a.batch_size, a.gen) == (False, "feature_action", False, 256, None)
    assert T.policy_input_dim(a, 6) == 8 * 256 + 7 * 6 == 2090
    a = T.parse_args(["--real", "r.npz", "--gen", "g.npz", "--uncertainty_type", "disagreement", "--uncertainty_penalty_lambda", "2",
                      "--latent_dir", "d", "--steps", "0", "--out", "o", "--freeze_slac", "--slac_policy_input_type", "latent_z", "--bf16"])
    assert a.freeze_slac and a.bf16 and a.uncertainty_penalty_lambda == 2.0 and T.policy_input_dim(a, 6) == 288
    assert T.IQL_KWARGS["quantile"] == 0.7 and T.IQL_KWARGS["target_update_period"] == 2 and T.IQL_KWARGS["clip_score"] == 100
    for bad in (["--latent_dir", "d", "--steps", "5", "--out", "o"],                                     # no --real
                ["--real", "r", "--latent_dir", "d", "--steps", "5", "--out", "o", "--slac_policy_input_type", "pixels"],
                ["--real", "r", "--latent_dir", "d", "--steps", "-1", "--out", "o"],
                ["--real", "r", "--latent_dir", "d", "--steps", "1", "--out", "o", "--uncertainty_type", "aleatoric"]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)
