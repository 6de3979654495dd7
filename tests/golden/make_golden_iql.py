"""Generates tests/golden/iql_golden_v1.npz by RUNNING THE REAL REFERENCE trainer (`rlkit.torch.sac.iql_trainer.IQLTrainer` with
`examples/iql/custom_networks.{Qfunction, Vfunction, CriticSLAC, TanhGaussianPolicyWithEncoder}`, importable in the build container
only) on the CPU in fp64 and in fp32, in its shipped SLAC configuration (`examples/iql/mujoco_finetune.py:91-119`).  `torchvision`,
`torchvision.models` and `gtimer` are empty stand-in modules; `slac_algo` is a stand-in whose `prepare_batch` returns the given
latents, with `freeze_slac=True`.  The fixture holds data only: sizes Z 40, A 3, H 64, P 50, B 37; the initial state_dicts (last
layers scaled up: the reference's +-3e-3 init makes vf and the advantages degenerate); three batches; after step 0 the four losses,
every parameter gradient and the advantage weights; after step 2 every parameter, targets included; each with `ref32_err`, the
deviation of the trainer's own fp32 run from its fp64 run (relative to the fp64 maximum); the key / shape lists of the real modules.
Run:  python tests/golden/make_golden_iql.py"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for name in ("torchvision", "torchvision.models", "gtimer"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["torchvision"].models = sys.modules["torchvision.models"]
sys.modules["torchvision.models"].resnet18 = None
sys.path.insert(0, "/root/reference")
sys.path.insert(0, "/root/reference/examples/iql")
sys.path.insert(0, os.path.dirname(HERE))
from rlkit.torch.sac.iql_trainer import IQLTrainer  # noqa: E402  (the real reference)
from custom_networks import CriticSLAC, Qfunction, TanhGaussianPolicyWithEncoder, Vfunction  # noqa: E402
import iql_ref as R  # noqa: E402

Z, A, H, P, B, STEPS = 40, 3, 64, 50, 37, 3


class SlacStandIn:
    def prepare_batch(self, obs, actions):
        return obs["z"], obs["next_z"], actions, obs["feature_action"], None


def build(seed):
    torch.manual_seed(seed)
    q = [Qfunction(input_size=Z + A, output_size=1, hidden_sizes=[H, H]) for _ in range(4)]
    vf = Vfunction(input_size=Z, output_size=1, hidden_sizes=[H, H])
    policy = TanhGaussianPolicyWithEncoder(obs_dim=P, action_dim=A, hidden_sizes=[H, H], encoder=None)
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=vf)
    with torch.no_grad():       # larger last layers: vf_err of both signs, exp(adv / beta) on both sides of the clip, log stds beyond the clamp
        for m in q + [vf]:
            m.last_fc.weight.mul_(600.0)
        policy.last_fc.weight.mul_(300.0)
        policy.last_fc_log_std.weight.mul_(1500.0)
        policy.last_fc_log_std.bias.add_(1.0)
    return critic, policy


def trainer_of(critic, policy):
    t = IQLTrainer(env=None, policy=policy, qf1=critic.qf1, qf2=critic.qf2, vf=critic.vf, target_qf1=critic.target_qf1,
                   target_qf2=critic.target_qf2, discount=0.99, policy_lr=1e-4, qf_lr=3e-4, reward_scale=1, soft_target_tau=0.005,
                   policy_weight_decay=0, q_weight_decay=0, beta=1.0 / 10, quantile=0.7, clip_score=100, image_rl=True,
                   policy_update_period=1, q_update_period=1, target_update_period=2, training_start_steps=0, critic=critic,
                   slac_representation=True, slac_algo=SlacStandIn(), freeze_slac=True, slac_update_period=1,
                   slac_policy_input_type="feature_action")
    t.replay_buffer = []
    return t


def run(critic, policy, batches, dtype):
    critic, policy = copy.deepcopy(critic).to(dtype), copy.deepcopy(policy).to(dtype)
    t = trainer_of(critic, policy)
    out = {}
    for step, b in enumerate(batches):
        b = {k: v.to(dtype) for k, v in b.items()}
        if step == 0:
            with torch.no_grad():
                _, _, tq1, tq2, v = critic(b["z"], b["action"])
                out["weights"] = torch.clamp(torch.exp((torch.min(tq1, tq2) - v) / t.beta), max=t.clip_score)[:, 0]
        t._need_to_update_eval_statistics = True
        t.train_from_torch(dict(rewards=b["rewards"][:, None], terminals=b["terminals"][:, None], actions=b["action"],
                                observations=dict(z=b["z"], next_z=b["next_z"], feature_action=b["policy_input"])))
        for k, v in list(critic.named_parameters()) + [("policy." + k, v) for k, v in policy.named_parameters()]:
            assert (v.grad is None) == k.startswith("target"), k              # the targets receive no gradient
            if v.grad is not None:
                out["step%d.grad.%s" % (step, k)] = v.grad.detach().clone()
        if step == 0:
            for k, name in (("qf1_loss", "QF1 Loss"), ("qf2_loss", "QF2 Loss"), ("vf_loss", "VF Loss"), ("policy_loss", "Policy Loss")):
                out[k] = torch.tensor(float(t.eval_statistics[name]), dtype=torch.float64)
    assert t._n_train_steps_total == STEPS
    for k, v in critic.state_dict().items():
        out["final." + k] = v.detach().clone()
    for k, v in policy.state_dict().items():
        out["final.policy." + k] = v.detach().clone()
    return out


def main():
    critic, policy = build(20261018)
    # The reference's u = log(1 + v) / 2 - log(1 - v) / 2 is unstable in fp32 at the clamp (1 - 0.999999 carries 6 % rounding
    # error), so the actions beyond the clamp sit in batch 0 only, in the two rows of the smallest advantage weights: the branch
    # runs, and the fp32 runs of the three steps still agree well enough to pin the Adam steps.
    csd0, psd0 = ({k: v.double() for k, v in m.state_dict().items()} for m in (critic, policy))
    b0 = R.make_batch(B, Z, A, P, 100, extreme_rows=None)
    rows = torch.argsort(R.losses(csd0, psd0, {k: v.double() for k, v in b0.items()})["weights"])[:2].tolist()
    batches = [R.make_batch(B, Z, A, P, 100 + s, terminals=(s == 1), extreme_rows=rows if s == 0 else None) for s in range(STEPS)]
    out = {"sizes": np.array([Z, A, H, P, B, STEPS])}
    csd, psd = critic.state_dict(), policy.state_dict()
    out["critic_keys"], out["policy_keys"] = np.array(list(csd.keys())), np.array(list(psd.keys()))
    out["critic_shapes"] = np.array([",".join(map(str, v.shape)) for v in csd.values()])
    out["policy_shapes"] = np.array([",".join(map(str, v.shape)) for v in psd.values()])
    out.update(("sd." + k, v.numpy()) for k, v in csd.items())
    out.update(("sd.policy." + k, v.numpy()) for k, v in psd.items())
    for s, b in enumerate(batches):
        out.update(("batch%d.%s" % (s, k), v.numpy()) for k, v in b.items())

    # no branch is dead (checked on the restatement's intermediate values, which the test pins to this fixture at 1e-9)
    c64, p64 = ({k: v.double() for k, v in sd.items()} for sd in (csd, psd))
    for s, b in enumerate(batches):
        o = R.losses(c64, p64, {k: v.double() for k, v in b.items()})
        if s == 0:
            assert (o["vf_err"] > 0).any() and (o["vf_err"] < 0).any(), "vf_err of both signs"
            assert (o["exp_adv_unclipped"] > 100).any() and (o["exp_adv_unclipped"] < 100).any(), "both sides of the clip"
            assert (o["raw_log_std"] > 2).any() or (o["raw_log_std"] < -20).any(), "a raw log sigma outside the clamp"
            assert ((o["raw_log_std"] >= -20) & (o["raw_log_std"] <= 2)).any()
            print("step 0: vf_err > 0 in %d / %d rows, clipped weights %d, log stds outside the clamp %d / %d" % (
                int((o["vf_err"] > 0).sum()), B, int((o["exp_adv_unclipped"] > 100).sum()),
                int(((o["raw_log_std"] > 2) | (o["raw_log_std"] < -20)).sum()), B * A))
    assert (batches[0]["action"].abs() > 0.999999).any(), "an action beyond the clamp"
    assert any(float(b["terminals"].sum()) > 0 for b in batches), "non-zero terminals in one batch"

    r64, r32 = run(critic, policy, batches, torch.float64), run(critic, policy, batches, torch.float32)
    for k in r64:
        if k.startswith("step") and not k.startswith("step0"):
            continue                              # (the later steps' gradients are not stored)
        key = k[6:] if k.startswith("step0.") else k
        out[key] = r64[k].numpy().astype(np.float64)       # fp64 throughout: tests/test_iql.py pins the restatement to 1e-9
        out[key + ".ref32_err"] = np.float64(R.rel_max(r32[k], r64[k]))
    # The first Adam steps move an element by about lr whatever the size of its gradient (lr g / (|g| + eps)), so an element whose
    # gradient CANCELS to near zero could differ by up to lr between two fp32 runs.  This fixture has no such element: the
    # trainer's own fp32 run reproduces every step-2 parameter's UPDATE (final - initial, the quantity the steps produce) to the
    # `update_ref32_err` stored here, relative to the tensor's largest update, over the WHOLE tensor -- asserted below to stay under
    # 1e-3 of the update, so no element is left out of the comparison.  (The smallest gradients, ~1e-13, belong to ReLU units that
    # are active only on rows of a tiny advantage weight: products, not cancellations, so their relative precision is full.)
    init = {"final." + k: v for k, v in csd.items()}
    init.update(("final.policy." + k, v) for k, v in psd.items())
    worst = 0.0
    for k in [k for k in r64 if k.startswith("final.")]:
        upd64, upd32 = r64[k] - init[k].double(), r32[k].double() - init[k].double()
        out[k + ".update_ref32_err"] = np.float64(float((upd32 - upd64).abs().max() / upd64.abs().max()))
        worst = max(worst, float(out[k + ".update_ref32_err"]))
        print("%-40s largest update %.3e  update ref32_err %.3e" % (k, float(upd64.abs().max()), out[k + ".update_ref32_err"]))
    assert worst < 1e-3, worst
    print({k: float(out[k]) for k in ("qf1_loss", "qf2_loss", "vf_loss", "policy_loss")},
          {k: float(out[k + ".ref32_err"]) for k in ("qf1_loss", "qf2_loss", "vf_loss", "policy_loss", "weights")})
    path = os.path.join(HERE, "iql_golden_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
