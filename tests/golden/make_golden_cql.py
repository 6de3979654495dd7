"""Generates tests/golden/cql_golden_v1.npz by RUNNING THE REAL REFERENCE trainer (`rlkit.torch.sac.cql_trainer.CQLTrainer` with
`examples/iql/custom_networks.{Qfunction, Vfunction, CriticSLAC, TanhGaussianPolicyWithEncoder}`, importable in the build container
only) on the CPU in fp64 and in fp32, in its shipped SLAC configuration (`examples/iql/mujoco_finetune.py:120-143`) except
`policy_eval_start = 2` and `num_random = 4`: step 0 takes the behaviour-cloning branch, steps 1-2 the SAC branch.  The stand-ins are
those of make_golden_iql.py (empty `torchvision`, `torchvision.models`, `gtimer`; a `slac_algo` whose `prepare_batch` returns the
given latents, `freeze_slac=True`); `batch['observations']` is a dict with a `shape`, which the trainer reads.  The fp64 run holds
`log_alpha` in fp64 too (the reference creates it in fp32 whatever the networks' precision).

The noise.  The reference draws it in fp32 in both precisions (`ptu.zeros / ones`, `torch.FloatTensor(..).uniform_`), so one
`torch.manual_seed` per step gives both runs the same draws; they are replayed here in the trainer's own order (eps0, eps1, uniform,
eps2, eps3) by the same calls after the same seed, stored, and PROVEN by the assertion that tests/cql_ref.py fed with them
reproduces the trainer to 1e-9 in fp64.

The fixture holds data only: sizes; the initial state_dicts (last layers scaled up); three batches and their noise; after steps 0
and 1 the statistics of cql_ref.STATS and every critic and policy gradient (the policy's captured at `policy_optimizer.step()`:
afterwards `.grad` also holds the discarded share of the critic loss); after step 2 every parameter (targets included) and
`log_alpha`; each with `ref32_err`, and the final parameters with `update_ref32_err` over whole tensors.
Run:  python tests/golden/make_golden_cql.py"""
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
from rlkit.torch.sac.cql_trainer import CQLTrainer  # noqa: E402  (the real reference)
from custom_networks import CriticSLAC, Qfunction, TanhGaussianPolicyWithEncoder, Vfunction  # noqa: E402
import cql_ref as C  # noqa: E402
import iql_ref as R  # noqa: E402

Z, A, H, P, B, RN, STEPS = 40, 3, 64, 50, 37, 4, 3
SEED = 4242
KEEP = {"QF1 Loss", "QF2 Loss", "min QF1 Loss", "min QF2 Loss", "Std QF1 values", "Std QF2 values", "Policy Loss", "Alpha", "Alpha Loss"}


class SlacStandIn:
    def prepare_batch(self, obs, actions):
        return obs["z"], obs["next_z"], actions, obs["feature_action"], obs["next_feature_action"]


class Obs(dict):
    @property
    def shape(self):
        return self["z"].shape


class Env:
    class action_space:
        shape = (A,)


def build(seed):
    torch.manual_seed(seed)
    q = [Qfunction(input_size=Z + A, output_size=1, hidden_sizes=[H, H]) for _ in range(4)]
    vf = Vfunction(input_size=Z, output_size=1, hidden_sizes=[H, H])
    policy = TanhGaussianPolicyWithEncoder(obs_dim=P, action_dim=A, hidden_sizes=[H, H], encoder=None)
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=vf)
    with torch.no_grad():       # larger last layers: a log-sum-exp that is not flat, min(q1, q2) from both networks, log stds beyond the clamp
        for m in q:
            m.last_fc.weight.mul_(600.0)
        policy.last_fc.weight.mul_(300.0)
        policy.last_fc_log_std.weight.mul_(1500.0)
        policy.last_fc_log_std.bias.add_(1.0)
    return critic, policy


def trainer_of(critic, policy):
    return CQLTrainer(env=Env(), policy=policy, qf1=critic.qf1, qf2=critic.qf2, target_qf1=critic.target_qf1,
                      target_qf2=critic.target_qf2, discount=0.99, soft_target_tau=5e-3, policy_lr=1e-4, qf_lr=3e-4, reward_scale=1,
                      use_automatic_entropy_tuning=True, policy_eval_start=2, num_qs=2, temp=1.0, min_q_version=3, min_q_weight=5.0,
                      with_lagrange=False, lagrange_thresh=-1.0, num_random=RN, max_q_backup=False, deterministic_backup=False,
                      image_rl=True, critic=critic, slac_representation=True, slac_algo=SlacStandIn(), freeze_slac=True,
                      slac_update_period=1, slac_policy_input_type="feature_action")


def replay_noise(step):
    """The trainer's five draws of a step, by its own calls in its own order after the same seed."""
    torch.manual_seed(SEED + step)

    def normal(rows):
        return torch.distributions.Independent(torch.distributions.Normal(torch.zeros(rows, A), torch.ones(rows, A)), 1).sample()

    n = {"eps0": normal(B), "eps1": normal(B)}
    n["uniform"] = torch.FloatTensor(B * RN, A).uniform_(-1, 1)
    n["eps2"], n["eps3"] = normal(B * RN), normal(B * RN)
    return n


def run(critic, policy, batches, dtype):
    critic, policy = copy.deepcopy(critic).to(dtype), copy.deepcopy(policy).to(dtype)
    t = trainer_of(critic, policy)
    t.log_alpha.data = t.log_alpha.data.to(dtype)
    out, seen = {}, {}
    step_of_policy = t.policy_optimizer.step

    def policy_step(*a, **k):                     # the policy's gradients as its optimizer sees them
        seen["grads"] = {n: p.grad.detach().clone() for n, p in policy.named_parameters()}
        return step_of_policy(*a, **k)

    t.policy_optimizer.step = policy_step
    backward = torch.Tensor.backward

    def recording_backward(self, *a, **k):        # the three losses of a step in order: alpha, policy, critic
        seen.setdefault("losses", []).append(self.detach().clone().reshape(()))
        return backward(self, *a, **k)

    for step, b in enumerate(batches):
        b = {k: v.to(dtype) for k, v in b.items()}
        t._need_to_update_eval_statistics = True
        seen.clear()
        torch.manual_seed(SEED + step)
        torch.Tensor.backward = recording_backward
        try:
            t.train_from_torch(dict(rewards=b["rewards"][:, None], terminals=b["terminals"][:, None], actions=b["action"],
                                    observations=Obs(z=b["z"], next_z=b["next_z"], feature_action=b["policy_input"],
                                                     next_feature_action=b["policy_next_input"])))
        finally:
            torch.Tensor.backward = backward
        assert len(seen["losses"]) == 3
        if step < 2:
            for k, v in critic.named_parameters():
                assert (v.grad is None) == (not k.startswith(("qf1.", "qf2."))), k     # none for the targets and vf
                if v.grad is not None:
                    out["step%d.grad.%s" % (step, k)] = v.grad.detach().clone()
            for k, g in seen["grads"].items():
                out["step%d.grad.policy.%s" % (step, k)] = g
            for k in KEEP:
                out["step%d.%s" % (step, k)] = torch.tensor(float(t.eval_statistics[k]), dtype=torch.float64)
            out["step%d.policy_loss" % step] = seen["losses"][1].double()
            assert abs(float(seen["losses"][0]) - float(t.eval_statistics["Alpha Loss"])) < 1e-6
    assert t._n_train_steps_total == STEPS and t._current_epoch == STEPS
    for k, v in critic.state_dict().items():
        out["final." + k] = v.detach().clone()
    for k, v in policy.state_dict().items():
        out["final.policy." + k] = v.detach().clone()
    out["final.log_alpha"] = t.log_alpha.detach().clone()
    return out


def main():
    critic, policy = build(20261018)
    batches = [C.make_batch(B, Z, A, P, 300 + s, terminals=(s == 1)) for s in range(STEPS)]
    noises = [replay_noise(s) for s in range(STEPS)]
    out = {"sizes": np.array([Z, A, H, P, B, RN, STEPS])}
    csd, psd = critic.state_dict(), policy.state_dict()
    out["critic_keys"], out["policy_keys"] = np.array(list(csd.keys())), np.array(list(psd.keys()))
    out["critic_shapes"] = np.array([",".join(map(str, v.shape)) for v in csd.values()])
    out["policy_shapes"] = np.array([",".join(map(str, v.shape)) for v in psd.values()])
    out.update(("sd." + k, v.numpy()) for k, v in csd.items())
    out.update(("sd.policy." + k, v.numpy()) for k, v in psd.items())
    for s, (b, n) in enumerate(zip(batches, noises)):
        out.update(("batch%d.%s" % (s, k), v.numpy()) for k, v in b.items())
        out.update(("noise%d.%s" % (s, k), v.numpy()) for k, v in n.items())
    assert any(float(b["terminals"].sum()) > 0 for b in batches), "non-zero terminals in one batch"

    # no branch is dead and no term degenerate (on the restatement's values, which are pinned to the trainer below)
    c64, p64 = ({k: v.double() for k, v in sd.items()} for sd in (csd, psd))
    b0, n0 = ({k: v.double() for k, v in d.items()} for d in (batches[0], noises[0]))
    new_a, _, _, raw_ls = C.sample(p64, b0["policy_input"], n0["eps0"])
    q1, q2 = C.q_of(c64, "qf1", b0["z"], new_a), C.q_of(c64, "qf2", b0["z"], new_a)
    assert (q1 < q2).any() and (q2 < q1).any(), "min(q1, q2) selects each network in some rows"
    outside = (raw_ls > 2) | (raw_ls < -20)
    assert outside.any() and (~outside).any(), "raw log stds outside and inside the clamp"
    zr = b0["z"].repeat_interleave(RN, 0)
    spread = C.q_of(c64, "qf1", zr, n0["uniform"]).view(B, RN).std(1)
    assert float(spread.min()) > 1e-3, "the log-sum-exp is not flat"
    print("q1 < q2 in %d / %d rows; log stds outside the clamp %d / %d; smallest spread of Q over the random actions %.3e" % (
        int((q1 < q2).sum()), B, int(outside.sum()), B * A, float(spread.min())))

    r64, r32 = run(critic, policy, batches, torch.float64), run(critic, policy, batches, torch.float32)
    per_step, (fc, fp, fla) = C.train(csd, psd, batches, noises, torch.float64)
    worst = 0.0
    for k, v in r64.items():
        if k.startswith("step"):
            s, name = int(k[4]), k[6:]
            mine = per_step[s][name]
        elif k == "final.log_alpha":
            mine = fla
        else:
            mine = fp[k[13:]] if k.startswith("final.policy.") else fc[k[6:]]
        worst = max(worst, R.rel_max(mine, v))
        assert R.rel_max(mine, v) < 1e-9, (k, R.rel_max(mine, v))
    print("the restatement with the replayed noise reproduces the trainer to %.2e" % worst)

    for k in r64:
        out[k] = r64[k].numpy().astype(np.float64)
        out[k + ".ref32_err"] = np.float64(R.rel_max(r32[k], r64[k]))
    # as in make_golden_iql.py: the first Adam steps move an element by about lr whatever the size of its gradient, so the final
    # parameters are compared through their UPDATE over the whole tensor, and the trainer's own fp32 run must stay within 1e-3 of it
    init = {"final." + k: v for k, v in csd.items()}
    init.update(("final.policy." + k, v) for k, v in psd.items())
    init["final.log_alpha"] = torch.zeros(1)
    worst = 0.0
    for k in [k for k in r64 if k.startswith("final.")]:
        upd64, upd32 = r64[k] - init[k].double(), r32[k].double() - init[k].double()
        if k.startswith("final.vf."):
            assert float(upd64.abs().max()) == 0.0                 # vf takes part in no loss
            out[k + ".update_ref32_err"] = np.float64(0.0)
            continue
        out[k + ".update_ref32_err"] = np.float64(float((upd32 - upd64).abs().max() / upd64.abs().max()))
        worst = max(worst, float(out[k + ".update_ref32_err"]))
        print("%-40s largest update %.3e  update ref32_err %.3e" % (k, float(upd64.abs().max()), out[k + ".update_ref32_err"]))
    assert worst < 1e-3, worst
    for s in range(2):
        print("step", s, {k: (float(out["step%d.%s" % (s, k)]), float(out["step%d.%s.ref32_err" % (s, k)])) for k in sorted(KEEP) + ["policy_loss"]})
    path = os.path.join(HERE, "cql_golden_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
