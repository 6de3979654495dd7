"""N3l -- the `mlp_compute` keyword of IQLTrainer and CQLTrainer on the GPU, at Z 40, A 3, H 64, P 50, B 37, R 4.

Default unchanged: mlp_compute="fp32" and no keyword give bitwise equal losses, gradients and weights after two steps, and their
`launches` name no _bf16 entry.  Routing: in bf16 mode every wide launch (N = 64) names a _bf16 entry and every narrow one (N = 1,
N = 2 A) the fp32 entry, for IQL and for CQL in the cloning and the SAC branch.  Network parity: one Q network and the policy trunk
through `mlp.Net` tables in bf16 mode, forward and backward, against the fp64 MLP of tests/mlp_bf16_ref.py by the project's rule --
deviation <= K_TOL x max(ref32_err, 1e-6), K_TOL = 4, ref32_err the helper's own fp32 run against its fp64 run, which carries the same
rounding flips as the device (an fp32 activation next to a bf16 rounding boundary rounds the other way than its fp64 twin).  End to
end: three steps of each trainer in bf16 mode give finite losses, fp32 state_dicts that a fresh trainer loads strict; the bf16-mode
losses are printed beside the fp32-mode ones (recorded, not asserted)."""
from collections import OrderedDict

import pytest
import torch

import iql_ref as R
import mlp_bf16_ref as M

pytestmark = pytest.mark.gpu
Z, A, H, P, B, RN = 40, 3, 64, 50, 37, 4
K_TOL, FLOOR = 4.0, 1e-6
MLP = "s2p_mlp_linear_"


def _trainer(kind, dev, sd=None, **kw):
    from s2p_amd.cql import CQLTrainer
    from s2p_amd.iql import CriticSLAC, IQLTrainer, Qfunction, TanhGaussianPolicy, Vfunction
    q = [Qfunction(hidden_sizes=[H, H], output_size=1, input_size=Z + A) for _ in range(4)]
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=[H, H], output_size=1, input_size=Z), device=dev)
    policy = TanhGaussianPolicy(hidden_sizes=[H, H], obs_dim=P, action_dim=A, device=dev)
    if sd is not None:
        critic.load_state_dict(sd[0], strict=True)
        policy.load_state_dict(sd[1], strict=True)
    if kind == "iql":
        return IQLTrainer(None, policy, critic=critic, policy_lr=1e-4, qf_lr=3e-4, beta=0.1, quantile=0.7, clip_score=100, **kw)
    return CQLTrainer(None, policy, critic=critic, policy_lr=1e-4, qf_lr=3e-4, min_q_weight=5.0, num_random=RN, **kw)


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    b = dict(z=torch.randn(B, Z, generator=g), next_z=torch.randn(B, Z, generator=g), action=torch.rand(B, A, generator=g) * 1.8 - 0.9,
             policy_input=torch.randn(B, P, generator=g), policy_next_input=torch.randn(B, P, generator=g),
             rewards=torch.randn(B, generator=g), terminals=(torch.rand(B, generator=g) < 0.1).float())
    noise = dict(eps0=torch.randn(B, A, generator=g), eps1=torch.randn(B, A, generator=g), uniform=torch.rand(B * RN, A, generator=g) * 2 - 1,
                 eps2=torch.randn(B * RN, A, generator=g), eps3=torch.randn(B * RN, A, generator=g))
    return b, noise


def _step(kind, tr, seed):
    b, noise = _batch(seed)
    if kind == "iql":
        return tr.train_from_latents(b["z"], b["next_z"], b["action"], b["policy_input"], b["rewards"], b["terminals"]).clone()
    return tr.train_from_latents(b["z"], b["next_z"], b["action"], b["policy_input"], b["policy_next_input"], b["rewards"], b["terminals"],
                                 noise=noise).clone()


def _state(tr):
    return tr.critic.state_dict(), tr.policy.state_dict()


def _mlp_launches(tr):
    return {k: v for k, v in tr.launches.items() if k.startswith(MLP)}


@pytest.mark.parametrize("kind", ["iql", "cql"])
def test_default_is_unchanged(hip_device, kind):
    a = _trainer(kind, hip_device)
    b = _trainer(kind, hip_device, _state(a), mlp_compute="fp32")
    assert a.mlp_compute == "fp32"
    for s in range(2):
        la, lb = _step(kind, a, 10 + s), _step(kind, b, 10 + s)
        assert torch.equal(la, lb), (s, la, lb)
        assert torch.equal(a.critic.grad, b.critic.grad) and torch.equal(a.policy.grad, b.policy.grad)
        assert float(a.critic.grad.abs().max()) > 0 and float(a.policy.grad.abs().max()) > 0
    assert torch.equal(a.critic.flat, b.critic.flat) and torch.equal(a.critic.target_flat, b.critic.target_flat)
    assert torch.equal(a.policy.flat, b.policy.flat)
    for tr in (a, b):
        assert _mlp_launches(tr) and not any(k.endswith("_bf16") for k in tr.launches), dict(tr.launches)


def _routed(counts, bf16):
    """{(kind, wide): count} -> the launches by entry-point name in a compute mode."""
    out = {}
    for (kind, wide), n in counts.items():
        name = MLP + kind + ("_bf16" if bf16 and wide else "")
        out[name] = out.get(name, 0) + n
    return out


# per step: IQL runs the six networks as one launch per layer and width (two wide layers; the last layer in widths 1 and 2 A), forward and
# backward.  CQL runs four forward passes of three layers (policy, qf under the policy's action, the policy again, the critics), the
# policy's backward, the critics' backward with the wide layers split by rows, and in the SAC branch the dgrad through the critics
IQL_COUNTS = {("fwd", True): 2, ("fwd", False): 2, ("bwd", True): 2, ("bwd", False): 2}
CQL_COUNTS = {("fwd", True): 8, ("fwd", False): 4, ("bwd", True): 2, ("bwd", False): 2, ("bwd_split", True): 2}
CQL_SAC_COUNTS = {**CQL_COUNTS, ("dgrad", True): 2, ("dgrad", False): 1}


@pytest.mark.parametrize("kind,kw,counts", [("iql", {}, IQL_COUNTS), ("cql", dict(policy_eval_start=100), CQL_COUNTS),
                                            ("cql", dict(policy_eval_start=0), CQL_SAC_COUNTS)])
def test_routing(hip_device, kind, kw, counts):
    for mode in ("bf16", "fp32"):
        tr = _trainer(kind, hip_device, mlp_compute=mode, **kw)
        assert bool(torch.isfinite(_step(kind, tr, 20)).all())
        assert _mlp_launches(tr) == _routed(counts, mode == "bf16"), (mode, dict(tr.launches))


# ---- one network through mlp.Net tables in bf16 mode against the helper's MLP -------------------------------------------------------------
def _check(what, got, f64, f32):
    err, ref = R.rel_max(got.detach().cpu(), f64), max(R.rel_max(f32, f64), FLOOR)
    print("%-28s err %.3e  ref32_err %.3e  ratio %.3f" % (what, err, ref, err / ref))
    assert err <= K_TOL * ref, (what, err, K_TOL * ref)


@pytest.mark.parametrize("name,widths", [("q network", (Z + A, H, H, 1)), ("policy trunk", (P, H, H))])
def test_network_parity(hip_device, name, widths):
    from s2p_amd.mlp import Net, Packed, bwd_plan, bwd_tables, fwd_plan, fwd_tables, run
    from s2p_amd.ops import pad_to
    g, dev, f = torch.Generator().manual_seed(len(widths)), hip_device, torch.float32
    dims = list(zip(widths[:-1], widths[1:]))
    layers = [(torch.randn(n, k, generator=g) / k ** 0.5, torch.randn(n, generator=g) * 0.1) for k, n in dims]
    x, dout = torch.randn(B, widths[0], generator=g), torch.randn(B, widths[-1], generator=g)
    pk = Packed(dims)
    flat, grad = torch.zeros(pk.end, dtype=f, device=dev), torch.full((pk.end,), 7.0, dtype=f, device=dev)
    for li, (w, b) in enumerate(layers):
        pk.put(flat, li, w, b)
    xd = torch.zeros(B, pad_to(widths[0], 4), dtype=f, device=dev)
    xd[:, :widths[0]] = x
    out, dx = torch.empty(B, widths[-1], dtype=f, device=dev), torch.empty_like(xd)
    net = Net(name, pk, B, B).bind(flat, grad, xd, out, dout.to(dev).contiguous(), dx)
    called = []

    def call(entry, *args):
        from s2p_amd._lib import check, lib
        called.append(entry)
        check(getattr(lib(), entry)(*args), entry)

    run(fwd_tables(fwd_plan([net])), "s2p_mlp_linear_fwd", call, "bf16")
    run(bwd_tables(bwd_plan([net])), "s2p_mlp_linear_bwd", call, "bf16")
    torch.cuda.synchronize()
    assert called == [MLP + "fwd" + ("_bf16" if n > 16 else "") for _, n in dims] + [MLP + "bwd" + ("_bf16" if n > 16 else "") for _, n in dims[::-1]]
    ref = {}
    for dtype in (torch.float64, torch.float32):
        y, leaves, xin = M.mlp(layers, x, dtype)
        y.backward(dout.to(dtype))
        ref[dtype] = dict(out=y.detach().double(), dx=xin.grad.double(), **{"dw%d" % i: w.grad.double() for i, (w, _) in enumerate(leaves)},
                          **{"db%d" % i: b.grad.double() for i, (_, b) in enumerate(leaves)})
    got = dict(out=out, dx=dx[:, :widths[0]])
    for li, (k, n) in enumerate(dims):
        got["dw%d" % li], got["db%d" % li] = pk.w(grad, li)[:, :k], pk.b(grad, li)
    for k in got:
        _check("%s %s" % (name, k), got[k], ref[torch.float64][k], ref[torch.float32][k])


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["iql", "cql"])
def test_three_steps_in_bf16_mode(hip_device, kind):
    kw = dict(policy_eval_start=2) if kind == "cql" else {}                           # one cloning step, then the SAC branch
    tr = _trainer(kind, hip_device, mlp_compute="bf16", **kw)
    ref = _trainer(kind, hip_device, _state(tr), mlp_compute="fp32", **kw)
    init = OrderedDict((k, v.clone()) for sd in _state(tr) for k, v in sd.items())
    for s in range(3):
        lb, lf = _step(kind, tr, 30 + s).cpu(), _step(kind, ref, 30 + s).cpu()
        print("%s step %d losses  bf16 mode %s   fp32 mode %s" % (kind, s, [round(float(v), 6) for v in lb], [round(float(v), 6) for v in lf]))
        assert bool(torch.isfinite(lb).all()), lb
    assert any(k.endswith("_bf16") for k in tr.launches)
    critic_sd, policy_sd = _state(tr)
    for k, v in list(critic_sd.items()) + list(policy_sd.items()):
        assert v.dtype == torch.float32 and bool(torch.isfinite(v).all()), k
    assert any(not torch.equal(v, init[k]) for k, v in critic_sd.items())             # the networks were trained
    fresh = _trainer(kind, hip_device, mlp_compute="bf16", **kw)
    fresh.critic.load_state_dict(critic_sd, strict=True)
    fresh.policy.load_state_dict(policy_sd, strict=True)
    fresh.load_state_dict(tr.state_dict())
    assert torch.equal(fresh.critic.flat, tr.critic.flat) and torch.equal(fresh.policy.flat, tr.policy.flat)
    assert torch.equal(_step(kind, fresh, 40), _step(kind, tr, 40))                   # and the restored trainer continues bit for bit
