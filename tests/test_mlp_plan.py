"""The launch description of s2p_amd/mlp.py (no device): which layer of which network is a group of which grouped launch, with the
launch's N, activation and the groups' row counts, for the IQL step, the CQL step and a mixed-depth table, from shapes alone.  The
device half (the ctypes tables made from a plan) is what tests/test_iql_gpu.py and tests/test_cql_gpu.py run."""
import pytest

from s2p_amd._lib import ACT_NONE, ACT_RELU

HID, Z, A, P, B = [20, 24], 10, 3, 13, 5


def _nets(hidden=HID):
    from s2p_amd.offline_rl import CriticSLAC, Qfunction, TanhGaussianPolicy, Vfunction
    q = [Qfunction(hidden_sizes=hidden, output_size=1, input_size=Z + A) for _ in range(4)]
    critic = CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=hidden, output_size=1, input_size=Z), device=None)
    return critic, TanhGaussianPolicy(hidden_sizes=hidden, obs_dim=P, action_dim=A, device=None)


def _shape(plan):
    return [(len(l.nets), l.N, l.act) for l in plan]


def _names(plan):
    return [[n.name for n in l.nets] for l in plan]


def test_iql_plan():
    from s2p_amd.iql import step_plan
    nets, fwd, bwd = step_plan(*_nets(), B)
    every = ["qf1", "qf2", "target_qf1", "target_qf2", "vf", "policy"]
    assert list(nets) == every
    assert _shape(fwd) == [(6, 20, ACT_RELU), (6, 24, ACT_RELU), (5, 1, ACT_NONE), (1, 6, ACT_NONE)]
    assert _names(fwd) == [every, every, every[:5], ["policy"]]
    assert [l.li for l in fwd] == [0, 1, 2, 2]
    assert [[n.rows for n in l.nets] for l in fwd[:2]] == [[B, B, B, B, 2 * B, B]] * 2 and nets["vf"].rows == 10
    trained = ["qf1", "qf2", "vf", "policy"]
    assert _shape(bwd) == [(3, 1, ACT_RELU), (1, 6, ACT_RELU), (4, 24, ACT_RELU), (4, 20, ACT_NONE)]
    assert _names(bwd) == [trained[:3], ["policy"], trained, trained]
    assert [l.li for l in bwd] == [2, 2, 1, 0]
    assert all(n.bwd_rows == B for l in bwd for n in l.nets)
    assert nets["target_qf1"].bwd_rows is None and nets["target_qf2"].bwd_rows is None
    # the input widths a group's K comes from: padded to a multiple of 4 floats
    assert [nets[n].pk.off[0][2] for n in every] == [16, 16, 16, 16, 12, 16]


def test_cql_plan():
    from s2p_amd.cql import step_plan
    R = 2
    M = B * (1 + 3 * R)
    nets, plans = step_plan(*_nets(), B, R)
    fwd3 = lambda G, last: [(G, 20, ACT_RELU), (G, 24, ACT_RELU), (G, last, ACT_NONE)]          # noqa: E731
    bwd3 = lambda G, last: [(G, last, ACT_RELU), (G, 24, ACT_RELU), (G, 20, ACT_NONE)]          # noqa: E731
    assert list(plans) == ["policy_fwd", "policy_bwd", "policy2_fwd", "qpol_fwd", "qpol_dgrad", "critic_fwd", "critic_bwd"]
    assert _shape(plans["policy_fwd"]) == fwd3(1, 6) and _shape(plans["policy_bwd"]) == bwd3(1, 6)
    assert _shape(plans["policy2_fwd"]) == fwd3(1, 6)
    assert _shape(plans["qpol_fwd"]) == fwd3(2, 1) and _shape(plans["qpol_dgrad"]) == bwd3(2, 1)
    assert _shape(plans["critic_fwd"]) == fwd3(4, 1) and _shape(plans["critic_bwd"]) == bwd3(2, 1)
    rows = {k: [[n.rows for n in l.nets] for l in p] for k, p in plans.items() if k.endswith("fwd")}
    assert rows == dict(policy_fwd=[[B]] * 3, policy2_fwd=[[2 * B]] * 3, qpol_fwd=[[B, B]] * 3, critic_fwd=[[M, M, B, B]] * 3)
    brows = {k: [[n.bwd_rows for n in l.nets] for l in p] for k, p in plans.items() if not k.endswith("fwd")}
    assert brows == dict(policy_bwd=[[B]] * 3, qpol_dgrad=[[B, B]] * 3, critic_bwd=[[M, M]] * 3)
    assert _names(plans["critic_fwd"]) == [["qf1", "qf2", "target_qf1", "target_qf2"]] * 3
    assert _names(plans["critic_bwd"]) == _names(plans["qpol_dgrad"]) == [["qf1", "qf2"]] * 3
    assert [l.li for l in plans["critic_fwd"]] == [0, 1, 2] and [l.li for l in plans["critic_bwd"]] == [2, 1, 0]
    assert all(n.bwd_rows is None for n in nets["pol2"] + nets["qtgt"])


def test_unequal_depth_and_mixed_widths_are_refused():
    from s2p_amd.mlp import Net, bwd_plan, fwd_plan
    critic, policy = _nets()
    _, deep = _nets([20, 24, 28])
    a, b = Net("policy", policy.packed, B, B), Net("deep", deep.packed, B, B)
    for plan in (fwd_plan, bwd_plan):
        with pytest.raises(ValueError, match="unequal depth"):
            plan([a, b])
    q = Net("qf1", critic.packed["qf1"], B, B)
    assert _shape(fwd_plan([q, a]))[2:] == [(1, 1, ACT_NONE), (1, 6, ACT_NONE)]             # partitioned by width ...
    for plan in (fwd_plan, bwd_plan):
        with pytest.raises(ValueError, match="output widths"):                             # ... unless the caller wants one launch a layer
            plan([q, a], True)
