"""N3n on the host: the helper tests/imagine_bf16_ref.py holds what tests/test_imagine_bf16_gpu.py relies on (the exact data of its
policy test really is exact and really is bf16; the rule's own fp32 runs stay under the cap the GPU test gives a kernel), the entry
point s2p_imagine_chain_fwd_bf16 is exported, declared and refuses bad arguments before any launch, `paired` is the paired statistic,
and select_policy.py's parser follows the chain options' rule."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import imagine_bf16_ref as IB
import select_policy
import slac_imagine_ref as IM
import slac_latent_ref as R
from s2p_amd.slac_imagine import paired

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS, WS, AS = (1, 15, 16, 17, 33), (128, 384, 1024), (6, 1, 8)


# ---- the policy rule -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,A", [(128, 6), (384, 1), (1024, 8)])
def test_exact_data_holds_its_premises_and_is_the_plain_policy(W, A):
    pol, z0 = IB.exact_policy(W, A), IB.exact_z0(33)
    a64 = IB.assert_exact_premises(pol, z0)
    # on such data the rule rounds nothing: it is the plain policy, in fp64 and in fp32, in any summation order
    assert torch.equal(IB.policy_rule(pol, z0, torch.float64), a64)
    assert torch.equal(a64, IM.act({k: v.double() for k, v in pol.items()}, z0.double()))
    assert torch.equal(IB.policy_rule(pol, z0, torch.float32), IB.policy_rule(pol, z0, torch.float32, torch.Generator().manual_seed(1)))
    assert len(torch.unique(a64)) > 4 and float(a64.abs().max()) < 1                                           # the actions vary, unsaturated
    for B in BS:
        assert torch.equal(IB.exact_z0(B), z0[:B])


def test_rule_rounds_on_random_data():
    pol, z0, _ = IB.random_case(128, 0)
    plain = IM.act({k: v.double() for k, v in pol.items()}, z0.double())
    ruled = IB.policy_rule(pol, z0, torch.float64)
    dev = float((plain - ruled).abs().max())
    print("random data: the rule's fp64 actions are %.3e from the unrounded policy's" % dev)
    assert dev > 1e-5                                      # real rounding; bf16 keeps 8 bits, an operand moves by up to 2^-9 of itself
    assert bool((ruled.abs() <= 1).all())


@pytest.mark.parametrize("W", [128, 1024])
def test_helper_fp32_runs_stay_under_the_cap(W):
    """On the inputs of the GPU test (B 33, H 3, A 6, three seeds; 297 (row, step) pairs), teacher-forced on the z of a free fp32
    rollout: the rule's fp32 runs in two summation orders against its fp64 run.  A kernel is given CAP = 5 % of pairs outside 4e-6;
    the rule's own fp32 arithmetic must fit under that cap too, or the cap would be a statement about rounding flips, not kernels."""
    A, B, H = 6, 33, 3
    p = {k: v for k, v in R.make_params(A).items()}
    worst = 0.0
    for order in ("plain", "permuted"):
        devs = []
        for seed in (0, 1, 2):
            pol, z0, noise = IB.random_case(W, seed, B, H, A)
            z = IM.imagine(p, pol, z0, noise)[3]
            x = IB.rollout_inputs(z0, z)
            gen = torch.Generator().manual_seed(9 + seed) if order == "permuted" else None
            devs.append(IB.action_deviation(IB.policy_rule(pol, x, torch.float32, gen), IB.policy_rule(pol, x, torch.float64)))
        dev = torch.cat(devs)
        miss = int((dev > IB.TIGHT).sum())
        print("W %d %s order: %d of %d pairs not tight (%.2f %%), worst %.3e" % (W, order, miss, dev.numel(), 100.0 * miss / dev.numel(),
                                                                                float(dev.max())))
        assert dev.numel() == 297 and miss <= IB.CAP * dev.numel()
        worst = max(worst, float(dev.max()))
    assert worst > 0


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_declared_and_versioned():
    from s2p_amd import _lib
    header = open(os.path.join(ROOT, "include", "s2p_hip.h")).read()
    sig, twin = _lib.SIGNATURES[IB.NAME], _lib.SIGNATURES["s2p_imagine_chain_fwd"]
    assert len(sig) == len(twin) == 22
    assert [t for i, t in enumerate(sig) if i not in (4, 10)] == [t for i, t in enumerate(twin) if i not in (4, 10)]
    assert sig[4] == ctypes.POINTER(_lib.ChainMlpBf16) and sig[10] == ctypes.POINTER(_lib.PolicyMlpBf16)
    assert "int %s(" % IB.NAME in header and "} s2p_policy_mlp_bf16;" in header
    L = _lib.lib()
    assert hasattr(L, IB.NAME) and L.s2p_version() == 125
    assert ctypes.sizeof(_lib.PolicyMlpBf16) == 6 * 8 + 2 * 4


def test_refusals_and_no_ops_without_a_device():
    from s2p_amd import _lib
    assert IB.check_refusals(_lib) >= 30
    L = _lib.lib()
    assert getattr(L, IB.NAME)(*IB.abi_args(_lib, B=0, z0=None, policy_ptr=None)) == 0


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------------
def test_keywords_default_to_fp32():
    from s2p_amd import ops, slac_imagine
    from s2p_amd.offline_rl import TanhGaussianPolicy
    from s2p_amd.slac import LatentModel
    assert inspect.signature(LatentModel.imagine).parameters["compute"].default == "fp32"
    assert list(inspect.signature(LatentModel.imagine).parameters)[:6] == ["self", "policy", "z0", "horizon", "noise", "sample"]
    assert inspect.signature(slac_imagine.imagined_returns).parameters["compute"].default == "fp32"
    names = list(inspect.signature(slac_imagine.compare_policies).parameters)
    assert names == ["latent", "policies", "frames_u8_nhwc", "actions", "horizon", "discount", "critics", "context", "noise", "sample",
                     "posterior_noise", "compute"]
    assert callable(ops.policy_mlp_bf16) and callable(ops.imagine_chain_fwd_bf16) and callable(TanhGaussianPolicy.packed_bf16)


# ---- paired ----------------------------------------------------------------------------------------------------------------------------------
def test_paired_on_hand_made_returns():
    r = np.array([[1.0, 2.0, 3.0, 6.0],                    # mean 3
                  [2.0, 3.0, 4.0, 7.0],                    # mean 4: the best; every window 1 above policy 0
                  [1.0, 2.0, 3.0, 6.0],                    # policy 0 again
                  [8.0, 0.0, 4.0, 4.0]])                   # mean 4 as well: a tie with policy 1, which was given first
    s = paired(r)
    assert s["order"].tolist() == [1, 3, 0, 2] and s["best"] == 1
    assert np.array_equal(s["mean"], [3.0, 4.0, 3.0, 4.0])
    assert np.allclose(s["se"], r.std(axis=1, ddof=1) / 2.0, rtol=1e-15, atol=0)
    # the common part of the windows cancels: the difference of policy 0 to the best is -1 in EVERY window, its SE is 0 although each
    # policy's own SE is above 1
    assert np.array_equal(s["diff_mean"], [-1.0, 0.0, -1.0, 0.0]) and s["diff_se"][0] == 0.0 and s["diff_se"][1] == 0.0 and s["se"][0] > 1
    d3 = r[3] - r[1]
    assert s["diff_se"][3] == d3.std(ddof=1) / 2.0 and s["diff_se"][3] > 0
    # a duplicated policy: difference 0, SE 0
    two = paired(r[[0, 2]])
    assert two["order"].tolist() == [0, 1] and np.array_equal(two["diff_mean"], [0.0, 0.0]) and np.array_equal(two["diff_se"], [0.0, 0.0])
    one = paired(r[:1, :1])                                # one policy, one window: no spread to estimate
    assert one["se"].tolist() == [0.0] and one["diff_se"].tolist() == [0.0] and one["order"].tolist() == [0]
    assert paired(torch.tensor(r))["order"].tolist() == [1, 3, 0, 2]
    for bad in (np.zeros(3), np.zeros((0, 3)), np.zeros((2, 0))):
        with pytest.raises(ValueError):
            paired(bad)


# ---- select_policy.py --------------------------------------------------------------------------------------------------------------------------
NEED = ["--data", "d.npz", "--latent_dir", "l", "--out", "o.npz", "--policy_dirs"]


def test_select_policy_parser(capsys):
    a = select_policy.parse_args(NEED + ["p0", "p1", "p2"])
    assert a.policy_dirs == ["p0", "p1", "p2"] and (a.context, a.horizon, a.windows, a.batch, a.discount, a.seed) == (8, 16, 256, 256, 0.99, 0)
    assert a.stride is None and not (a.mean or a.bf16 or a.bootstrap or a.fused_chain or a.bf16_chain)
    assert not hasattr(a, "fused_chain_grad")
    from s2p_amd.latent_cli import chain_settings
    assert chain_settings(a) == dict(fused_chain=False, fused_chain_grad=False, chain_compute="fp32")
    b = select_policy.parse_args(NEED + ["p0", "--fused_chain", "--bf16_chain", "--mean", "--bootstrap", "--stride", "3"])
    assert b.policy_dirs == ["p0"] and b.fused_chain and b.bf16_chain and b.mean and b.bootstrap and b.stride == 3
    assert chain_settings(b) == dict(fused_chain=True, fused_chain_grad=False, chain_compute="bf16")
    for argv, text in ((NEED + ["p0", "--bf16_chain"], "--bf16_chain needs --fused_chain"), (NEED, "expected at least one argument"),
                       (NEED[:-1], "--policy_dirs"), (NEED + ["p0", "--context", "0"], "--context"),
                       (NEED + ["p0", "--batch", "0"], "at least 1")):
        with pytest.raises(SystemExit):
            select_policy.parse_args(argv)
        assert text in capsys.readouterr().err, argv
    assert select_policy.build_parser() is not select_policy.build_parser()
