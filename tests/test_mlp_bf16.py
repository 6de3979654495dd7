"""N3l -- the bf16 compute mode of the grouped MLP layers, what needs no GPU: the four entry points are declared, exported and bound;
the entry-selection function; the command-line flag; the `mlp_compute` keyword; and the kernel tests' per-element bound
(tests/mlp_bf16_ref.py) admits a correct implementation: fp32 torch matmuls of the rounded operands lie inside it at every shape of
tests/test_mlp_bf16_kernels_gpu.py."""
import ctypes
import os
import re
import sys

import pytest
import torch

import mlp_bf16_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("s2p_mlp_linear_fwd_bf16", "s2p_mlp_linear_bwd_bf16", "s2p_mlp_linear_dgrad_bf16", "s2p_mlp_linear_bwd_split_bf16")


def test_the_four_entry_points_are_declared_exported_and_bound():
    from s2p_amd import _lib
    header = open(os.path.join(ROOT, "include", "s2p_hip.h")).read()
    so = ctypes.CDLL(_lib._SO)
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert hasattr(so, name), name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name[:-5]], name          # the signature of the fp32 counterpart
    assert _lib.lib().s2p_version() == 125


def test_entry_selection():
    from s2p_amd.mlp import entry_point
    for kind in ("fwd", "bwd", "dgrad", "bwd_split"):
        fp32 = "s2p_mlp_linear_" + kind
        assert entry_point(kind, 16, "bf16") == fp32                               # the narrow layers keep the fp32 kernels
        assert entry_point(kind, 20, "bf16") == fp32 + "_bf16"
        assert entry_point(kind, 1, "bf16") == fp32 and entry_point(kind, 1024, "bf16") == fp32 + "_bf16"
        for N in (1, 16, 20, 1024):
            assert entry_point(kind, N, "fp32") == fp32 and entry_point(kind, N) == fp32
        with pytest.raises(ValueError):
            entry_point(kind, 20, "fp16")
    with pytest.raises(KeyError):
        entry_point("wgrad", 20, "bf16")


def test_the_flag_parses_in_both_scripts_and_defaults_to_off():
    sys.path.insert(0, ROOT)
    import train_cql
    import train_iql
    base = ["--real", "r.npz", "--latent_dir", "d", "--steps", "5", "--out", "o"]
    for T in (train_iql, train_cql):
        a = T.parse_args(base)
        assert a.bf16_mlp is False and a.bf16 is False
        a = T.parse_args(base + ["--bf16_mlp"])
        assert a.bf16_mlp is True and a.bf16 is False                              # independent of --bf16
        a = T.parse_args(base + ["--bf16"])
        assert a.bf16_mlp is False and a.bf16 is True


def test_a_bad_mlp_compute_raises():
    from s2p_amd.cql import CQLTrainer
    from s2p_amd.iql import CriticSLAC, IQLTrainer, Qfunction, TanhGaussianPolicy, Vfunction
    from s2p_amd.offline_rl import LatentTrainer

    def nets():
        q = [Qfunction(hidden_sizes=[32, 32], output_size=1, input_size=12) for _ in range(4)]
        return (CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=[32, 32], output_size=1, input_size=8), device=None),
                TanhGaussianPolicy(hidden_sizes=[32, 32], obs_dim=8, action_dim=4, device=None))

    for bad in ("fp16", "BF16", None, True):
        critic, policy = nets()
        with pytest.raises(ValueError, match="mlp_compute"):
            IQLTrainer(None, policy, critic=critic, mlp_compute=bad)
        with pytest.raises(ValueError, match="mlp_compute"):
            CQLTrainer(None, policy, critic=critic, mlp_compute=bad)
        with pytest.raises(ValueError, match="mlp_compute"):
            LatentTrainer(None, policy, critic, None, None, None, None, None, 1e-3, 1e-3, None, False, 1, "latent_z", mlp_compute=bad)


def test_fp32_matmul_of_rounded_operands_lies_inside_the_bound():
    """Every shape of the GPU test, standard normal data: the worst |got - ref| / bound over all outputs, printed."""
    g, worst = torch.Generator().manual_seed(0), {}
    for rows, N, K in M.SHAPES:
        x, w, b = torch.randn(rows, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
        d, pp = torch.randn(rows, N, generator=g), torch.randn(rows, K, generator=g)
        (p64, pmag), (p32, _) = M.fwd(x, w, b), M.fwd(x, w, b, torch.float32)
        (w64, wmag, _), (w32, _, _) = M.wgrad(d, x), M.wgrad(d, x, torch.float32)
        (d64, dmag), (d32, _) = M.dgrad(d, w, pp), M.dgrad(d, w, pp, torch.float32)
        for what, r in (("pre", M.worst_ratio(p32, p64, K, pmag)), ("dw", M.worst_ratio(w32, w64, rows, wmag)),
                        ("dprev", M.worst_ratio(d32, d64, N, dmag))):
            worst[what] = max(worst.get(what, 0.0), r)
            assert r <= 1.0, (what, rows, N, K, r)
    print("worst |fp32 - fp64| / bound:", {k: "%.3f" % v for k, v in worst.items()})
    assert M.worst_ratio(torch.tensor([float("nan")]), torch.zeros(1, dtype=torch.float64), 4, torch.ones(1, dtype=torch.float64)) == float("inf")
