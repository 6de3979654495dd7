"""The rounding rule of the policy half of the bf16-compute imagination chain (SPEC.md N3n) restated in torch on the CPU -- TEST
INFRASTRUCTURE ONLY.  Builds on tests/chain_bf16_ref.py (the rule of the latent half, `_dot`) and tests/slac_imagine_ref.py (the
policy's weights and the fp32 / fp64 restatement of the rollout).

Per policy layer: both operands rounded to bf16 (nearest even) -- z(h), the two hidden activations, the weights -- the products summed
in `dtype` (fp64: the reference; fp32: what a kernel can do), relu(acc + bias) resp. tanh(acc + bias); a(h) is not rounded.  `gen`
permutes each layer's summation index ("another summation order").  The rule is evaluated TEACHER-FORCED: on given z(h), so that one
evaluation's rounding flips do not travel down the chain."""
import torch

import chain_bf16_ref as C
import chain_refusals as CR
import slac_imagine_ref as IM

Z = C.Z
TIGHT, CAP, K_TOL = 4e-6, 0.05, 4.0


def policy_rule(pol, z, dtype, gen=None):
    """a = tanh(last_fc(relu(fc1(relu(fc0(z)))))) under the rule, z [..., 288] (fp32 values) -> [..., A] in `dtype`."""
    h = z
    for name in ("fc0", "fc1"):
        h = torch.relu(C._dot(h, pol[name + ".weight"], dtype, gen) + pol[name + ".bias"].to(dtype))
    return torch.tanh(C._dot(h, pol["last_fc.weight"], dtype, gen) + pol["last_fc.bias"].to(dtype))


def rollout_inputs(z0, z):
    """z(h), h = 0 .. H-1, of a rollout that returned z [B,H,288] (slot h = z(h+1)) from z0 -> [B,H,288]: what the policy read."""
    return torch.cat([z0[:, None], z[:, :-1]], dim=1)


def action_deviation(got, ref):
    """Per (row, step): max_A |got - ref| relative to the step's maximum |ref| -> a flat fp64 tensor of B H values."""
    g, r = got.double().cpu(), ref.double().cpu()
    return ((g - r).abs().amax(-1) / r.abs().amax((0, 2), keepdim=True).squeeze(-1)).flatten()


def random_case(W, seed, B=33, H=3, A=6):
    """Policy weights, z0 [B,288] and noise [B,H,288] of one teacher-forced case: `IM.make_policy_params(W, A)` and seeded normal draws."""
    g = torch.Generator().manual_seed(2024 + 1000 * seed + 100 * H + A)
    return IM.make_policy_params(W, A), torch.randn(B, Z, generator=g), torch.randn(B, H, Z, generator=g)


def exact_policy(W, A, seed=0):
    """Policy weights on which every sum of the three layers is exact in fp32 in any order and every hidden activation is exactly a
    bf16 number, given `exact_z0`: weights in {0, +-1/4} with two non-zeros per row, biases multiples of 1/4 in [-1, 1].  Then
    z0 in 1/4 steps, |z0| < 2  ->  h1 in 1/16 steps in [0, 2]  ->  h2 in 1/64 steps in [0, 2] (at most 8 significant bits)  ->  the
    last layer's acc in 1/256 steps."""
    g = torch.Generator().manual_seed(515 + 13 * W + A + 1000 * seed)
    p = IM.make_policy_params(W, A)
    for name, (co, ci) in (("fc0", (W, Z)), ("fc1", (W, W)), ("last_fc", (A, W))):
        w = torch.zeros(co, ci)
        for n in range(co):
            w[n, torch.randperm(ci, generator=g)[:2]] = (torch.randint(0, 2, (2,), generator=g).float() * 2 - 1) / 4
        p[name + ".weight"] = w
        p[name + ".bias"] = torch.randint(-4, 5, (co,), generator=g).float() / 4
    return p


def exact_z0(B):
    """z0 [B,288]: multiples of 1/4 in (-2, 2); row b is the same whatever B is."""
    g = torch.Generator().manual_seed(616)
    return (torch.randint(-7, 8, (33, Z), generator=g).float() / 4)[:B]


def assert_exact_premises(pol, z0):
    """The premises of the exact-data test: every operand and both hidden activations are bf16 numbers, and every layer's fp32 sum is
    exact (equal to the fp64 sum, in the natural and in a permuted order).  -> a(0) of the rule in fp64."""
    x = z0
    for name, last in (("fc0", False), ("fc1", False), ("last_fc", True)):
        w, b = pol[name + ".weight"], pol[name + ".bias"]
        assert torch.equal(C.bf(x), x) and torch.equal(C.bf(w), w), name + ": an operand is not a bf16 number"
        ref = C._dot(x, w, torch.float64, None)
        for gen in (None, torch.Generator().manual_seed(3)):
            assert torch.equal(C._dot(x, w, torch.float32, gen).double(), ref), name + ": an fp32 sum is not exact"
        pre = ref + b.double()
        assert torch.equal(pre.float().double(), pre), name + ": acc + bias is not exact in fp32"
        if last:
            return torch.tanh(pre)
        x = torch.relu(pre).float()
        assert float(x.max()) > 0


# ---- the C ABI of s2p_imagine_chain_fwd_bf16: its rows of the table of every chain entry point (tests/chain_refusals.py) ----------------
NAME = "s2p_imagine_chain_fwd_bf16"
P = CR.P
REFUSALS = tuple(CR.cases(NAME))                       # (the edit, a piece of the message)


def abi_args(_lib, **edit):
    """The 22 arguments of a valid call (B 17, H 2, A 6, W 256) on fake addresses, with `edit` applied (chain_refusals.args)."""
    return CR.args(_lib, NAME, **edit)


def check_refusals(_lib):
    """Every case of REFUSALS returns a negative value with its message, and the no-ops return 0 looking at no pointer."""
    return CR.check(_lib, NAME)
