"""Generates tests/golden/actor_golden_v1.npz by RUNNING THE REAL REFERENCE `rollout()` (`rlkit/samplers/rollout_functions.py`, its SLAC
branch) on the CPU, in fp64 and in fp32, with the real `SlacObservation`, the real `LatentModel` / `Encoder`, the real
`SlacAlgorithm.preprocess` / `prepare_batch` and `MakeDeterministic(TanhGaussianPolicyWithEncoder)`, on the scripted environment, the
seeded weights and the recorded posterior noise of tests/actor_ref.py.  `torchvision`, `torchvision.models` and `gtimer` are empty
stand-in modules, as in the other fixture generators (and `torch.utils.tensorboard`, `pandas`, `tqdm` where they are not installed).
The reference's `SlacAlgorithm` is constructed as it is (CPU, a 16-window buffer); PYTORCH_JIT=0 makes its traced / scripted functions plain Python so `torch.randn_like` can be replaced, for the duration of
a `prepare_batch`, by a function that hands out the recorded eps (draw order z1(0), z2(0), z1(1), ...).

The reference's acting path is fp32 by construction (`.float()`, `dtype=torch.float`, `ptu.from_numpy`): for the fp64 run those three
are redirected to fp64 for the duration of the rollout, nothing else of it is touched.

Data only: seeds and a weight checksum; per configuration (policy input type x reset_w_same_obs) and episode, per step the policy
input (whole where it is short, else norm, sum and a strided sample) and the action, per episode return, length and terminal flag;
per configuration `ref32_err`, the largest deviation of the reference's own fp32 run from its fp64 run over all steps, for the
policy input and for the action, in the measures the tests use.
Run:  python tests/golden/make_golden_actor.py REFERENCE_DIR"""
import os
import sys
import types

os.environ["PYTORCH_JIT"] = "0"
import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("S2P_REFERENCE_DIR", "")
for name in ("torchvision", "torchvision.models", "gtimer"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["torchvision"].models = sys.modules["torchvision.models"]
sys.modules["torchvision.models"].resnet18 = None
for name, attr in (("torch.utils.tensorboard", "SummaryWriter"), ("pandas", "DataFrame"), ("tqdm", "tqdm")):
    try:                                                     # (rlkit/torch/slac/trainer.py imports them beside SlacObservation)
        __import__(name)
    except ImportError:
        sys.modules[name] = types.ModuleType(name)
        setattr(sys.modules[name], attr, None)
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REF, "examples", "iql"))
import actor_ref as AR  # noqa: E402
import slac_latent_ref as R  # noqa: E402
import rlkit.torch.pytorch_util as ptu  # noqa: E402
from rlkit.samplers.rollout_functions import rollout  # noqa: E402  (the real reference)
from rlkit.torch.sac.policies import MakeDeterministic  # noqa: E402
from rlkit.torch.slac.algo import SlacAlgorithm  # noqa: E402
from custom_networks import TanhGaussianPolicyWithEncoder  # noqa: E402


class AsDouble:
    """Redirect the fp32 conversions of the reference's acting path to fp64 (see the module docstring)."""

    def __enter__(self):
        self.saved = (torch.Tensor.float, torch.tensor, ptu.from_numpy)
        orig_tensor = torch.tensor
        torch.Tensor.float = lambda t, *a, **k: t.double()
        torch.tensor = lambda *a, **k: orig_tensor(*a, **{**k, "dtype": torch.float64 if k.get("dtype") is torch.float else k.get("dtype")})
        ptu.from_numpy = lambda *a, **k: torch.from_numpy(*a, **k).double()
        return self

    def __exit__(self, *exc):
        torch.Tensor.float, torch.tensor, ptu.from_numpy = self.saved


class Recorder(torch.nn.Module):
    """Sits in the policy's `encoder` slot (identity): the one place the reference's policy input passes as a tensor."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def forward(self, x, detach=False):
        self.seen.append(x.detach().clone()[0])
        return x


def run(input_type, same_obs, dtype, latent_p):
    algo = SlacAlgorithm(AR.STATE_SHAPE, (AR.A,), action_repeat=1, device=torch.device("cpu"), seed=0, buffer_size=16, num_sequences=AR.S,
                         image_size=100)
    algo.latent.load_state_dict(R.full_state_dict(latent_p), strict=True)
    algo.latent.to(dtype)
    obs_dim = AR.obs_dim_of(input_type)
    rec = Recorder()
    policy = TanhGaussianPolicyWithEncoder(obs_dim=obs_dim, action_dim=AR.A, hidden_sizes=[AR.H, AR.H], encoder=rec)
    policy.load_state_dict(AR.make_policy_params(obs_dim), strict=True)
    policy.to(dtype)
    agent = MakeDeterministic(policy)
    env = AR.ScriptedEnv()
    out = []
    orig_randn_like, orig_prepare = torch.randn_like, algo.prepare_batch
    for ep in range(AR.EPISODES):
        step = [0]

        def prepare_batch(state_, action_):
            noise = AR.make_noise(ep, step[0]).to(dtype)
            step[0] += 1
            draws = []
            for t in range(AR.S):
                draws += [noise[:, t, :R.Z1], noise[:, t, R.Z1:]]
            it = iter(draws)

            def recorded(x, **kw):
                e = next(it)
                assert e.shape == x.shape
                return e
            torch.randn_like = recorded
            try:
                res = orig_prepare(state_, action_)
                assert next(it, None) is None
            finally:
                torch.randn_like = orig_randn_like
            return res

        algo.prepare_batch = prepare_batch
        rec.seen = []
        ctx = AsDouble() if dtype == torch.float64 else None
        if ctx:
            ctx.__enter__()
        try:
            path = rollout(env, agent, max_path_length=AR.MAX_PATH, slac_algo=algo, slac_policy_input_type=input_type,
                           slac_obs_reset_w_same_obs=same_obs)
        finally:
            if ctx:
                ctx.__exit__()
        T = len(path["actions"])
        assert len(rec.seen) == T and rec.seen[0].dtype == dtype and path["actions"].dtype == (np.float64 if dtype == torch.float64 else np.float32)
        out.append(dict(inputs=rec.seen, actions=path["actions"], ret=float(path["rewards"].sum()), length=T,
                        terminal=bool(path["terminals"][-1, 0])))
    return out


def main():
    torch.set_num_threads(8)
    ptu.device = torch.device("cpu")
    latent_p = R.make_params(AR.A)
    policy_ps = [AR.make_policy_params(AR.obs_dim_of(t)) for t in AR.INPUT_TYPES]
    out = dict(seeds=np.array([AR.SEEDS[k] for k in ("frames", "policy", "noise")] + [R.SEEDS[k] for k in ("enc", "dec", "heads")]),
               sizes=np.array([AR.A, AR.H, AR.S, AR.DONE_STEP, AR.MAX_PATH, AR.EPISODES]),
               checksum=np.float64(AR.checksum(latent_p, policy_ps)))
    for input_type in AR.INPUT_TYPES:
        for same in (False, True):
            name = AR.config_name(input_type, same)
            r64, r32 = run(input_type, same, torch.float64, latent_p), run(input_type, same, torch.float32, latent_p)
            e_in, e_act, spread = 0.0, 0.0, []
            for ep, (a, b) in enumerate(zip(r64, r32)):
                assert (a["length"], a["terminal"], a["ret"]) == (b["length"], b["terminal"], b["ret"])
                out["%s.ep%d.return" % (name, ep)] = np.float64(a["ret"])
                out["%s.ep%d.length" % (name, ep)] = np.int64(a["length"])
                out["%s.ep%d.terminal" % (name, ep)] = np.bool_(a["terminal"])
                out["%s.ep%d.actions" % (name, ep)] = np.asarray(a["actions"], dtype=np.float64)
                for t in range(a["length"]):
                    rec = AR.input_record(a["inputs"][t])
                    for k, v in rec.items():
                        out["%s.ep%d.input%d.%s" % (name, ep, t, k)] = v
                    e_in = max(e_in, AR.input_err(b["inputs"][t], rec))
                    e_act = max(e_act, R.rel_max(b["actions"][t], a["actions"][t]))
                spread.append(np.abs(a["actions"]))
            spread = np.concatenate(spread).reshape(-1)
            assert ((spread > 0.1) & (spread < 0.9)).mean() > 0.3, "the actions are spread over (-1, 1)"
            out[name + ".input.ref32_err"], out[name + ".action.ref32_err"] = np.float64(e_in), np.float64(e_act)
            print("%-22s lengths %s terminals %s returns %s  ref32_err input %.2e action %.2e  |a| in [%.3f, %.3f]" % (
                name, [e["length"] for e in r64], [e["terminal"] for e in r64], [e["ret"] for e in r64], e_in, e_act,
                spread.min(), spread.max()))
            assert [e["length"] for e in r64] == [AR.DONE_STEP, AR.MAX_PATH] and [e["terminal"] for e in r64] == [True, False]
    path = os.path.join(HERE, "actor_golden_v1.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
