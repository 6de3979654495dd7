"""What the command lines of the latent pipeline share (train_latent.py, train_iql.py, train_cql.py, evaluate_policy.py,
predict_latent.py, imagine_policy.py, select_policy.py): the dataset and chain options, the rule between them, and the way from parsed options to a loaded
`LatentModel`, a filled `SlacAlgorithm` and a finished offline-RL run.  A new switch of the chains is threaded here, once: its option
in `add_chain_options`, its rule in `check_chain_options`, its way into the model in `chain_settings`."""
import os

import torch

BF16_CHAIN_HELP = ("with --fused_chain: bf16 matrix-core compute inside the fused no-grad latent chain (SPEC.md N3m), independent of --bf16 and "
                   "--bf16_mlp: weights and LDS activations rounded to bf16, fp32 sums, heads and outputs; mixed precision, not the same numbers")


def need_device(script):
    if not torch.cuda.is_available():
        raise SystemExit("%s needs a HIP device (no CPU fallback)" % script)


def add_dataset_options(ap):
    from .slac_algo import UNCERTAINTY_TYPES
    ap.add_argument("--real", required=True, help="dataset of real transitions (.npz, or .hdf5 with h5py)")
    ap.add_argument("--gen", help="generated dataset (all_state_1step_random_action) made from the real one")
    ap.add_argument("--uncertainty_type", choices=[t for t in UNCERTAINTY_TYPES if t], default=None)
    ap.add_argument("--uncertainty_penalty_lambda", type=float, default=0.0)


def add_chain_options(ap, fused_chain=None, fused_chain_grad=None, bf16_chain=False, bf16_help=None):
    """--bf16 and the chain switches a script has, in this order.  `bf16_help`, `fused_chain`, `fused_chain_grad`: the script's own
    help text of that option (None: not added here; a script whose --help lists them apart calls twice); `bf16_chain`: whether to add it."""
    for flag, text in (("--bf16", bf16_help), ("--fused_chain", fused_chain), ("--fused_chain_grad", fused_chain_grad),
                       ("--bf16_chain", BF16_CHAIN_HELP if bf16_chain else None)):
        if text:
            ap.add_argument(flag, action="store_true", help=text)


def check_chain_options(ap, a):
    if getattr(a, "bf16_chain", False) and not a.fused_chain:
        ap.error("--bf16_chain needs --fused_chain: the bf16 compute mode exists only in the fused chain kernels")


def chain_settings(a):
    """The parsed switches as `LatentModel`'s attributes / `SlacAlgorithm`'s keywords; a switch the script does not have is off."""
    return dict(fused_chain=getattr(a, "fused_chain", False), fused_chain_grad=getattr(a, "fused_chain_grad", False),
                chain_compute="bf16" if getattr(a, "bf16_chain", False) else "fp32")


def load_latent_pth(latent, directory):
    latent.load_state_dict(torch.load(os.path.join(directory, "latent.pth"), map_location="cpu"), strict=True)


def load_latent(a, state_shape, action_dim):
    """A `LatentModel` in the dtype of --bf16 holding --latent_dir's `latent.pth` (strict), its chains set as the options say."""
    from .slac import LatentModel
    latent = LatentModel(state_shape, (action_dim,), dtype=torch.bfloat16 if a.bf16 else torch.float32, device="cuda:0")
    load_latent_pth(latent, a.latent_dir)
    for k, v in chain_settings(a).items():
        setattr(latent, k, v)
    return latent


def build_algo(a, real, gen, frames_stored=False, **kw):
    """A `SlacAlgorithm` over the arrays `real` (and `gen`, or None) with every window loaded as the reference's `load_data_in_buffer`
    does; with --latent_dir it trains on from that `latent.pth`.  `kw`: the script's batch sizes.  Exits on a buffer without a window."""
    from .slac_algo import SlacAlgorithm
    rows = len(real["actions"]) + (len(gen["actions"]) if gen else 0)
    shape = real["image_observations"].shape
    # frame_capacity: a window stores at most one new frame beyond its episode's reset frame, the generated file its own copy of them
    algo = SlacAlgorithm((shape[3],) + shape[1:3], (real["actions"].shape[1],), 1, "cuda:0", a.seed, buffer_size=max(rows, 1),
                         num_sequences=a.num_sequences, dtype=torch.bfloat16 if a.bf16 else torch.float32,
                         frame_capacity=2 * rows + a.num_sequences + 1, **chain_settings(a), **kw)
    if getattr(a, "latent_dir", None):
        load_latent_pth(algo.latent, a.latent_dir)
    algo.load_data_in_buffer(real)
    if gen is not None:
        algo.load_data_in_buffer(gen, data_num=len(gen["actions"]), uncertainty_type=a.uncertainty_type,
                                 uncertainty_penalty_lambda=a.uncertainty_penalty_lambda, generated_for_slac=True,
                                 data_mix_type="all_state_1step_random_action")
    print("buffer: %d windows (%d real)" % (len(algo.buffer), algo.buffer._real_n) + (", %d frames stored" % algo.buffer._head if frames_stored else ""))
    if len(algo.buffer) == 0:
        raise SystemExit("no window of %d steps in the data" % a.num_sequences)
    return algo


def net_shape(sd, prefix=""):
    """(hidden sizes, input size, output size) of the MLP under `prefix` of a state_dict (`policy.pth`, or a net of `critic.pth`)."""
    hidden = []
    while "%sfc%d.weight" % (prefix, len(hidden)) in sd:
        hidden.append(int(sd["%sfc%d.weight" % (prefix, len(hidden))].shape[0]))
    return hidden, int(sd[prefix + "fc0.weight"].shape[1]), int(sd[prefix + "last_fc.weight"].shape[0])


def policy_input_type(obs_dim, action_dim, context, where="policy.pth", feature_dim=256, z_dim=288):
    """The input type an imagined rollout finds in a `policy.pth` by its obs_dim: None for `latent_z` (z_dim), else S of a
    `feature_action` input S feature_dim + (S - 1) A.  Exits where no integer S >= 2 fits, or --context + 1 < S."""
    if obs_dim == z_dim:
        return None
    S, rem = divmod(obs_dim + action_dim, feature_dim + action_dim)
    if rem or S < 2:
        raise SystemExit("%s reads %d inputs: neither a latent_z policy (obs_dim %d) nor a feature_action policy (obs_dim S * %d + (S - 1) * %d "
                         "for an integer S >= 2)" % (where, obs_dim, z_dim, feature_dim, action_dim))
    if context + 1 < S:
        raise SystemExit("%s is a feature_action policy of %d frames: --context + 1 >= %d is needed, not --context %d" % (where, S, S, context))
    return S


def input_type_name(S):
    return "latent_z" if S is None else "feature_action (%d frames)" % S


def policy_input_dim(a, action_dim, feature_dim=256, z_dim=288):
    """finetune_rl.py:204: S features and S - 1 actions, or the latent."""
    return a.num_sequences * feature_dim + (a.num_sequences - 1) * action_dim if a.slac_policy_input_type == "feature_action" else z_dim


def offline_networks(a, action_dim, z_dim=288):
    """(critic, policy) of an IQL / CQL run: four Q networks and V on the latent, the policy on --slac_policy_input_type's input."""
    from .offline_rl import CriticSLAC, Qfunction, TanhGaussianPolicy, Vfunction
    hid = [a.hidden, a.hidden]
    q = [Qfunction(hidden_sizes=hid, output_size=1, input_size=z_dim + action_dim) for _ in range(4)]
    return (CriticSLAC(q[0], q[1], q[2], q[3], vf=Vfunction(hidden_sizes=hid, output_size=1, input_size=z_dim)),
            TanhGaussianPolicy(hidden_sizes=hid, obs_dim=policy_input_dim(a, action_dim), action_dim=action_dim))


def sample_form(a, algo):
    """The `frames` argument of `random_batch`: with --cache_features, build the feature table first and report its size and time."""
    if not a.cache_features:
        return None
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    algo.cache_features()
    torch.cuda.synchronize()
    t = algo.buffer.features
    print("feature table: %d rows x %d fp32 = %.1f MB, built in %.2f s" % (t.shape[0], t.shape[1], t.numel() * 4 / 1e6,
                                                                         time.perf_counter() - t0))
    return "features"


def run_offline(a, algo, trainer, critic, policy):
    """--steps training steps on batches of the buffer, logged every --log_every, then the four .pth files of the run in --out."""
    frames = sample_form(a, algo)
    for step in range(1, a.steps + 1):
        trainer.train_from_torch(algo.buffer.random_batch(a.batch_size, frames=frames))
        if step % a.log_every == 0 or step == a.steps:
            trainer.end_epoch(step)
            print("step %d  %s" % (step, "  ".join("%s %.4f" % kv for kv in trainer.eval_statistics.items())))
    os.makedirs(a.out, exist_ok=True)
    torch.save(critic.state_dict(), os.path.join(a.out, "critic.pth"))
    torch.save(policy.state_dict(), os.path.join(a.out, "policy.pth"))
    algo.save_model(a.out)
