"""Roll the trained ensemble state-dynamics model over a real dataset (stage between [A] and the generator, SPEC.md N2c) and write
the `all_state_1step_random_action` generated dataset (reference state_transition_rollout.py):

    python rollout_dynamics.py --data real.npz --model_dir world_model/cheetah --iter 50 --out gen_states.npz

--data: an .npz (or .hdf5 where h5py is installed) with the reference's keys `observations`, `actions`, `rewards`,
`next_observations`, `timeouts` (and `terminals`, all zero); every other key, e.g. `image_observations`, is copied to the output.
--model_dir / --iter: the two files train_dynamics.py wrote, normalize_configs_dict.pkl and model_dist_state_dict_<iter>.pkl.
--out: for every row one random action in [--action_low, --action_high] (one value, or one per action column), one random ensemble
member, that member's de-normalised next state and reward, the disagreement / aleatoric uncertainties and the SLAC window index
tables; the input's actions and rewards are kept as `original_actions` / `original_rewards`.  This is the file `augment.py --input`
takes.  A seed reproduces the numpy stream of the reference under `np.random.seed(seed)`.  Needs a HIP device."""
import argparse

from s2p_amd import transition_rollout


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", required=True)
    ap.add_argument("--model_dir", required=True)
    ap.add_argument("--iter", type=int, required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--action_low", type=float, nargs="+", default=[-1.0])
    ap.add_argument("--action_high", type=float, nargs="+", default=[1.0])
    ap.add_argument("--num_sequences", type=int, default=8)
    ap.add_argument("--chunk", type=int, default=16384)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    a.action_low = a.action_low[0] if len(a.action_low) == 1 else a.action_low
    a.action_high = a.action_high[0] if len(a.action_high) == 1 else a.action_high
    return a


def main(argv=None):
    a = parse_args(argv)
    out = transition_rollout.run(a.data, a.model_dir, a.iter, a.out, act_low=a.action_low, act_high=a.action_high, seed=a.seed,
                                 S=a.num_sequences, chunk=a.chunk, device=a.device)
    for k, v in out.items():
        print("key : %s shape : %s %s" % (k, getattr(v, "shape", None), getattr(v, "dtype", "")))
    print("wrote %s (%d rows)" % (a.out, len(out["actions"])))
    return out


if __name__ == "__main__":
    main()
