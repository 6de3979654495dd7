"""Train the ensemble state-dynamics model (stage [A], SPEC.md N2b) on an offline dataset and write the two files the rollout
loads (reference state_transition_rollout.py:88-100):

    python train_dynamics.py --data dataset.npz --out world_model/cheetah --epochs 50

--data: an .npz with the reference's dataset keys `observations` [n, obs], `actions` [n, act], `next_observations` [n, obs],
`rewards` [n] or [n, 1] (state_transition_rollout.py:61-64).  Writes (torch.save, as the reference torch.load()s them)
  <out>/normalize_configs_dict.pkl          obs_mean, obs_std, next_obs_mean, next_obs_std, reward_mean, reward_std
  <out>/model_dist_state_dict_<epochs>.pkl  the reference module's 18-key state dict, CPU fp32 tensors (strict=True loadable)
The model input is [normalised obs | action], the target [normalised next_obs | normalised reward].  Needs a HIP device."""
import argparse
import os

import numpy as np
import torch

from s2p_amd.dynamics import EnsembleTrainer, EnsembleTransition


def normalisation(data):
    eps = 1e-6
    rew = data["rewards"].reshape(-1)
    return {"obs_mean": data["observations"].mean(0), "obs_std": data["observations"].std(0) + eps,
            "next_obs_mean": data["next_observations"].mean(0), "next_obs_std": data["next_observations"].std(0) + eps,
            "reward_mean": float(rew.mean()), "reward_std": float(rew.std() + eps)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--hidden_features", type=int, default=256)
    ap.add_argument("--hidden_layers", type=int, default=3)
    ap.add_argument("--ensemble_size", type=int, default=7)
    ap.add_argument("--n_elite", type=int, default=5)
    ap.add_argument("--holdout", type=float, default=0.1)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)

    with np.load(a.data) as z:
        data = {k: np.asarray(z[k], np.float32) for k in ("observations", "actions", "next_observations", "rewards")}
    cfg = normalisation(data)
    obs = (data["observations"] - cfg["obs_mean"]) / cfg["obs_std"]
    nobs = (data["next_observations"] - cfg["next_obs_mean"]) / cfg["next_obs_std"]
    rew = (data["rewards"].reshape(-1, 1) - cfg["reward_mean"]) / cfg["reward_std"]
    inputs = torch.from_numpy(np.concatenate([obs, data["actions"]], 1).astype(np.float32))
    targets = torch.from_numpy(np.concatenate([nobs, rew], 1).astype(np.float32))

    model = EnsembleTransition(obs.shape[1], data["actions"].shape[1], a.hidden_features, a.hidden_layers,
                               ensemble_size=a.ensemble_size, device=a.device).init_parameters(a.seed)
    trainer = EnsembleTrainer(model, lr=a.lr)
    info = trainer.fit(inputs, targets, a.epochs, batch_size=a.batch_size, holdout=a.holdout, n_elite=min(a.n_elite, a.ensemble_size),
                       seed=a.seed, log=lambda ep, mse, imp: print("epoch %d holdout mse %s saved %s" % (
                           ep + 1, " ".join("%.4f" % float(v) for v in mse), imp), flush=True))
    os.makedirs(a.out, exist_ok=True)
    torch.save(cfg, os.path.join(a.out, "normalize_configs_dict.pkl"))
    path = os.path.join(a.out, "model_dist_state_dict_%d.pkl" % a.epochs)
    torch.save(model.state_dict(), path)
    print("elites %s; wrote %s" % (info["elites"], path))


if __name__ == "__main__":
    main()
