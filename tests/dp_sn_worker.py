"""Child process of tests/test_spectral_dp_gpu.py: one data-parallel rank running two Pix2PixTrainer iterations (G step + D step)
with --norm_G spectralmatinstance --norm_D spectralinstance (SPEC.md D5s).
Usage: python dp_sn_worker.py RANK WORLD PORT OUTFILE   (global batch 4; every rank shares GPU 0; gloo carries the collectives)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch
    import torch.distributed as dist
    from s2p_amd.options.train_options import TrainOptions
    from s2p_amd.trainers.pix2pix_trainer import Pix2PixTrainer
    if world > 1:
        dist.init_process_group(backend="gloo")
    B = 4
    per = B // world
    opt = TrainOptions().parse(["--env_type", "cheetah", "--batchSize", str(per), "--precision", "bf16", "--gpu_ids", "0",
                                "--checkpoints_dir", os.path.dirname(out), "--norm_G", "spectralmatinstance",
                                "--norm_D", "spectralinstance"], quiet=True)
    torch.manual_seed(7 + rank)                 # ranks start from DIFFERENT weights and u / v: the broadcast must fix that
    tr = Pix2PixTrainer(opt)
    model = tr.pix2pix_model
    g = torch.Generator().manual_seed(99)
    prev = torch.rand(B, 3, 84, 84, generator=g) * 2 - 1
    real = torch.rand(B, 3, 84, 84, generator=g) * 2 - 1
    state = torch.randn(B, 17, generator=g)
    sl = slice(rank * per, (rank + 1) * per)
    data = dict(prev_image=prev[sl], state=state[sl], image=real[sl])
    cpu = lambda t: t.detach().cpu().clone()  # noqa: E731

    def uv():
        torch.cuda.synchronize()
        return [cpu(t) for net in (model.netG, model.netD) for t in (net.store.sn_u, net.store.sn_v)]

    res = dict(world=tr.dp.world_size, uv0=uv())
    w0 = cpu(model.netG.store.master)
    # iteration 1: the gradients (projected, reduced, scaled) of each step against the one-rank run.  As in dp_worker.py, G's
    # initial weights go back before the D step, so that both runs make the same fake (Adam's first step is sign-like where a
    # gradient is ~0); the power iteration depends on the weights alone, so u and v stay bitwise equal to the one-rank run's.
    tr.run_generator_one_step(data)
    res["gG"] = cpu(model.netG.store.grad * tr.optimizer_G.grad_scale)
    model.netG.store.master.copy_(w0.to(model.netG.store.master.device))
    model.netG.store.repack()
    tr.run_discriminator_one_step(data)
    tr.sync()
    res["gD"] = cpu(model.netD.store.grad * tr.optimizer_D.grad_scale)
    res["uv1"] = uv()
    res["losses1"] = {k: float(v) for k, v in tr.get_latest_losses().items()}
    # iteration 2, as the trainer runs it
    tr.run_generator_one_step(data)
    tr.run_discriminator_one_step(data)
    tr.sync()
    res["uv2"] = uv()
    res["wG"], res["wD"] = cpu(model.netG.store.master), cpu(model.netD.store.master)
    res["lrG"], res["lrD"] = tr.optimizer_G.param_groups[0]["lr"], tr.optimizer_D.param_groups[0]["lr"]
    torch.save(res, out)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
