"""train.py -- S2P training (README.md:59):
    python train.py --dataroot=./datasets/cheetah.hdf5 --env_type=cheetah --netG=s2p --batchSize=16 --gpu_ids=0
Multi-GPU: one process per GPU,  python -m torch.distributed.run --nproc-per-node 8 train.py ...  (RCCL all-reduce of
the flat G/D gradient buffers)."""
import time

import torch

from s2p_amd.data import create_dataloader, create_device_loader
from s2p_amd.options.train_options import TrainOptions
from s2p_amd.trainers.pix2pix_trainer import Pix2PixTrainer


def open_loader(opt, trainer):
    """The batches of a run.  --device_data: the dataset lives on the device and one launch per step builds the batch there
    (s2p_amd/data: DeviceDataset); the batches and their order are those of the DataLoader with --nThreads 0."""
    if not opt.device_data:
        return create_dataloader(opt, trainer.dp.rank, trainer.dp.world_size)
    if int(opt.nThreads) and trainer.dp.rank == 0:
        print("warning: --nThreads %d is ignored with --device_data (no batch is built on the host)" % int(opt.nThreads))
    return create_device_loader(opt, trainer.pix2pix_model.device, trainer.dp.rank, trainer.dp.world_size)


class BatchLoop:
    """What the loop does with one batch (tests/tools/bench_train_input.py times exactly this).
    --hip_graph: the G+D step is captured once into hipGraph segments (s2p_amd/stepgraph.py) and replayed; each batch is copied
    into static device buffers first (with --device_data it is gathered straight into them, outside the graph).  The capture
    bakes the learning rate in, so it is redone when the rate changes."""

    def __init__(self, opt, trainer, dl):
        self.opt, self.trainer, self.dl = opt, trainer, dl
        self.graphed = opt.hip_graph and opt.D_steps_per_G == 1
        self.sg, self.static, self.captured_lr, self.warned_graph = None, None, None, False

    def batches(self):
        """One epoch: the loader's batches, or with --device_data --hip_graph their frame numbers alone."""
        return self.dl.batches() if self.opt.device_data and self.graphed else self.dl

    def train_step(self):
        self.trainer.run_generator_one_step(self.static)
        self.trainer.run_discriminator_one_step(self.static)

    def step(self, i, data):
        opt, trainer = self.opt, self.trainer
        if self.graphed:
            from s2p_amd.stepgraph import StepGraph
            if opt.device_data:
                self.static = self.dl.dataset.gather(data, out=self.static)
            else:
                if self.static is None:
                    dev = trainer.pix2pix_model.device
                    self.static = {k: data[k].to(dev, torch.float32).contiguous().clone() for k in ("prev_image", "state", "image")}
                for k in self.static:
                    self.static[k].copy_(data[k], non_blocking=True)
            trained = False
            if self.sg is None or self.captured_lr != trainer.old_lr:
                if self.sg is None:
                    self.train_step()                      # the very first batch is trained on eagerly (allocator / library warm-up)
                    trained = True
                self.sg = StepGraph()
                trainer.seg = self.sg
                self.sg.capture(self.train_step)           # kernels are only RECORDED during capture: no update happens here
                self.captured_lr = trainer.old_lr
            if not trained:
                self.sg.replay()                           # every other batch (also the one a re-capture saw) is trained on by a replay
        else:
            if opt.hip_graph and not self.warned_graph and trainer.dp.rank == 0:
                print("warning: --hip_graph is ignored with --D_steps_per_G %d (the captured step is one G + one D step)" % opt.D_steps_per_G)
                self.warned_graph = True
            if i % opt.D_steps_per_G == 0:
                trainer.run_generator_one_step(data)
            trainer.run_discriminator_one_step(data)


def main(args=None):
    opt = TrainOptions().parse(args, save=True)
    trainer = Pix2PixTrainer(opt)
    dl = open_loader(opt, trainer)
    loop = BatchLoop(opt, trainer, dl)
    total_epochs = opt.niter + opt.niter_decay
    it = trainer.pix2pix_model.iters_done                 # > 0 when resuming with --continue_train
    for epoch in range(trainer.first_epoch, total_epochs + 1):
        if hasattr(dl.sampler, "set_epoch"):
            dl.sampler.set_epoch(epoch)
        t0 = time.time()
        for i, data in enumerate(loop.batches()):
            it += 1
            loop.step(i, data)
            if it % opt.print_freq == 0 and trainer.dp.rank == 0:
                losses = {k: float(v) for k, v in trainer.get_latest_losses().items()}
                print("(epoch %d, iters %d) " % (epoch, it) + " ".join("%s: %.3f" % kv for kv in losses.items()))
        trainer.update_learning_rate(epoch)
        trainer.end_of_epoch(epoch, it)
        if trainer.dp.rank == 0:
            print("End of epoch %d / %d \t Time Taken: %d sec" % (epoch, total_epochs, time.time() - t0))
        if epoch % opt.save_epoch_freq == 0 or epoch == total_epochs:
            trainer.save("latest")
            trainer.save(epoch)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
