"""N3b measurement: the SLAC latent model at the reference's configuration (B = 32 sequences, S = 8, A = 6, uint8 frames):
(a) prepare_batch-style no-grad encoder + sample_posterior, (b) calculate_loss + backward + torch.optim.Adam.step, fp32 and bf16
conv stacks; warm-up, `iters` calls between two synchronisations, median of `reps` repeats.  Prints the launch count of the
sequential chain per time step.  Yardstick on the same GPU: the plain-torch restatement of tests/slac_latent_ref.py with torch's
own ROCm ops (reported only if torch's conv path runs on this machine)."""
import os, statistics, sys, time
R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("", "oracle", "tests"): sys.path.insert(0, os.path.join(R, p))
import torch
import slac_latent_ref as REF
from slac_chain_util import count_calls
from s2p_amd.slac import LatentModel

B, S, A = 32, 8, 6
WARM, ITERS, REPS = 5, 20, 5


def timed(fn):
    for _ in range(WARM): fn()
    out = []
    for _ in range(REPS):
        torch.cuda.synchronize(); t = time.perf_counter()
        for _ in range(ITERS): fn()
        torch.cuda.synchronize(); out.append((time.perf_counter() - t) / ITERS * 1e3)
    return statistics.median(out), min(out), max(out)


g = torch.Generator().manual_seed(0)
frames = (torch.rand(B, S + 1, 100, 100, 3, generator=g) * 255).to(torch.uint8).cuda()
action, reward = torch.randn(B, S, A, generator=g).cuda(), torch.randn(B, S, 1, generator=g).cuda()
done = (torch.rand(B, S, 1, generator=g) < 0.1).float().cuda()
params = REF.make_params(A)
print("device:", torch.cuda.get_device_name(0), " B=%d S=%d A=%d uint8 frames; %d warm-up, %d iters x %d repeats (median [min, max])" % (B, S, A, WARM, ITERS, REPS))
for dt in (torch.float32, torch.bfloat16):
    m = LatentModel((3, 100, 100), (A,), image_size=100, dtype=dt)
    m.load_state_dict(REF.full_state_dict(params))
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)

    def prepare():
        with torch.no_grad():
            return m.sample_posterior(m.encoder(frames), action)

    def train():
        opt.zero_grad(set_to_none=True)
        sum(m.calculate_loss(frames, action, reward, done)).backward()
        opt.step()

    name = str(dt).split(".")[-1]
    print("%-8s prepare_batch (no-grad encoder + sample_posterior): %.3f ms [%.3f, %.3f]" % ((name,) + timed(prepare)))
    print("%-8s calculate_loss + backward + Adam.step:              %.3f ms [%.3f, %.3f]" % ((name,) + timed(train)))
    if dt == torch.float32:
        feat = m.encoder(frames).detach()
        c1 = count_calls(lambda: m.sample_posterior(feat, action))
        m2 = LatentModel((3, 100, 100), (A,), image_size=100, dtype=dt); m2.load_state_dict(REF.full_state_dict(params))
        f2 = torch.cat([feat, feat[:, -1:]], dim=1); a2 = torch.cat([action, action[:, -1:]], dim=1)
        c2 = count_calls(lambda: m2.sample_posterior(f2, a2))
        print("chain launches per time step, forward: %d (C-ABI calls at S=9 minus S=8)" % (sum(c2.values()) - sum(c1.values())))
        z = m.sample_posterior(feat.requires_grad_(True), action)
        cb1 = count_calls(lambda: (z[2].sum() + z[3].sum() + z[0].sum()).backward())
        z = m2.sample_posterior(f2.requires_grad_(True), a2)
        cb2 = count_calls(lambda: (z[2].sum() + z[3].sum() + z[0].sum()).backward())
        print("chain launches per time step, backward: %d" % (sum(cb2.values()) - sum(cb1.values())))

# yardstick: the same model in plain torch ops on the same GPU
try:
    p = {k: v.cuda().requires_grad_(True) for k, v in params.items()}
    opt = torch.optim.Adam(list(p.values()), lr=1e-4)
    state = frames.permute(0, 1, 4, 2, 3).float() / 255.0
    noise = torch.randn(B, S + 1, 288, device="cuda")
    enc = {k[len("encoder."):]: v for k, v in p.items() if k.startswith("encoder.")}

    def t_prepare():
        with torch.no_grad():
            return REF.sample_posterior(p, REF.SO.encoder_forward(enc, state), action, noise)

    def t_train():
        opt.zero_grad(set_to_none=True)
        sum(REF.calculate_loss(p, state, action, reward, done, noise)[0]).backward()
        opt.step()

    print("torch ops fp32 prepare_batch: %.3f ms [%.3f, %.3f]" % timed(t_prepare))
    print("torch ops fp32 calculate_loss + backward + Adam.step: %.3f ms [%.3f, %.3f]" % timed(t_train))
except Exception as e:                                       # torch's conv path (MIOpen) may be unusable on the machine
    print("torch-ops yardstick not available on this machine: %s: %s" % (type(e).__name__, str(e)[:200]))
