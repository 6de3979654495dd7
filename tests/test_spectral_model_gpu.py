"""GPU: spectral normalization in the networks and the trainer (--norm_D spectralinstance, --norm_G spectralmatinstance;
SPEC.md D5s) against a float64 reference written here: W / sigma fed into the functional oracle, the backward through
W / (u . W v) by torch autograd with u and v detached."""
import os

import pytest
import torch

import s2p_oracle as O
from s2p_amd.models.pix2pix_model import Pix2PixModel
from s2p_amd.options.train_options import TrainOptions
from s2p_amd.models import autograd_nodes
from test_model_gpu import _nchw, check_grads, dstep_masks, grad_errors, make_inputs, randomize, rel_l2

pytestmark = pytest.mark.gpu

SN_D = ["--norm_D", "spectralinstance"]
SN_G = ["--norm_G", "spectralmatinstance"]
EPS = 1e-12


def _normalize(x):
    return x / x.norm().clamp_min(EPS)


def sn_ref(W, u, v, training):
    """torch.nn.utils.spectral_norm in float64: W [Cout, Cin, kh, kw], u, v in torch's order.  Returns (W / sigma, u', v', sigma)
    with u', v' detached (as the hook does)."""
    Wm = W.reshape(W.shape[0], -1)
    with torch.no_grad():
        if training:
            v = _normalize(Wm.t() @ u)
            u = _normalize(Wm @ v)
    sigma = u @ (Wm @ v)
    return W / sigma, u, v, sigma


def sn_state(net, plain):
    """A state dict for an SN network: the plain oracle weights, each SN layer's under `weight_orig`, and the network's own
    current u / v."""
    sd = net.export_state_dict()
    for k, t in plain.items():
        sd[k + "_orig" if k[:-len(".weight")] in dict(net.sn_layers()) and k.endswith(".weight") else k] = t
    return sd


def build_sn(precision, tmp_path, extra):
    opt = TrainOptions().parse(["--env_type", "cheetah", "--batchSize", "2", "--precision", precision, "--gpu_ids", "0",
                                "--checkpoints_dir", str(tmp_path)] + list(extra), quiet=True)
    model = Pix2PixModel(opt)
    spec = O.Spec(state_dim=opt.state_dim)
    pg = randomize(O.init_params(O.generator_param_shapes(spec), 1), 11, 1.0)
    pd = randomize(O.init_params(O.discriminator_param_shapes(spec), 2), 12, 1.0)
    model.netG.load_state_dict(sn_state(model.netG, pg))
    model.netD.load_state_dict(sn_state(model.netD, pd))
    return opt, model, spec, pg, pd


def uv_torch(net):
    sd = net.export_state_dict()
    return {n: (sd[n + ".weight_u"].double(), sd[n + ".weight_v"].double()) for n, _ in net.sn_layers()}


def test_discriminator_training_forward_matches_oracle(hip_device, tmp_path):
    opt, model, spec, pg, pd = build_sn("fp32", tmp_path, SN_D)
    netD = model.netD
    uv0 = uv_torch(netD)
    prev, _, real = make_inputs(2, 84, 84, 17, seed=3)
    x = torch.cat([prev, real], 1)
    feats = netD(x.cuda())                     # training mode: one power iteration first
    torch.cuda.synchronize()
    p64 = {k: v.double() for k, v in pd.items()}
    uv1 = uv_torch(netD)
    for name, (u, v) in uv0.items():
        Wsn, u1, v1, _ = sn_ref(p64[name + ".weight"], u, v, True)
        p64[name + ".weight"] = Wsn
        assert (uv1[name][0] - u1).abs().max() <= 1e-5 and (uv1[name][1] - v1).abs().max() <= 1e-5, name
    ref = O.multiscale_discriminator(p64, x.double(), spec)
    for k, (fs, rs) in enumerate(zip(feats, ref)):
        for j, (f, r) in enumerate(zip(fs, rs)):
            err = rel_l2(f.cpu(), r)
            assert err < 1e-5, (k, j, err)             # the bound of the default path's fp32 feature tests


def test_generator_eval_forward_uses_stored_uv(hip_device, tmp_path):
    opt, model, spec, pg, pd = build_sn("fp32", tmp_path, SN_G)
    netG = model.netG.eval()
    uv0 = uv_torch(netG)
    prev, state, _ = make_inputs(2, 84, 84, 17, seed=4)
    with torch.no_grad():
        y = netG(prev.cuda(), state.cuda()).cpu()
        y2 = netG(prev.cuda(), state.cuda()).cpu()
    assert torch.equal(y, y2)
    uv1 = uv_torch(netG)
    p64 = {k: v.double() for k, v in pg.items()}
    for name, (u, v) in uv0.items():
        assert torch.equal(uv1[name][0], u) and torch.equal(uv1[name][1], v), name
        p64[name + ".weight"] = sn_ref(p64[name + ".weight"], u, v, False)[0]
    y_ref = O.generator_forward(p64, prev.double(), state.double(), spec)
    err = rel_l2(y, y_ref)
    assert err < 1e-5, err


def test_dstep_with_sn_matches_oracle(hip_device, tmp_path):
    """D step with --norm_D spectralinstance (fp32): one power iteration, losses and projected weight gradients against float64."""
    opt, model, spec, pg, pd = build_sn("fp32", tmp_path, SN_D + SN_G)
    prev, state, real = make_inputs(2, 84, 84, 17, seed=21)
    data = dict(prev_image=prev.cuda(), state=state.cuda(), image=real.cuda())
    with torch.no_grad():
        model(data, mode="generator")          # advances u, v of both networks once
    uvD = uv_torch(model.netD)
    model.netD.store.zero_grad()
    d_losses = model(data, mode="discriminator")
    dnode = d_losses["D_Fake"].grad_fn
    dmasks = dstep_masks(model.netD, dnode, 2)
    fake_hip = _nchw(dnode.dctx_f[0][0], 6)[:, 3:6].double()
    sum(d_losses.values()).backward()
    model.netD.store.sn_project_grad()
    torch.cuda.synchronize()
    pd64 = {k: v.detach().double().requires_grad_(True) for k, v in pd.items()}
    p_in = dict(pd64)
    for name, (u, v) in uvD.items():
        p_in[name + ".weight"] = sn_ref(pd64[name + ".weight"], u, v, True)[0]
    D64 = O.discriminator_losses(None, p_in, prev.double(), state.double(), real.double(), spec, masks=dmasks, fake=fake_hip)
    sum(D64.values()).backward()
    for k in D64:
        a, b = float(d_losses[k].detach()), float(D64[k].detach())
        assert abs(a - b) <= 1e-4 * max(abs(b), 1e-2), (k, a, b)
    check_grads(grad_errors(dict(model.netD.named_parameters()), pd64), 1e-5, "SN D step")


def test_dstep_with_sn_recomputes_the_real_pass_bitwise(hip_device, tmp_path, monkeypatch):
    """With D spectral norm the D step's power iteration changes sigma, so the real pass the G step left in model._dreal_cache
    must not be reused: the D step's gradients are bitwise those of a D step that may not reuse it (DREAL_REUSE off), run from
    the same u / v.  bf16, as test_dstep_reuses_the_gstep_real_pass: the fp32 weight-gradient path accumulates with atomics."""
    opt, model, spec, pg, pd = build_sn("bf16", tmp_path, SN_D + SN_G)
    prev, state, real = make_inputs(2, 84, 84, 17, seed=21)
    data = dict(prev_image=prev.cuda(), state=state.cuda(), image=real.cuda())
    with torch.no_grad():
        model(data, mode="generator")
    assert model._dreal_cache is not None
    sn_bufs = [t for st in (model.netG.store, model.netD.store) for t in (st.sn_u, st.sn_v)]
    uv_before = [t.clone() for t in sn_bufs]

    def d_step():
        model.netD.store.zero_grad()
        sum(model(data, mode="discriminator").values()).backward()
        torch.cuda.synchronize()
        return model.netD.store.grad.clone(), [t.clone() for t in sn_bufs]

    g_step, uv_after = d_step()
    for t, b in zip(sn_bufs, uv_before):
        t.copy_(b)
    monkeypatch.setattr(autograd_nodes, "DREAL_REUSE", False)
    g_fresh, uv_fresh = d_step()
    assert torch.equal(g_step, g_fresh)
    assert all(torch.equal(a, b) for a, b in zip(uv_after, uv_fresh))


def _trainer(tmp_path, extra=(), sub="a"):
    from s2p_amd.trainers.pix2pix_trainer import Pix2PixTrainer
    opt = TrainOptions().parse(["--env_type", "cheetah", "--batchSize", "2", "--precision", "bf16", "--gpu_ids", "0",
                                "--checkpoints_dir", os.path.join(str(tmp_path), sub)] + SN_D + SN_G + list(extra), quiet=True)
    torch.manual_seed(0)
    return Pix2PixTrainer(opt)


def _snapshot(tr):
    m = tr.pix2pix_model
    torch.cuda.synchronize()
    return [t.detach().cpu().clone() for net in (m.netG, m.netD) for t in (net.store.master, net.store.sn_u, net.store.sn_v)]


def test_trainer_is_deterministic_and_resumes_bitwise(hip_device, tmp_path):
    prev, state, real = make_inputs(2, 84, 84, 17, seed=7)
    data = dict(prev_image=prev, state=state, image=real)

    def run(tr, n):
        for _ in range(n):
            tr.run_generator_one_step(data)
            tr.run_discriminator_one_step(data)

    a = _trainer(tmp_path, sub="a")
    run(a, 3)
    sa = _snapshot(a)
    b = _trainer(tmp_path, sub="b")
    run(b, 2)
    b.save("latest")
    run(b, 1)
    for x, y in zip(sa, _snapshot(b)):
        assert torch.equal(x, y)
    ck = torch.load(os.path.join(str(tmp_path), "b", "cheetah_latest.pth"), map_location="cpu")
    snG = ["blocks.%d.conv_%d" % (i, j) for i in range(6) for j in range(2)]
    snD = ["discriminator_%d.model%d" % (i, n) for i in range(2) for n in (1, 2, 3)]
    for key, names in (("netG", snG), ("netD", snD)):
        sd = ck[key]
        assert {k.rsplit(".", 1)[0] for k in sd if k.endswith(("_orig", "_u", "_v"))} == set(names)
        for n in names:
            assert n + ".weight" not in sd and {n + ".weight_orig", n + ".weight_u", n + ".weight_v"} <= set(sd)
    # resume from the file written after two iterations: one more iteration is bitwise the uninterrupted third
    c = _trainer(tmp_path, extra=["--continue_train", "--which_epoch", "latest"], sub="b")
    run(c, 1)
    for x, y in zip(sa, _snapshot(c)):
        assert torch.equal(x, y)
    # the checkpoint loads into torch modules wrapped in spectral_norm: W_sn (eval) and one power iteration (train)
    sd = ck["netD"]
    n = "discriminator_0.model2"
    w = sd[n + ".weight_orig"]
    conv = torch.nn.utils.spectral_norm(torch.nn.Conv2d(w.shape[1], w.shape[0], 4, bias=False))
    conv.load_state_dict({"weight_orig": w, "weight_u": sd[n + ".weight_u"], "weight_v": sd[n + ".weight_v"]})
    Wm = w.double().reshape(w.shape[0], -1)
    u, v = sd[n + ".weight_u"].double(), sd[n + ".weight_v"].double()
    conv.eval()
    conv(torch.zeros(1, w.shape[1], 8, 8))
    assert torch.allclose(conv.weight.double(), w.double() / (u @ (Wm @ v)), rtol=1e-5, atol=1e-7)
    conv.train()
    conv(torch.zeros(1, w.shape[1], 8, 8))
    Wsn, u1, v1, _ = sn_ref(w.double(), u, v, True)
    assert torch.allclose(conv.weight_u.double(), u1, atol=1e-5) and torch.allclose(conv.weight_v.double(), v1, atol=1e-5)
    assert torch.allclose(conv.weight.double(), Wsn, rtol=1e-5, atol=1e-7)


def test_graph_replay_matches_eager_bitwise_bs64(hip_device, tmp_path):
    """bf16, bs 64, both options: three eager iterations and (one eager + capture + two replays) give bitwise equal masters, u and
    v -- the captured refresh launches advance u and v exactly once per forward on every replay, and the capture pass runs none."""
    from s2p_amd.stepgraph import StepGraph
    prev, state, real = make_inputs(64, 84, 84, 17, seed=9)

    def make(sub):
        tr = _trainer(tmp_path, extra=["--batchSize", "64"], sub=sub)
        static = {k: t.cuda().contiguous() for k, t in (("prev_image", prev), ("state", state), ("image", real))}

        def step():
            tr.run_generator_one_step(static)
            tr.run_discriminator_one_step(static)
        return tr, step

    a, step_a = make("eager")
    for _ in range(3):
        step_a()
    b, step_b = make("graph")
    step_b()
    sg = StepGraph()
    b.seg = sg
    sg.capture(step_b)
    for _ in range(2):
        sg.replay()
    for x, y in zip(_snapshot(a), _snapshot(b)):
        assert torch.equal(x, y)
