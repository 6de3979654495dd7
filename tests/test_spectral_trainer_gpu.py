"""GPU: three fp32 trainer iterations (N = 2, 84x84) with --norm_G spectralmatinstance --norm_D spectralinstance against
float64 (SPEC.md D5s).  Each step of each iteration is re-derived in float64 from the state the HIP trainer started it with:
the power iterations (G step: G once, D once; D step: G once, D once -- two per network per iteration), every loss, the projected
gradient of every parameter as the trainer's Adam sees it (the projection runs inside adam_step), u / v / sigma of all 18 SN
layers, and the Adam update.  The oracle follows the branches the HIP step took (test_model_gpu.py's masks)."""
import pytest
import torch

import s2p_oracle as O
from s2p_amd.models import autograd_nodes
from s2p_amd.options.train_options import TrainOptions
from s2p_amd.params import ParamStore
from test_model_gpu import (_nchw, check_grads, discriminator_masks, dstep_masks, generator_masks, grad_errors, make_inputs,
                            randomize, vgg_masks)
from test_spectral_model_gpu import SN_D, SN_G, sn_ref, sn_state

pytestmark = pytest.mark.gpu


def snapshot(net):
    """float64 CPU copies of the network's parameters (torch layout), u / v (torch order), sigma, Adam m / v, step."""
    st = net.store
    torch.cuda.synchronize()
    names = {id(p): n for n, p in net.named_parameters()}
    P = {n: p.detach().cpu().double() for n, p in net.named_parameters()}
    M, V = {}, {}
    for e in st.entries:
        n = names[id(e["param"])]
        M[n] = ParamStore._view(st.m, e["offset"], e["param"], e["kind"]).detach().cpu().double()
        V[n] = ParamStore._view(st.v, e["offset"], e["param"], e["kind"]).detach().cpu().double()
    sd = net.export_state_dict()
    UV = {d["name"]: (sd[d["name"] + ".weight_u"].double(), sd[d["name"] + ".weight_v"].double()) for d in st.sn}
    sig = {d["name"]: float(st.sn_sigma[i]) for i, d in enumerate(st.sn)}
    step = int(st.step_dev.item()) if st.step_dev is not None else 0
    return dict(P=P, M=M, V=V, UV=UV, sig=sig, step=step)


def sn_apply(P, UV, leaf):
    """One training-mode power iteration of every SN layer: (parameter dict with W / sigma in place of W, {name: (u, v, sigma)})."""
    out = {k: (v.detach().requires_grad_(True) if leaf else v) for k, v in P.items()}
    p_in, ref = dict(out), {}
    for name, (u, v) in UV.items():
        Wsn, u1, v1, s = sn_ref(out[name + ".weight"], u, v, True)
        p_in[name + ".weight"] = Wsn if leaf else Wsn.detach()
        ref[name] = (u1, v1, float(s.detach()))
    return out, p_in, ref


def check_sn(net, ref, what):
    now = snapshot(net)
    for name, (u, v, s) in ref.items():
        U, Vv = now["UV"][name]
        assert float((U - u).abs().max()) <= 1e-5 and float((Vv - v).abs().max()) <= 1e-5, (what, name)
        assert abs(now["sig"][name] - s) <= 1e-5 * abs(s), (what, name, now["sig"][name], s)


def check_adam(net, before, leafs, lr, b1, b2, what):
    """The update of every well-conditioned weight against the oracle's Adam from the same m / v / step (the criterion of
    test_trainer_step_matches_oracle_adam)."""
    new = {n: p.detach().cpu().double() for n, p in net.named_parameters()}
    gmax = max(float(v.grad.abs().max()) for v in leafs.values())
    bad = total = 0
    for k, p0 in before["P"].items():
        g = leafs[k].grad
        if float(g.abs().max()) < 1e-9 * gmax:
            continue                        # structurally zero gradient (conv bias in front of an InstanceNorm)
        p1, _, _ = O.adam_step(p0, g, before["M"][k], before["V"][k], before["step"] + 1, lr, b1, b2)
        big = g.abs() > 0.05 * g.abs().max()
        bad += int((((new[k] - p0) - (p1 - p0)).abs() > 0.02 * lr)[big].sum())
        total += int(big.sum())
    print(f"{what}: {bad} of {total} well-conditioned weights differ from the oracle update by more than 2 % of lr")
    assert total > 1e4 and bad <= 1e-5 * total, (what, bad, total)


def test_three_fp32_iterations_with_both_options_match_float64(hip_device, tmp_path, monkeypatch):
    from s2p_amd.trainers.pix2pix_trainer import Pix2PixTrainer
    # the D step keeps its real half's activations until the backward (instead of running that backward early on a side
    # stream): only so that the oracle can be handed the branches of both halves -- the values are the same either way
    monkeypatch.setattr(autograd_nodes, "DREAL_EARLY_BWD", False)
    N = 2
    opt = TrainOptions().parse(["--env_type", "cheetah", "--batchSize", str(N), "--precision", "fp32", "--gpu_ids", "0",
                                "--checkpoints_dir", str(tmp_path)] + SN_D + SN_G, quiet=True)
    torch.manual_seed(0)
    tr = Pix2PixTrainer(opt)
    model = tr.pix2pix_model
    spec = O.Spec(state_dim=opt.state_dim)
    spec.lambda_feat, spec.lambda_vgg, spec.lambda_l1 = opt.lambda_feat, opt.lambda_vgg, opt.lambda_l1
    pg = randomize(O.init_params(O.generator_param_shapes(spec), 1), 11, 1.0)
    pd = randomize(O.init_params(O.discriminator_param_shapes(spec), 2), 12, 1.0)
    pv = O.init_params(O.vgg_param_shapes(), 3, kaiming=True)
    model.netG.load_state_dict(sn_state(model.netG, pg))
    model.netD.load_state_dict(sn_state(model.netD, pd))
    model.vgg.load_state_dict(pv)
    pv64 = {k: v.double() for k, v in pv.items()}
    prev, state, real = make_inputs(N, 84, 84, 17, seed=31)
    data = dict(prev_image=prev, state=state, image=real)
    p64, s64, r64 = prev.double(), state.double(), real.double()
    lrG, lrD, b1, b2 = opt.lr / 2, opt.lr * 2, 0.0, 0.9
    cap = {}
    backward = tr._backward

    def capture(losses):                     # the branches the HIP forward took, read before its backward frees them
        if "GAN" in losses:
            lnode = losses["GAN"].grad_fn
            m = generator_masks(model.netG, lnode.fake.grad_fn.c)
            m.update(discriminator_masks(model.netD, lnode.dctx, lnode.dctx_r, with_feat_l1=True))
            m.update(vgg_masks(lnode, N))
            cap["g"] = m
        else:
            dnode = losses["D_Fake"].grad_fn
            cap["d"] = dstep_masks(model.netD, dnode, N)
            cap["fake"] = _nchw(dnode.dctx_f[0][0], 6)[:, 3:6].double()
        backward(losses)
    tr._backward = capture

    for it in range(3):
        # ---- G step: G's power iteration, D's power iteration (D forward on fake + real), losses, projected G gradients, Adam
        G0, D0 = snapshot(model.netG), snapshot(model.netD)
        tr.run_generator_one_step(data)
        torch.cuda.synchronize()
        leafG, pg_in, refG = sn_apply(G0["P"], G0["UV"], True)
        _, pd_in, refD = sn_apply(D0["P"], D0["UV"], False)
        L64, _ = O.generator_losses(pg_in, pd_in, pv64, p64, s64, r64, spec, masks=cap.pop("g"))
        sum(L64.values()).backward()
        for k in L64:
            a, b = float(tr.g_losses[k].detach()), float(L64[k].detach())
            assert abs(a - b) <= 1e-4 * max(abs(b), 1e-2), (it, k, a, b)
        check_grads(grad_errors(dict(model.netG.named_parameters()), leafG), 1e-5, "SN G step %d" % it)
        check_sn(model.netG, refG, "G step %d: G" % it)
        check_sn(model.netD, refD, "G step %d: D" % it)
        check_adam(model.netG, G0, leafG, lrG, b1, b2, "Adam G, iteration %d" % it)
        # ---- D step: G's power iteration (no-grad forward of the fake), D's power iteration, losses, projected D gradients, Adam
        G1, D1 = snapshot(model.netG), snapshot(model.netD)
        tr.run_discriminator_one_step(data)
        torch.cuda.synchronize()
        _, _, refG = sn_apply(G1["P"], G1["UV"], False)
        leafD, pd_in, refD = sn_apply(D1["P"], D1["UV"], True)
        D64 = O.discriminator_losses(None, pd_in, p64, s64, r64, spec, masks=cap.pop("d"), fake=cap.pop("fake"))
        sum(D64.values()).backward()
        for k in D64:
            a, b = float(tr.d_losses[k].detach()), float(D64[k].detach())
            assert abs(a - b) <= 1e-4 * max(abs(b), 1e-2), (it, k, a, b)
        check_grads(grad_errors(dict(model.netD.named_parameters()), leafD), 1e-5, "SN D step %d" % it)
        check_sn(model.netG, refG, "D step %d: G" % it)
        check_sn(model.netD, refD, "D step %d: D" % it)
        check_adam(model.netD, D1, leafD, lrD, b1, b2, "Adam D, iteration %d" % it)
