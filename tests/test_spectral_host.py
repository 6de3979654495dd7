"""CPU: the host side of the opt-in spectral normalization (SPEC.md D5s) -- which layers the options select, the checkpoint
key / column-order mapping to torch.nn.utils.spectral_norm, refusal of mismatched checkpoints, and that the default options
leave the state-dict keys and the flat layout exactly as they were."""
import pytest
import torch

import s2p_oracle as O
from s2p_amd.models import networks
from s2p_amd.options.train_options import TrainOptions


def nets(*extra):
    opt = TrainOptions().parse(["--env_type", "cheetah"] + list(extra), quiet=True)
    return networks.define_G(opt), networks.define_D(opt)


def test_options_select_exactly_the_spade_layers():
    G, D = nets("--norm_D", "spectralinstance", "--norm_G", "spectralmatinstance")
    assert [n for n, _ in G.sn_layers()] == ["blocks.%d.conv_%d" % (b, j) for b in range(6) for j in range(2)]
    assert [n for n, _ in D.sn_layers()] == ["discriminator_%d.model%d" % (k, n) for k in range(2) for n in (1, 2, 3)]
    G, D = nets("--norm_D", "spectralinstance")
    assert G.sn_layers() == [] and len(D.sn_layers()) == 6
    G, D = nets("--norm_G", "spectralmatinstance")
    assert len(G.sn_layers()) == 12 and D.sn_layers() == []
    G, D = nets()
    assert G.sn_layers() == [] and D.sn_layers() == []
    # SPADE's prefix rule (SPEC.md D5s): upstream's default strings select the same layers
    G, D = nets("--norm_D", "spectralbatch", "--norm_G", "spectralspadesyncbatch3x3")
    assert len(G.sn_layers()) == 12 and len(D.sn_layers()) == 6


def test_default_options_keep_state_dict_keys_and_layout():
    G, D = nets()
    spec = O.Spec()
    assert set(G.export_state_dict()) == set(O.generator_param_shapes(spec))
    assert set(D.export_state_dict()) == set(O.discriminator_param_shapes(spec))
    # the flat layout (and so its signature) does not depend on the option: SN adds buffers, not parameters
    for a, b in zip(nets(), nets("--norm_D", "spectralinstance", "--norm_G", "spectralmatinstance")):
        for net in (a, b):
            net._declare_packs(torch.float32)
        names_a = {id(p): n for n, p in a.named_parameters()}
        names_b = {id(p): n for n, p in b.named_parameters()}
        for net in (a, b):                 # offsets as finalize() assigns them, without a device
            off = 0
            for e in net.store.entries:
                e["offset"], off = off, off + e["param"].numel()
        assert a.store.layout_signature(names_a) == b.store.layout_signature(names_b)
        assert b.store.sn and not a.store.sn


def test_checkpoint_names_and_v_order_match_torch_spectral_norm():
    G, D = nets("--norm_D", "spectralinstance", "--norm_G", "spectralmatinstance")
    for net, n in ((D, "discriminator_1.model2"), (G, "blocks.3.conv_1")):
        sd = net.export_state_dict()
        mod = dict(net.sn_layers())[n]
        assert n + ".weight" not in sd
        w = sd[n + ".weight_orig"]
        assert torch.equal(w, mod.weight.detach())
        cout, cin, kh, kw = w.shape
        # the module keeps v in the flat master's (tap, channel) column order; the checkpoint in torch's (channel, tap) order
        v_master = mod.weight_v.reshape(kh, kw, cin)
        v_torch = sd[n + ".weight_v"].reshape(cin, kh, kw)
        assert torch.equal(v_torch, v_master.permute(2, 0, 1))
        # W (torch layout) times v (torch order) == the master matrix times v (master order)
        Wm_master = mod.weight.detach().permute(0, 2, 3, 1).reshape(cout, -1)
        assert torch.allclose(w.reshape(cout, -1) @ sd[n + ".weight_v"], Wm_master @ mod.weight_v, atol=1e-5)
        # a torch module wrapped in spectral_norm takes the keys as they are
        conv = torch.nn.utils.spectral_norm(torch.nn.Conv2d(cin, cout, kh, bias=n.startswith("blocks")))
        part = {k[len(n) + 1:]: v for k, v in sd.items() if k.startswith(n + ".")}
        conv.load_state_dict(part)
        # ... and the round trip through load_state_dict restores the module's own order
        G2, D2 = nets("--norm_D", "spectralinstance", "--norm_G", "spectralmatinstance")
        net2 = G2 if net is G else D2
        net2.load_state_dict(sd)
        m2 = dict(net2.sn_layers())[n]
        assert torch.equal(m2.weight_v, mod.weight_v) and torch.equal(m2.weight_u, mod.weight_u)
        assert torch.equal(m2.weight.detach(), mod.weight.detach())


def test_mismatched_checkpoints_are_refused_naming_the_option():
    G, D = nets()
    Gs, Ds = nets("--norm_D", "spectralinstance", "--norm_G", "spectralmatinstance")
    with pytest.raises(RuntimeError, match="--norm_D spectralinstance"):
        D.load_state_dict(Ds.export_state_dict())
    with pytest.raises(RuntimeError, match="--norm_G spectralmatinstance"):
        G.load_state_dict(Gs.export_state_dict())
    with pytest.raises(RuntimeError, match="--norm_D spectralinstance"):
        Ds.load_state_dict(D.export_state_dict())
    with pytest.raises(RuntimeError, match="--norm_G spectralmatinstance"):
        Gs.load_state_dict(G.export_state_dict())
