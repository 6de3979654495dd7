"""N3p -- the posterior chain under grad in bf16 compute: s2p_posterior_chain_fwd_save_bf16, s2p_posterior_chain_bwd_bf16,
s2p_chain_pack_bf16, `LatentModel.chain_grad_compute`.

The forward's outputs are BITWISE those of the no-grad bf16 chain; what it saves and what the backward writes are checked LAYER BY
LAYER from the kernel's own buffers: each layer is recomputed in fp64 from the fp32 tensor upstream of it, rounded as the rule says,
and every element must lie within (K + 4) 2^-23 (sum |x w| + |add| + |bias|) -- K fp32 additions of the matrix core plus the
epilogue's -- so no rounding flip of a free-running chain enters.  The heads are bitwise the stand-alone head launches.  End to end
the gradients are held to N3m's loose rule against the fp64 run of tests/chain_grad_bf16_ref.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import chain_bf16_ref as C
import chain_grad_bf16_ref as G
import slac_latent_ref as R
from guard_region import SENT, Region
from slac_chain_util import build_model, count_calls, model_cache

pytestmark = pytest.mark.gpu
Z1, Z2, Z, FEAT, HID = 32, 256, 288, 256, 256
BS, TS, AS = (1, 15, 16, 17, 33), (1, 2, 3, 9), (6, 1)
HEADS = G.CHAIN_HEADS
COLS = (slice(0, FEAT), slice(0, Z1), slice(FEAT, FEAT + Z2), slice(0, Z))
STATE = ("a0_h1", "a0_h2", "a0_raw", "b0_h1", "b0_h2", "b0_raw", "h1a", "h2a", "rawa", "h1b", "h2b", "rawb", "xz")
GRADS = ("drawa", "dh2a", "dh1a", "drawb", "dh2b", "dh1b", "dxz")
U = 2.0 ** -23


@pytest.fixture(scope="module")
def models(hip_device):
    """action width -> a LatentModel with the seeded weights of tests/slac_latent_ref.py; left with every switch off."""
    return model_cache()


def _inputs(B, T, A, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 100 * T + A)
    feat, action, noise = torch.randn(33, T, FEAT, generator=g), torch.randn(33, T - 1, A, generator=g), torch.randn(33, T, Z, generator=g)
    gout = [torch.randn(33, T, c, generator=g) for c in (Z1, Z1, Z1, Z2)]               # dL/d(mean, std, z1, z2)
    return feat[:B].cuda(), action[:B].cuda(), noise[:B].cuda(), [t[:B].cuda() for t in gout]  # row b is the same whatever B is


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _direct(m, feat, action, noise, gout=None):
    """Both entry points on buffers of this test's own -> dict of every tensor they read and wrote (device)."""
    from s2p_amd import ops
    from s2p_amd.slac import _PosteriorFn
    B, T, _ = feat.shape
    S = T - 1
    heads = [getattr(m, h) for h in HEADS]
    pk, pf = [g.packed_bf16_grad() for g in heads], [g.packed() for g in heads]
    ra = rb = None
    if S > 0:
        ra, rb = _PosteriorFn._hoisted(feat, action, pf[2], pf[3])[2:]
    r = dict(mean=_nan(B, T, Z1), std=_nan(B, T, Z1), z=_nan(B, T, Z), ra=ra, rb=rb, pk=pk)
    st = [_nan(B, HID), _nan(B, HID), _nan(B, 64), _nan(B, HID), _nan(B, HID), _nan(B, 512)]
    if S > 0:
        st += [_nan(S, B, HID), _nan(S, B, HID), _nan(S, B, 64), _nan(S, B, HID), _nan(S, B, HID), _nan(S, B, 512), _nan(S, B, Z)]
    state = ops.chain_state(st[:3], st[3:6], st[6:] if S > 0 else None)
    ops.posterior_chain_fwd_save_bf16(feat[:, 0], ra, rb, noise, [ops.chain_mlp_bf16(p) for p in pk], r["mean"], r["std"], r["z"], state)
    r.update(zip(STATE, st))
    if S > 0 and gout is not None:
        gr = [_nan(S, B, 64), _nan(S, B, HID), _nan(S, B, HID), _nan(S, B, 512), _nan(S, B, HID), _nan(S, B, HID), _nan(S, B, Z)]
        r.update(dmean=gout[0].contiguous(), dstd=gout[1].contiguous(), dz=torch.cat(gout[2:], -1).contiguous())
        ops.posterior_chain_bwd_bf16(noise, r["dmean"], r["dstd"], r["dz"], [ops.chain_mlp_bwd_bf16(pk[2]), ops.chain_mlp_bwd_bf16(pk[3])],
                                     state, gr)
        r.update(zip(GRADS, gr))
    torch.cuda.synchronize()
    return r


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(a, b), (what, int((a != b).sum()), a.numel())


def _same_run(a, b, what, rows=None):
    for k in ("mean", "std", "z") + STATE + GRADS:
        if k in a:
            x, y = a[k], b[k]
            if rows is not None:                                 # a: one row alone; b: the full call
                lead = x.dim() - 2 if k in STATE[6:] + GRADS else 0
                y = y.select(lead, rows).unsqueeze(lead)
            _same(x, y, what + (k,))


# ---- 1. forward outputs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("A", AS)
def test_outputs_are_bitwise_the_no_grad_bf16_chain(models, A, T):
    from s2p_amd import ops
    m = models(A)
    for B in BS:
        feat, action, noise, _ = _inputs(B, T, A)
        r = _direct(m, feat, action, noise)
        want = [_nan(B, T, Z1), _nan(B, T, Z1), _nan(B, T, Z)]
        ops.posterior_chain_fwd_bf16(feat[:, 0], r["ra"], r["rb"], noise, [ops.chain_mlp_bf16(getattr(m, h).packed_bf16()) for h in HEADS], *want)
        torch.cuda.synchronize()
        for name, w in zip(("mean", "std", "z"), want):
            assert bool(torch.isfinite(w).all())
            _same(r[name], w, (A, T, B, name))
        for k in STATE[:6 if T == 1 else 13]:
            assert bool(torch.isfinite(r[k]).all()), (A, T, B, k)


def _parts(p, name, cols, x, add, dtype):
    """h1, h2, raw of one MLP under the rule (tests/chain_bf16_ref.py's mlp, which returns only the head's results)."""
    w = lambda i: p["%s.net.%d.weight" % (name, i)]
    b = lambda i: p["%s.net.%d.bias" % (name, i)].to(dtype)
    acc = C._dot(x, w(0)[:, cols], dtype, None)
    h1 = F.leaky_relu((acc + add.to(dtype)) + b(0) if add is not None else acc + b(0), 0.2)
    h2 = F.leaky_relu(C._dot(h1, w(2), dtype, None) + b(2), 0.2)
    return h1, h2, C._dot(h2, w(4), dtype, None) + b(4)


@pytest.mark.parametrize("A", AS)
def test_state_on_exact_data_is_the_rule_bitwise(hip_device, A):
    """On data whose every fp32 sum is exact (eps = 0, so z = mean): the free-running fp64 run of the rule, layer by layer."""
    B, T = 17, 3
    from s2p_amd.slac import LatentModel
    p = C.exact_params(A)
    m = LatentModel((3, 100, 100), (A,), image_size=100)
    m.load_state_dict(R.full_state_dict(p), strict=True)
    feat, action, noise = C.exact_inputs(B, T, A)
    r = _direct(m, feat.cuda(), action.cuda(), noise.cuda())
    ra, rb = C.hoisted_posterior(p, feat, action, torch.float64)
    assert torch.equal(ra.float().reshape(-1, HID), r["ra"].cpu()) and torch.equal(rb.float().reshape(-1, HID), r["rb"].cpu())
    dt = torch.float64
    want = dict(zip(STATE[:3], _parts(p, HEADS[0], COLS[0], feat[:, 0], None, dt)))
    z1 = want["a0_raw"][:, :Z1]
    want.update(zip(STATE[3:6], _parts(p, HEADS[1], COLS[1], z1, None, dt)))
    z2 = want["b0_raw"][:, :Z2]
    chain = [[] for _ in range(7)]
    for t in range(1, T):
        a = _parts(p, HEADS[2], COLS[2], z2, ra[t - 1], dt)
        z1 = a[2][:, :Z1]
        xz = torch.cat([z1, z2], -1)
        b = _parts(p, HEADS[3], COLS[3], xz, rb[t - 1], dt)
        z2 = b[2][:, :Z2]
        for c, v in zip(chain, a + b + (xz,)):
            c.append(v)
    want.update(zip(STATE[6:], (torch.stack(c) for c in chain)))
    for k in STATE:
        got = r[k].cpu()
        assert float(got.abs().max()) > 0
        _same(got, want[k].float(), ("exact", A, k))


# ---- 2. saved state, from the kernel's own tensors ------------------------------------------------------------------------------------------
def _layer_ok(x, w, bias, add, got, act, what):
    """got = [lrelu]((bf(x) . bf(w)^T (+ add)) + bias) within (K + 4) 2^-23 (sum |x w| + |add| + |bias|), everything fp64 on the CPU."""
    xh, wh = C.bf(x.double().cpu()), C.bf(w.double().cpu())
    K = xh.shape[-1]
    acc, mag = xh @ wh.t(), xh.abs() @ wh.abs().t() + bias.double().cpu().abs()
    if add is not None:
        acc, mag = acc + add.double().cpu(), mag + add.double().cpu().abs()
    want = acc + bias.double().cpu()
    if act:
        want = F.leaky_relu(want, 0.2)
    err, bound = (got.double().cpu() - want).abs(), (K + 4) * U * mag
    print("%-28s K %3d worst err / bound %.3f" % (what, K, float((err / bound).max())))
    assert bool((err <= bound).all()), (what, float((err / bound).max()))
    return float((err / bound).max())


@pytest.mark.parametrize("B,T,A", [(17, 3, 6), (33, 9, 6), (16, 2, 1), (1, 1, 6)])
def test_saved_state_layer_by_layer(models, B, T, A):
    from s2p_amd import ops
    m = models(A)
    feat, action, noise, _ = _inputs(B, T, A)
    r = _direct(m, feat, action, noise)
    S = T - 1
    mean, std, z = r["mean"], r["std"], r["z"]
    par = lambda h, i: (getattr(m, h).net._modules[str(i)].weight.detach(), getattr(m, h).net._modules[str(i)].bias.detach())
    # the samples in the saved input rows, the means in raw
    _same(r["a0_raw"][:, :Z1], mean[:, 0], "a0 raw | mean")
    if S > 0:
        _same(r["xz"][:, :, :Z1], z[:, 1:, :Z1].transpose(0, 1), "xz | z1")
        _same(r["xz"][:, :, Z1:], z[:, :-1, Z1:].transpose(0, 1), "xz | z2")
        _same(r["rawa"][:, :, :Z1], mean[:, 1:].transpose(0, 1), "rawa | mean")
    # the head of gauss_dev.h on the saved raw reproduces what the chain returned
    for t in range(T):
        ra_, rb_ = (r["a0_raw"], r["b0_raw"]) if t == 0 else (r["rawa"][t - 1], r["rawb"][t - 1])
        hm, hs, hz1, hz2 = _nan(B, Z1), _nan(B, Z1), _nan(B, Z1), _nan(B, Z2)
        ops.gauss_head_fwd(ra_, Z1, eps=noise[:, t, :Z1], mean=hm, std=hs, z=hz1)
        ops.gauss_head_fwd(rb_, Z2, eps=noise[:, t, Z1:], z=hz2)
        torch.cuda.synchronize()
        for name, a, b in (("mean", hm, mean[:, t]), ("std", hs, std[:, t]), ("z1", hz1, z[:, t, :Z1]), ("z2", hz2, z[:, t, Z1:])):
            _same(a, b, ("head", t, name))
    # every layer from its saved input
    worst = 0.0
    jobs = [("a0", HEADS[0], COLS[0], feat[:, 0], None, r["a0_h1"], r["a0_h2"], r["a0_raw"]),
            ("b0", HEADS[1], COLS[1], z[:, 0, :Z1], None, r["b0_h1"], r["b0_h2"], r["b0_raw"])]
    if S > 0:
        f2 = lambda t: t.reshape(S * B, t.shape[-1])
        jobs += [("a", HEADS[2], COLS[2], f2(r["xz"])[:, Z1:], r["ra"], f2(r["h1a"]), f2(r["h2a"]), f2(r["rawa"])),
                 ("b", HEADS[3], COLS[3], f2(r["xz"]), r["rb"], f2(r["h1b"]), f2(r["h2b"]), f2(r["rawb"]))]
    for tag, h, cols, x, add, h1, h2, raw in jobs:
        (w1, b1), (w2, b2), (w3, b3) = par(h, 0), par(h, 2), par(h, 4)
        worst = max(worst, _layer_ok(x, w1[:, cols], b1, add, h1, True, tag + " h1"), _layer_ok(h1, w2, b2, None, h2, True, tag + " h2"),
                    _layer_ok(h2, w3, b3, None, raw, False, tag + " raw"))
    assert worst > 0


# ---- 3. backward, layer by layer, from the kernel's own buffers ------------------------------------------------------------------------------
def _dgrad_ok(g, w, got, what, more=None):
    """got = bf(g) . bf(w) (+ a second sum `more` = (g, w)) within (N + 4) 2^-23 (sum |g w| (+ the second sum's))."""
    gh, wh = C.bf(g.double().cpu()), C.bf(w.double().cpu())
    N = gh.shape[-1]
    want, mag = gh @ wh, gh.abs() @ wh.abs()
    if more is not None:
        g2, w2 = C.bf(more[0].double().cpu()), C.bf(more[1].double().cpu())
        want, mag = want + g2 @ w2, mag + g2.abs() @ w2.abs()
    err, bound = (got.double().cpu() - want).abs(), (N + 4) * U * mag
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print("%-28s N %3d worst err / bound %.3f" % (what, N, ratio))
    assert bool((err <= bound).all()), (what, ratio)


@pytest.mark.parametrize("T", (2, 3, 9))
@pytest.mark.parametrize("B", (17, 33))
def test_backward_layer_by_layer(models, B, T):
    from s2p_amd import ops
    A, S = 6, T - 1
    m = models(A)
    feat, action, noise, gout = _inputs(B, T, A)
    r = _direct(m, feat, action, noise, gout)
    W = lambda h, i: getattr(m, h).net._modules[str(i)].weight.detach()
    dact = lambda dh, h: dh * torch.where(h > 0, 1.0, 0.2).float()                # ONE fp32 multiply, as the kernel does it
    for k in GRADS:
        assert bool(torch.isfinite(r[k]).all()) and float(r[k].abs().max()) > 0, k
    for t in range(S, 0, -1):
        s = t - 1
        db, da = _nan(B, 512), _nan(B, 64)
        ops.gauss_head_bwd(r["rawb"][s], Z2, db, eps=noise[:, t, Z1:], dz=r["dz"][:, t, Z1:], dz2=r["dxz"][t][:, Z1:] if t < S else None)
        ops.gauss_head_bwd(r["rawa"][s], Z1, da, eps=noise[:, t, :Z1], dmean=r["dmean"][:, t], dstd=r["dstd"][:, t], dz=r["dz"][:, t, :Z1],
                           dz2=r["dxz"][s][:, :Z1])
        torch.cuda.synchronize()
        _same(r["drawb"][s], db, ("drawb", t))
        _same(r["drawa"][s], da, ("drawa", t))
    f2 = lambda k: r[k].reshape(S * B, -1)
    _dgrad_ok(f2("drawb"), W(HEADS[3], 4), f2("dh2b"), "dh2b")
    _dgrad_ok(dact(f2("dh2b"), f2("h2b")), W(HEADS[3], 2), f2("dh1b"), "dh1b")
    _dgrad_ok(f2("drawa"), W(HEADS[2], 4), f2("dh2a"), "dh2a")
    _dgrad_ok(dact(f2("dh2a"), f2("h2a")), W(HEADS[2], 2), f2("dh1a"), "dh1a")
    gb, ga = dact(f2("dh1b"), f2("h1b")), dact(f2("dh1a"), f2("h1a"))
    wb, wa = W(HEADS[3], 0)[:, COLS[3]], W(HEADS[2], 0)[:, COLS[2]]
    _dgrad_ok(gb, wb[:, :Z1], f2("dxz")[:, :Z1], "dxz[:, :32]")
    _dgrad_ok(gb, wb[:, Z1:], f2("dxz")[:, Z1:], "dxz[:, 32:]", more=(ga, wa))


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------------
def test_gradients_end_to_end_against_the_rule(models, capsys):
    A, B, T = 6, 8, 3
    m = models(A)
    p = R.make_params(A)
    keys = G.param_keys()
    named = dict(m.named_parameters())
    params = [named[k] for k in keys]
    loose, got_dev, far = 0.0, {}, {}
    for seed in (0, 1, 2):
        feat, action, noise = C.random_inputs(B, T, A, seed)
        w = G.loss_weights(B, T, seed)
        ref = G.gradients(p, feat, action, noise, w, torch.float64)
        for gen in (None, torch.Generator().manual_seed(9 + seed)):
            loose = max(loose, max(G.deviation(G.gradients(p, feat, action, noise, w, torch.float32, gen), ref).values()))
        res = {}
        for mode in ("bf16", "fp32"):
            m.fused_chain_grad, m.chain_grad_compute = True, mode
            try:
                f, a = feat.cuda().requires_grad_(True), action.cuda().requires_grad_(True)
                mean, std, z1, z2 = m.sample_posterior(f, a, noise.cuda())
                assert (mean.grad_fn.bf16_packs is not None) == (mode == "bf16")
                loss = sum((o * x.cuda()).sum() for o, x in zip((mean, std, torch.cat([z1, z2], -1)), w))
                res[mode] = dict(zip(["dfeat", "daction"] + keys, torch.autograd.grad(loss, [f, a] + params)))
                torch.cuda.synchronize()
            finally:
                m.fused_chain_grad, m.chain_grad_compute = False, "fp32"
        for k, v in G.deviation(res["bf16"], ref).items():
            got_dev[k] = max(got_dev.get(k, 0.0), v)
        for k, v in G.deviation(res["bf16"], {k: v.double().cpu() for k, v in res["fp32"].items()}).items():
            far[k] = max(far.get(k, 0.0), v)
    bound = 4.0 * max(loose, 1e-6)
    with capsys.disabled():
        print("\nhelper fp32 runs: largest deviation %.3e -> bound %.3e" % (loose, bound))
        for k in ["dfeat", "daction"] + keys:
            print("  %-36s deviation from the rule %.3e   distance from the fp32 fused form %.3e" % (k, got_dev[k], far[k]))
    assert len(got_dev) == 26
    for k, v in got_dev.items():
        assert v <= bound, (k, v, bound)


# ---- 5. rows and repeats -------------------------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_their_tile_and_calls_repeat(models):
    A, T = 6, 3
    m = models(A)
    feat, action, noise, gout = _inputs(33, T, A)
    full, again = _direct(m, feat, action, noise, gout), _direct(m, feat, action, noise, gout)
    _same_run(again, full, ("repeat",))
    for row in (0, 32):                                      # the first row of the first tile, the only row of the last one
        q = slice(row, row + 1)
        _same_run(_direct(m, feat[q], action[q], noise[q], [t[q] for t in gout]), full, ("row", row), rows=row)
    bad = 16                                                 # the first row of the second tile; rows 17..31 share its tile
    others = [i for i in range(33) if i != bad]
    fnan, gnan = feat.clone(), [t.clone() for t in gout]
    fnan[bad, 0] = float("nan")
    got = _direct(m, fnan, action, noise, gout)
    assert bool(torch.isnan(got["z"][bad]).all()) and bool(torch.isnan(got["dxz"][:, bad]).any())
    gnan[3][bad] = float("nan")
    got2 = _direct(m, feat, action, noise, gnan)
    assert bool(torch.isnan(got2["dxz"][:, bad]).all())
    for g in (got, got2):
        for k in ("mean", "std", "z") + STATE + GRADS:
            lead = g[k].dim() - 2 if k in STATE[6:] + GRADS else 0
            _same(g[k].index_select(lead, torch.tensor(others, device="cuda")), full[k].index_select(lead, torch.tensor(others, device="cuda")), ("nan", k))


def _model_run(m, feat, action, noise, gout, mode, flip=None):
    """A grad-mode sample_posterior with fused_chain_grad and its backward -> (outputs, gradients, calls forward, calls backward)."""
    keys = G.param_keys()
    named = dict(m.named_parameters())
    m.fused_chain_grad, m.chain_grad_compute = True, mode
    try:
        f, a = feat.clone().requires_grad_(True), action.clone().requires_grad_(True)
        box = {}
        cf = count_calls(lambda: box.setdefault("out", m.sample_posterior(f, a, noise)))
        if flip is not None:
            m.chain_grad_compute = flip
        cb = count_calls(lambda: box.setdefault("g", torch.autograd.grad(box["out"], [f, a] + [named[k] for k in keys], grad_outputs=gout)))
        torch.cuda.synchronize()
        return [t.detach().clone() for t in box["out"]], [t.clone() for t in box["g"]], cf, cb
    finally:
        m.fused_chain_grad, m.chain_grad_compute = False, "fp32"


def test_the_backward_follows_the_forward_not_the_attribute(models):
    A, B, T = 6, 17, 3
    m = models(A)
    args = _inputs(B, T, A)
    for mode, other in (("bf16", "fp32"), ("fp32", "bf16")):
        want, flipped = _model_run(m, *args, mode), _model_run(m, *args, mode, flip=other)
        for i, (a, b) in enumerate(zip(want[0] + want[1], flipped[0] + flipped[1])):
            _same(a, b, (mode, i))
        assert want[3] == flipped[3] and (G.BWD in want[3]) == (mode == "bf16")
    m.fused_chain_grad, m.chain_grad_compute = True, "fp16"
    try:
        with pytest.raises(ValueError, match="chain_grad_compute"):
            m.sample_posterior(args[0].clone().requires_grad_(True), args[1], args[2])
        m.fused_chain_grad = False                               # read only where the fused form under grad is about to run
        m.sample_posterior(args[0].clone().requires_grad_(True), args[1], args[2])
        with torch.no_grad():
            m.sample_posterior(args[0], args[1], args[2])
    finally:
        m.fused_chain_grad, m.chain_grad_compute = False, "fp32"


# ---- 6. nothing else is written --------------------------------------------------------------------------------------------------------------
def _v3(t, B, T):
    return t.as_strided((B, T, t.shape[1]), (T * t.stride(0), t.stride(0), 1))


@pytest.mark.parametrize("layout", ["aligned", "odd"])
def test_only_the_declared_outputs_are_written(models, layout):
    from s2p_amd import ops
    A, B, T, X = 6, 17, 3, 3                                 # X: rows past B in every state and gradient buffer
    S = T - 1
    m = models(A)
    feat, action, noise, gout = _inputs(B, T, A)
    want = _direct(m, feat, action, noise, gout)
    pk = want["pk"]
    odd = layout == "odd"
    eps = Region(B * T, Z, pitch=Z + (13 if odd else 12), off=7 if odd else 8, fill=noise.reshape(B * T, Z))
    mean = Region(B * T, Z1, pitch=37 if odd else 40, off=3 if odd else 4)
    std = Region(B * T, Z1, pitch=33 if odd else 36, off=1 if odd else 0)
    z = Region(B * T, Z, pitch=Z + (31 if odd else 32), off=9 if odd else 16)
    dense = lambda rows, w: Region(rows + X, w, pitch=w, off=0)
    widths = (HID, HID, 64, HID, HID, 512)
    st0 = [dense(B, w) for w in widths]
    stc = [dense(S * B, w) for w in widths + (Z,)]
    state = ops.chain_state([r.v[:B] for r in st0[:3]], [r.v[:B] for r in st0[3:]], [r.v[:S * B].view(S, B, -1) for r in stc])
    ins = [feat, want["ra"], want["rb"], eps.buf] + [p.detach() for p in m._chain_params()] + [t for p in pk for t in p.values()]
    ins0 = [t.clone() for t in ins]
    ops.posterior_chain_fwd_save_bf16(feat[:, 0], want["ra"], want["rb"], _v3(eps.v, B, T), [ops.chain_mlp_bf16(p) for p in pk],
                                      _v3(mean.v, B, T), _v3(std.v, B, T), _v3(z.v, B, T), state)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(ins, ins0))
    for name, r in (("mean", mean), ("std", std), ("z", z)):
        _same(r.bits(name).view(want[name].shape), want[name].cpu(), (layout, name))
    for name, r, rows in zip(STATE, st0 + stc, [B] * 6 + [S * B] * 7):
        got = r.bits(name)
        _same(got[:rows].view(want[name].shape), want[name].cpu(), (layout, name))
        assert bool((got[rows:] == SENT).all()), (layout, name, "rows >= B")
    dz = Region(B * T, Z, pitch=Z + (21 if odd else 20), off=11 if odd else 12, fill=want["dz"].reshape(B * T, Z))
    dmean = Region(B * T, Z1, pitch=45 if odd else 44, off=9 if odd else 8, fill=want["dmean"].reshape(B * T, Z1))
    dstd = Region(B * T, Z1, pitch=33 if odd else 36, off=1 if odd else 4, fill=want["dstd"].reshape(B * T, Z1))
    outs = [dense(S * B, w) for w in (64, HID, HID, 512, HID, HID, Z)]
    bufs = [r.buf for r in st0 + stc] + [dz.buf, dmean.buf, dstd.buf, eps.buf]
    bufs0 = [t.clone() for t in bufs]
    ops.posterior_chain_bwd_bf16(_v3(eps.v, B, T), _v3(dmean.v, B, T), _v3(dstd.v, B, T), _v3(dz.v, B, T),
                                 [ops.chain_mlp_bwd_bf16(pk[2]), ops.chain_mlp_bwd_bf16(pk[3])], state, [r.v[:S * B].view(S, B, -1) for r in outs])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs, bufs0)) and all(torch.equal(a, b) for a, b in zip(ins, ins0))
    for name, r in zip(GRADS, outs):
        got = r.bits(name)
        _same(got[:S * B].view(want[name].shape), want[name].cpu(), (layout, name))
        assert bool((got[S * B:] == SENT).all()), (layout, name, "rows >= B")


# ---- 7. the pack launch ------------------------------------------------------------------------------------------------------------------------
SB = 0x5a5a                                              # the bit pattern of the pads around a pack


def _pack_check(src, what):
    """One job on a [rows, cols] fp32 view: dst and dst_t inside wider bf16 buffers of a sentinel bit pattern, against torch's cast."""
    from s2p_amd import ops
    rows, cols = src.shape
    dst, dst_t = (torch.full((r + 2, c + 8), SB, dtype=torch.int16, device="cuda").view(torch.bfloat16) for r, c in ((rows, cols), (cols, rows)))
    src0 = src.clone().contiguous()
    ops.chain_pack_bf16([(src, dst[:rows, :cols], dst_t[:cols, :rows])])
    ops.chain_pack_bf16([(src[:0], dst[:0, :cols], None), (src[:, :0], None, dst_t[:0, :rows])])      # empty shapes: no-ops
    torch.cuda.synchronize()
    want = src0.to(torch.bfloat16)
    bits = lambda t: t.contiguous().view(torch.int16)
    nan = torch.isnan(src0)
    for name, got, w, n in (("dst", dst[:rows, :cols], want, nan), ("dst_t", dst_t[:cols, :rows], want.t(), nan.t())):
        ok = bits(got) == bits(w)
        assert bool((ok | n).all()), (what, name, int((~ok).sum()))
        assert bool(torch.isnan(got.float())[n].all()), (what, name, "NaN stays NaN")
    for name, buf, r, c in (("dst", dst, rows, cols), ("dst_t", dst_t, cols, rows)):
        pad = bits(buf).clone()
        pad[:r, :c] = SB
        assert bool((pad == SB).all()), (what, name, "a pad was written")
    assert torch.equal(src.contiguous().view(torch.int32), src0.view(torch.int32)), (what, "src")


def test_pack_is_bitwise_the_cast_and_the_transpose(hip_device):
    g = torch.Generator().manual_seed(12)
    wide = torch.randn(256, 296, generator=g).cuda()
    _pack_check(wide[:, 8:296], "256 x 288 out of pitch 296")                     # a column-offset source with a pitch
    _pack_check(torch.randn(64, 256, generator=g).cuda(), "64 x 256")
    _pack_check(torch.randn(1, 8, generator=g).cuda(), "1 x 8")
    _pack_check(torch.randn(3, 5, generator=g).cuda() * 1e-3, "3 x 5")
    # exact ties of both parities, the largest finite value, subnormals, +-0, +-inf, NaN
    special = [0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x3f807fff, 0x3f808001, 0x7f7fffff, 0xff7fffff, 0x7f7f8000, 0x7f7f7fff,
               0x00000001, 0x00008000, 0x00018000, 0x807fffff, 0x00800000, 0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000,
               0xffc00001, 0x7f800001, 0x3f800000, 0x0000ffff]
    src = torch.from_numpy(np.array(special + special[::-1][:8], dtype=np.uint32).view(np.float32)).reshape(4, 8).cuda()
    _pack_check(src, "special values")
    _pack_check(src.t().contiguous(), "special values, 8 x 4")


def test_packed_bf16_grad_is_one_launch_and_the_packs_of_packed_bf16(hip_device):
    m = build_model(6)
    for h in HEADS:
        g = getattr(m, h)
        g.packed()
        calls = count_calls(lambda: g.packed_bf16_grad())
        torch.cuda.synchronize()
        assert calls == {"s2p_chain_pack_bf16": 1}, (h, calls)
        assert count_calls(lambda: g.packed_bf16_grad()) == {}                   # warm: the (data_ptr, _version) key rule
        a, b = g.packed_bf16_grad(), g.packed_bf16()
        for k in ("w1", "w2", "w3"):
            _same(a[k].view(torch.int16), b[k].view(torch.int16), (h, k))
            _same(a[k + "t"].view(torch.int16), b[k].t().contiguous().view(torch.int16), (h, k + "t"))
            assert a["b" + k[1]] is g.packed()["b" + k[1]]
        with torch.no_grad():
            g.net._modules["2"].weight.mul_(1.5)
        c = g.packed_bf16_grad()
        assert c is not a and torch.equal(c["w2"], g.net._modules["2"].weight.detach().to(torch.bfloat16)) and not torch.equal(c["w2"], a["w2"])


# ---- 8. off by default -----------------------------------------------------------------------------------------------------------------------
def test_off_by_default_and_the_same_calls_with_the_suffix(hip_device):
    A, B, T = 6, 17, 9
    m = build_model(A)                                       # a model whose switches no test has touched
    assert m.chain_grad_compute == "fp32"
    args = _inputs(B, T, A)
    m.fused_chain_grad = True
    try:
        f, a = args[0].clone().requires_grad_(True), args[1].clone().requires_grad_(True)
        box = {}
        cf = count_calls(lambda: box.setdefault("out", m.sample_posterior(f, a, args[2])))
        named = dict(m.named_parameters())
        cb = count_calls(lambda: box.setdefault("g", torch.autograd.grad(box["out"], [f, a] + [named[k] for k in G.param_keys()], grad_outputs=args[3])))
        torch.cuda.synchronize()
    finally:
        m.fused_chain_grad = False
    never = (box["out"], box["g"], cf, cb)                   # the attribute never set
    fp32 = _model_run(m, *args, "fp32")
    assert never[2] == fp32[2] and never[3] == fp32[3]
    for i, (x, y) in enumerate(zip(list(never[0]) + list(never[1]), fp32[0] + fp32[1])):
        _same(x.detach(), y, ("fp32", i))
    assert all("bf16" not in k for c in fp32[2:] for k in c)
    assert fp32[2].get("s2p_posterior_chain_fwd_save") == 1 and fp32[3].get("s2p_posterior_chain_bwd") == 1
    _model_run(m, *args, "bf16")                             # warms the packs
    bf = _model_run(m, *args, "bf16")
    strip = lambda c: {k[:-5] if k in (G.FWD, G.BWD) else k: v for k, v in c.items()}
    print("library calls, forward: fp32", fp32[2], " bf16", bf[2])
    print("library calls, backward: fp32", fp32[3], " bf16", bf[3])
    assert strip(bf[2]) == fp32[2] and strip(bf[3]) == fp32[3]
    assert bf[2].get(G.FWD) == 1 and bf[3].get(G.BWD) == 1 and G.PACK not in bf[2] and G.PACK not in bf[3]
    assert not torch.equal(bf[0][2], fp32[0][2])             # the mode multiplies other operands: not the same numbers


# ---- 9. the keyword -----------------------------------------------------------------------------------------------------------------------------
def test_slac_algorithm_keyword_sets_the_mode_and_update_latent_trains_in_it(hip_device):
    import slac_buffer_ref as SB
    from s2p_amd.slac_algo import SlacAlgorithm

    def make(**kw):
        a = SlacAlgorithm((3, 100, 100), (SB.A,), 1, hip_device, seed=0, batch_size_latent=2, buffer_size=32, num_sequences=SB.S,
                          frame_capacity=128, fused_chain_grad=True, **kw)
        a.latent.load_state_dict(R.full_state_dict(R.make_params(SB.A)), strict=True)
        a.load_data_in_buffer(SB.real_dataset(2, 12, 100, 100), **dict(SB.LOAD_ARGS["real"], data_num=24))
        return a
    assert make().latent.chain_grad_compute == "fp32"
    a = make(chain_grad_compute="bf16")
    assert a.latent.chain_grad_compute == "bf16" and a.latent.fused_chain_grad is True and a.latent.chain_compute == "fp32"
    start = {k: v.detach().clone() for k, v in a.latent.named_parameters()}
    np.random.seed(5)
    torch.manual_seed(5)
    calls = count_calls(lambda: [a.update_latent() for _ in range(2)])
    torch.cuda.synchronize()
    print("library calls of two update_latent steps:", {k: v for k, v in calls.items() if "chain" in k})
    assert calls.get(G.FWD) == 2 and calls.get(G.BWD) == 2 and calls.get(G.PACK) == 8          # the parameters change: four heads a step
    assert "s2p_posterior_chain_fwd_save" not in calls and "s2p_posterior_chain_bwd" not in calls
    for k, v in a.latent.named_parameters():
        assert bool(torch.isfinite(v).all()) and not torch.equal(v, start[k]), k
    a.latent.chain_grad_compute = "fp16"
    with pytest.raises(ValueError, match="chain_grad_compute"):
        a.update_latent()
