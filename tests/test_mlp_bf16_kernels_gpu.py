"""N3l -- the s2p_mlp_linear_*_bf16 entry points (csrc/mlp.hip over csrc/ens_tile_bf16.h) through the C ABI, at the edges of the tiles:
rows 1 / 31 / 33 / 70, N 20 / 36 / 68 / 128, K 4 / 12 / 20 / 36 / 296 (less than one step of 16, a partial last step, the production
first layer), x_pitch > K, three groups of unequal rows and K with one empty, ReLU and none, the row split at S = 1, 2, 3.

1. EXACT data: integer operands in [-4, 4] are exact in bf16 and every sum stays below 2^24, so every output of every _bf16 entry
   equals the fp32 entry's BITWISE -- any indexing, masking or tail error shows with no tolerance in play.
2. Random data against the fp64 restatement of tests/mlp_bf16_ref.py, per element:
   |got - ref| <= (K_sum + 2) 2^-23 (sum |a^ b^| + |bias|), K_sum = K (forward), rows (dw), N (dprev); a NaN counts as outside.  db is
   an fp32 sum of the unrounded values: the fp32 kernel's rule, K_TOL x max(ref32_err, 1e-6) with K_TOL = 4.  Worst ratios are printed.
3. Two identical calls are bitwise equal; the split at S = 1 is _bwd_bf16; _dgrad_bf16 is the dprev of _bwd_bf16.
4. Refusals through s2p_last_error."""
import pytest
import torch

import mlp_bf16_ref as M

pytestmark = pytest.mark.gpu
K_TOL, FLOOR, CANARY = 4.0, 1e-6, 7.0
WORST = {}


def _L():
    from s2p_amd import _lib
    return _lib


def _ptr(t):
    return None if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


class Layer:
    """One group's operands on the host and the device: x [rows][xp >= K], w [N][K], bias [N], dpre [rows][dp >= N], pre_prev
    [rows][pp >= K].  `exact`: integers in [-4, 4], else standard normal."""

    def __init__(self, rows, K, N, dev, g, exact, extra=4):
        def draw(*shape):
            return torch.randint(-4, 5, shape, generator=g).float() if exact else torch.randn(*shape, generator=g)

        self.rows, self.K, self.N, self.xp, self.dp, self.pp = rows, K, N, K + extra, N + extra, K + extra
        self.x, self.w, self.b, self.d, self.pre_prev = draw(rows, K), draw(N, K), draw(N), draw(rows, N), draw(rows, K)
        pad = lambda t, p: torch.cat([t, torch.full((t.shape[0], p - t.shape[1]), 3.0)], 1).contiguous().to(dev)   # noqa: E731
        self.xd, self.dd, self.ppd = pad(self.x, self.xp), pad(self.d, self.dp), pad(self.pre_prev, self.pp)
        self.wd, self.bd = self.w.to(dev), self.b.to(dev)


def run_fwd(layers, relu, bf16, dev):
    L = _L()
    N = layers[0].N
    outs = [(torch.full((l.rows, N + 4), CANARY, device=dev), torch.full((l.rows, N + 4), CANARY, device=dev)) for l in layers]
    arr = (L.MlpFwdGroup * len(layers))(*[L.MlpFwdGroup(_ptr(l.xd), _ptr(l.wd), _ptr(l.bd), _ptr(pre), _ptr(act), l.xp, N + 4, l.rows, l.K)
                                          for l, (pre, act) in zip(layers, outs)])
    name = "s2p_mlp_linear_fwd" + ("_bf16" if bf16 else "")
    L.check(getattr(L.lib(), name)(arr, len(layers), N, L.ACT_RELU if relu else L.ACT_NONE, _st()), name)
    torch.cuda.synchronize()
    return outs


def run_bwd(layers, relu, bf16, dev, kind="bwd", S=1):
    """kind: bwd, dgrad (dw / db NULL-free canaries must stay) or bwd_split.  -> [(dw, db, dprev)] per group."""
    L = _L()
    N = layers[0].N
    outs = [(torch.full((N, l.K), CANARY, device=dev), torch.full((N,), CANARY, device=dev), torch.full((l.rows, l.pp), CANARY, device=dev))
            for l in layers]
    arr = (L.MlpBwdGroup * len(layers))(*[
        L.MlpBwdGroup(None if kind == "dgrad" else _ptr(l.xd), _ptr(l.dd), _ptr(l.wd), _ptr(dw), _ptr(db), _ptr(l.ppd) if relu else None,
                      _ptr(dp), l.xp, l.dp, l.pp, l.rows, l.K) for l, (dw, db, dp) in zip(layers, outs)])
    name, act = "s2p_mlp_linear_" + kind + ("_bf16" if bf16 else ""), L.ACT_RELU if relu else L.ACT_NONE
    if kind == "bwd_split":
        need = L.lib().s2p_mlp_linear_bwd_split_workspace(arr, len(layers), N, S)
        ws = torch.full((need // 4 + 8,), float("nan"), device=dev)
        L.check(getattr(L.lib(), name)(arr, len(layers), N, act, S, _ptr(ws), need, _st()), name)
        torch.cuda.synchronize()
        assert bool(torch.isnan(ws[need // 4:]).all())                               # nothing written past the stated size
    else:
        L.check(getattr(L.lib(), name)(arr, len(layers), N, act, _st()), name)
        torch.cuda.synchronize()
    return outs


def _same(a, b):
    return all(torch.equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))


# ---- 1. exact data: bitwise the fp32 entry points -------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("N", M.WIDTHS)
def test_exact_data_is_bitwise_the_fp32_entry(hip_device, N, relu):
    g = torch.Generator().manual_seed(N + relu)
    cases = [[Layer(rows, K, N, hip_device, g, True)] for rows in M.ROWS for K in M.DEPTHS]
    cases.append([Layer(rows, K, N, hip_device, g, True, extra=0 if i else 8) for i, (rows, K) in enumerate(M.GROUPED)])
    for layers in cases:
        tag = [(l.rows, l.K) for l in layers]
        assert _same(run_fwd(layers, relu, True, hip_device), run_fwd(layers, relu, False, hip_device)), ("fwd", N, tag)
        want = run_bwd(layers, relu, False, hip_device)
        assert _same(run_bwd(layers, relu, True, hip_device), want), ("bwd", N, tag)
        got = run_bwd(layers, relu, True, hip_device, "dgrad")
        assert all(torch.equal(a[2], b[2]) for a, b in zip(got, want)), ("dgrad", N, tag)
        assert all(bool((a[0] == CANARY).all()) and bool((a[1] == CANARY).all()) for a in got)          # dw / db are not touched
        for S in M.SPLITS if layers[0].rows == 70 else (1,):
            assert _same(run_bwd(layers, relu, True, hip_device, "bwd_split", S), want), ("bwd_split", S, N, tag)
    l = cases[0][0]
    pre, act = run_fwd([l], relu, True, hip_device)[0]                                # (and the data is not trivially zero)
    assert float(pre[:, :N].abs().max()) > 0 and bool((pre[:, N:] == CANARY).all()) and bool((act[:, N:] == CANARY).all())


# ---- 2. random data against the fp64 restatement, per element ---------------------------------------------------------------------------
def _ratio(what, got, ref, k_sum, mag, tag):
    r = M.worst_ratio(got, ref, k_sum, mag)
    WORST[what] = max(WORST.get(what, 0.0), r)
    assert r <= 1.0, (what, tag, r)


def _db(got, d, tag):
    b64, b32 = d.double().sum(0), d.sum(0).double()
    err, ref = float((got.cpu().double() - b64).abs().max() / b64.abs().max()), max(float((b32 - b64).abs().max() / b64.abs().max()), FLOOR)
    WORST["db (x ref32_err)"] = max(WORST.get("db (x ref32_err)", 0.0), err / ref)
    assert err <= K_TOL * ref, ("db", tag, err, K_TOL * ref)


def _check_layer(l, relu, pre_act, bwd, tag):
    pre, act = pre_act
    dw, db, dprev = bwd
    p64, pmag = M.fwd(l.x, l.w, l.b)
    _ratio("pre", pre[:, :l.N], p64, l.K, pmag, tag)
    want_act = torch.relu(pre[:, :l.N]) if relu else pre[:, :l.N]
    assert torch.equal(act[:, :l.N], want_act), ("act", tag)                          # the activation of the stored pre, bit for bit
    w64, wmag, _ = M.wgrad(l.d, l.x)
    _ratio("dw", dw, w64, l.rows, wmag, tag)
    _db(db, l.d, tag)
    d64, dmag = M.dgrad(l.d, l.w, l.pre_prev if relu else None)
    _ratio("dprev", dprev[:, :l.K], d64, l.N, dmag, tag)
    assert bool((pre[:, l.N:] == CANARY).all()) and bool((dprev[:, l.K:] == CANARY).all())            # nothing past a row's end


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("N", M.WIDTHS)
def test_random_data_within_the_accumulation_bound(hip_device, N, relu):
    g = torch.Generator().manual_seed(100 + N + relu)
    cases = [[Layer(rows, K, N, hip_device, g, False)] for rows in M.ROWS for K in M.DEPTHS]
    cases.append([Layer(rows, K, N, hip_device, g, False, extra=0 if i else 8) for i, (rows, K) in enumerate(M.GROUPED)])
    for layers in cases:
        fw, bw = run_fwd(layers, relu, True, hip_device), run_bwd(layers, relu, True, hip_device)
        for l, pa, b in zip(layers, fw, bw):
            if l.rows == 0:
                assert all(bool((t == CANARY).all()) for t in pa + b)                 # an empty group writes nothing
                continue
            _check_layer(l, relu, pa, b, (l.rows, N, l.K))
        # 3. the identities
        assert _same(run_fwd(layers, relu, True, hip_device), fw) and _same(run_bwd(layers, relu, True, hip_device), bw)
        assert _same(run_bwd(layers, relu, True, hip_device, "bwd_split", 1), bw)
        dg = run_bwd(layers, relu, True, hip_device, "dgrad")
        assert all(torch.equal(a[2], b[2]) for a, b in zip(dg, bw)) and _same(run_bwd(layers, relu, True, hip_device, "dgrad"), dg)
        if layers[0].rows == 70:
            for S in M.SPLITS[1:]:
                sp = run_bwd(layers, relu, True, hip_device, "bwd_split", S)
                assert _same(run_bwd(layers, relu, True, hip_device, "bwd_split", S), sp)
                for l, (dw, db, dprev), b in zip(layers, sp, bw):
                    if l.rows == 0:
                        continue
                    assert torch.equal(dprev, b[2])                                   # the input tiles are those of _bwd_bf16
                    w64, wmag, _ = M.wgrad(l.d, l.x)
                    _ratio("dw split", dw, w64, l.rows, wmag, (S, l.rows, N, l.K))
                    _db(db, l.d, (S, l.rows, N, l.K))
    print("worst |got - ref| / bound at N %d relu %d: %s" % (N, relu, {k: "%.3f" % v for k, v in WORST.items()}))


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_no_ops(hip_device):
    L, g = _L(), torch.Generator().manual_seed(5)
    l = Layer(33, 36, 36, hip_device, g, False)
    pre, dw, db, dp = (torch.full(s, CANARY, device=hip_device) for s in ((33, 40), (36, 36), (36,), (33, l.pp)))
    ws = torch.empty(4 * (36 * 36 + 36), device=hip_device)
    FW = ("x", "w", "bias", "pre", "act", "x_pitch", "y_pitch", "rows", "K")
    BW = ("x", "dpre", "w", "dw", "db", "pre_prev", "dprev", "x_pitch", "dpre_pitch", "prev_pitch", "rows", "K")

    def fgroup(**kw):
        f = dict(x=_ptr(l.xd), w=_ptr(l.wd), bias=_ptr(l.bd), pre=_ptr(pre), act=None, x_pitch=l.xp, y_pitch=40, rows=33, K=36)
        f.update(kw)
        return L.MlpFwdGroup(*[f[k] for k in FW])

    def bgroup(**kw):
        f = dict(x=_ptr(l.xd), dpre=_ptr(l.dd), w=_ptr(l.wd), dw=_ptr(dw), db=_ptr(db), pre_prev=_ptr(l.ppd), dprev=_ptr(dp), x_pitch=l.xp,
                 dpre_pitch=l.dp, prev_pitch=l.pp, rows=33, K=36)
        f.update(kw)
        return L.MlpBwdGroup(*[f[k] for k in BW])

    def rc(kind, gs, N=36, G=None, act=L.ACT_RELU):
        arr = ((L.MlpFwdGroup if kind == "fwd" else L.MlpBwdGroup) * len(gs))(*gs) if gs is not None else None
        n = (len(gs) if gs is not None else 1) if G is None else G
        tail = (2, _ptr(ws), ws.numel() * 4, _st()) if kind == "bwd_split" else (_st(),)
        return getattr(L.lib(), "s2p_mlp_linear_%s_bf16" % kind)(arr, n, N, act, *tail)

    def refused(code, what):
        assert code != 0, what
        msg = L.lib().s2p_last_error().decode()
        assert msg.startswith("s2p_mlp_linear_") and "_bf16" in msg.split(":")[0], (what, msg)
        return msg

    assert rc("fwd", [fgroup()]) == 0
    for kind in ("bwd", "dgrad", "bwd_split"):
        assert rc(kind, [bgroup()]) == 0
    bad_fwd = dict(negative_rows=fgroup(rows=-1), negative_K=fgroup(K=-4), null_x=fgroup(x=None), null_w=fgroup(w=None), null_bias=fgroup(bias=None),
                   no_output=fgroup(pre=None), short_x_pitch=fgroup(x_pitch=32), short_y_pitch=fgroup(y_pitch=32),
                   misaligned_x=fgroup(x=_ptr(l.xd) + 4), misaligned_w=fgroup(w=_ptr(l.wd) + 4), K_not_4=fgroup(K=34))
    for what, grp in bad_fwd.items():
        refused(rc("fwd", [grp]), "fwd " + what)
    bad_bwd = dict(negative_rows=bgroup(rows=-1), negative_K=bgroup(K=-4), null_dpre=bgroup(dpre=None), null_w=bgroup(w=None),
                   null_pre_prev=bgroup(pre_prev=None), short_dpre_pitch=bgroup(dpre_pitch=32), short_prev_pitch=bgroup(prev_pitch=32),
                   misaligned_dpre=bgroup(dpre=_ptr(l.dd) + 4), dpre_pitch_not_4=bgroup(dpre_pitch=l.dp + 1))
    weights_only = dict(null_x=bgroup(x=None), null_dw=bgroup(dw=None), null_db=bgroup(db=None), short_x_pitch=bgroup(x_pitch=32))
    for kind in ("bwd", "dgrad", "bwd_split"):
        for what, grp in dict(bad_bwd, **({} if kind == "dgrad" else weights_only)).items():
            refused(rc(kind, [grp]), kind + " " + what)
        refused(rc(kind, [bgroup(dprev=None)]), kind + " null dprev") if kind == "dgrad" else None
    for kind in ("fwd", "bwd", "dgrad", "bwd_split"):
        one = [fgroup()] if kind == "fwd" else [bgroup()]
        assert "N" in refused(rc(kind, one, N=16), kind + " N = 16") and refused(rc(kind, one, N=4), kind + " N = 4")
        refused(rc(kind, one, N=-1), kind + " negative N")
        refused(rc(kind, one, G=-1), kind + " negative G")
        refused(rc(kind, None), kind + " null table")
        refused(rc(kind, one, act=3), kind + " activation")
        refused(rc(kind, one * 9), kind + " nine groups")
        assert rc(kind, one, G=0) == 0 and rc(kind, one, N=0) == 0 and rc(kind, None, G=0) == 0        # a size of 0: no pointer looked at
        empty = fgroup(rows=0, x=None, w=None, bias=None, pre=None) if kind == "fwd" else bgroup(rows=0, x=None, dpre=None, w=None, dw=None, db=None, dprev=None)
        assert rc(kind, [empty] + one) == 0 and rc(kind, [empty]) == 0
    refused(rc("bwd", [bgroup()], N=38), "N not a multiple of 4")
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in (pre, dw, db, dp))
