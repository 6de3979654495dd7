"""Kernel-level parity of csrc/linear_small.hip (s2p_linear_fwd / s2p_linear_bwd, the state path's and the SLAC latent model's small
fp32 layers) through the C ABI against float64 torch on the CPU: every activation the header names, bias == NULL, n_store above N,
db == NULL, dx == NULL, dw_row > k_real, accumulation onto existing gradients, the split-K input gradient on both sides of its
N = 2048 threshold with a short last split, its workspace refusals, unknown activation ids, and bitwise repeatability.  Every tensor is
a pitched, column-offset view inside a sentinel-filled buffer (guard_region.Region): no byte outside a declared view may change.

Tolerance: the project's rule (tests/test_ensemble_train_gpu.py, tests/test_iql_kernels_gpu.py) -- per quantity
K_TOL x max(ref32_err, 1e-6), K_TOL = 4, ref32_err being the deviation of the SAME formula run in fp32 torch on the CPU from its fp64
run, both relative to the fp64 maximum: the kernels are that fp32 arithmetic in another summation order (MFMA k-chunks; split-K
partials added in split order).  Worst observed ratios: DESIGN.md section 6b.8 (printed by test_zz_report_worst_ratios)."""
import pytest
import torch
import torch.nn.functional as F

from ensemble_train_ref import rel_max
from guard_region import BAND, SENT, Region

pytestmark = pytest.mark.gpu
K_TOL, FLOOR = 4.0, 1e-6
SLOPE = 0.2
WORST = {}


def _check(group, got, f64, f32, what=""):
    err, ref = rel_max(got, f64), max(rel_max(f32, f64), FLOOR)
    WORST[group] = max(WORST.get(group, 0.0), err / ref)
    print("%-18s %-44s err %.3e  ref32_err %.3e  ratio %.3f" % (group, what, err, ref, err / ref))
    assert err <= K_TOL * ref, (group, what, err, K_TOL * ref)


def _L():
    from s2p_amd import _lib
    return _lib


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(r):
    return None if r is None else r.ptr


def _act(pre, act):
    L = _L()
    if act == L.ACT_RELU:
        return torch.relu(pre)
    if act == L.ACT_LRELU:
        return F.leaky_relu(pre, SLOPE)
    if act == L.ACT_TANH:
        return torch.tanh(pre)
    if act == L.ACT_SWISH:
        return pre * torch.sigmoid(pre)
    return pre


# ---- forward ---------------------------------------------------------------------------------------------------------------------------
def fwd_call(x_r, w_r, b_r, M, K, N, act, y_r, n_store, slope=SLOPE):
    return _L().lib().s2p_linear_fwd(x_r.ptr, M, K, x_r.pitch, w_r.ptr, w_r.pitch, _p(b_r), N, act, slope, y_r.ptr, y_r.pitch, n_store, _st())


@pytest.mark.parametrize("M", [1, 17, 65])
@pytest.mark.parametrize("K,N,n_store", [(4, 1, 4), (132, 20, 24), (260, 72, 72)])
def test_forward_every_activation_with_and_without_bias(hip_device, M, K, N, n_store):
    """K = 132 crosses the 128-wide unrolled k step by one float4, N = 20 leaves a 4-column tail in the second 16-wide tile, M = 65
    one row in a second 64-row block.  One weight row and its bias are exactly zero: an exact zero passes through every activation."""
    L = _L()
    g = torch.Generator().manual_seed(1000 * M + K)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5 * 1.5
    b = torch.randn(N, generator=g)
    zr = 1 if N > 1 else None
    if zr is not None:
        w[zr] = 0
        b[zr] = 0
    x_r, w_r, b_r = Region(M, K, pitch=K + 8, off=4, fill=x), Region(N, K, pitch=K + 8, off=4, fill=w), Region(1, N, off=1, fill=b[None])
    for act in (L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU, L.ACT_TANH, L.ACT_SWISH):
        for bias in (True, False):
            y_r = Region(M, n_store, pitch=n_store + 8, off=4)
            L.check(fwd_call(x_r, w_r, b_r if bias else None, M, K, N, act, y_r, n_store), "s2p_linear_fwd")
            y = y_r.get("y act %d" % act)
            ref = {}
            for dt in (torch.float64, torch.float32):
                ref[dt] = _act(F.linear(x.to(dt), w.to(dt), b.to(dt) if bias else None), act)
            _check("forward act %d" % act, y[:, :N], ref[torch.float64], ref[torch.float32], "M %d K %d N %d bias %d" % (M, K, N, bias))
            assert bool((y[:, N:] == 0).all())                                  # the padding columns [N, n_store) are exactly zero
            assert zr is None or bool((y[:, zr] == 0).all())                    # the planted zero row: act(0) = 0 exactly
            y2 = Region(M, n_store, pitch=n_store + 8, off=4)
            L.check(fwd_call(x_r, w_r, b_r if bias else None, M, K, N, act, y2, n_store), "s2p_linear_fwd")
            assert torch.equal(y2.bits(), y_r.bits())                           # two identical calls: equal bits
    for r in (x_r, w_r, b_r):
        r.get("an input was written")


def test_forward_refuses_unknown_activations_and_an_empty_batch_is_a_no_op(hip_device):
    L = _L()
    lib = L.lib()
    M, K, N = 5, 8, 4
    x_r, w_r, b_r = Region(M, K, off=4, fill=torch.ones(M, K)), Region(N, K, off=4, fill=torch.ones(N, K)), Region(1, N, fill=torch.ones(1, N))
    y_r = Region(M, N, off=4)
    for act in (5, -1):
        assert fwd_call(x_r, w_r, b_r, M, K, N, act, y_r, N) != 0 and lib.s2p_last_error(), act
        assert y_r.untouched(), act
    for bad in (dict(M=-1), dict(K=6), dict(N=0), dict(n_store=N - 1)):
        a = dict(M=M, K=K, N=N, n_store=N)
        a.update(bad)
        assert lib.s2p_linear_fwd(x_r.ptr, a["M"], a["K"], x_r.pitch, w_r.ptr, w_r.pitch, b_r.ptr, a["N"], L.ACT_NONE, SLOPE, y_r.ptr, y_r.pitch,
                                  a["n_store"], _st()) != 0 and lib.s2p_last_error(), bad
        assert y_r.untouched(), bad
    assert lib.s2p_linear_fwd(x_r.ptr, M, K, x_r.pitch, None, w_r.pitch, b_r.ptr, N, L.ACT_NONE, SLOPE, y_r.ptr, y_r.pitch, N, _st()) != 0
    assert y_r.untouched()
    # M == 0: a successful no-op that looks at no pointer
    assert lib.s2p_linear_fwd(None, 0, K, 8, None, 8, None, N, L.ACT_NONE, SLOPE, None, 8, N, _st()) == 0
    assert lib.s2p_linear_bwd(None, 8, None, 4, None, 4, 0, K, K, N, None, 4, L.ACT_NONE, SLOPE, None, 8, None, None, 8, None, 0, _st()) == 0
    assert fwd_call(x_r, w_r, b_r, M, K, N, L.ACT_SWISH, y_r, N) == 0          # and the same arguments with a known id are accepted
    want = torch.full((M, N), float(K + 1), dtype=torch.float64)
    assert rel_max(y_r.get(), want * torch.sigmoid(want)) < 1e-6


# ---- backward --------------------------------------------------------------------------------------------------------------------------
class BwdCase:
    """Host data and guarded device views of one s2p_linear_bwd problem.  x's columns [k_real, K) and w_bwd's rows [k_real, K) are the
    zero padding a caller has there; y (the saved OUTPUT) holds planted exact zeros; dw / db start from random content."""

    def __init__(self, M, k_real, K, N, seed, wide_dx=True):
        g = torch.Generator().manual_seed(seed)
        self.M, self.k_real, self.K, self.N = M, k_real, K, N
        self.x = torch.zeros(M, K)
        self.x[:, :k_real] = torch.randn(M, k_real, generator=g)
        self.w = torch.zeros(N, K)
        self.w[:, :k_real] = torch.randn(N, k_real, generator=g) / N ** 0.5
        self.dy = torch.randn(M, N, generator=g)
        self.y = torch.randn(M, N, generator=g)
        self.y[0, ::3] = 0
        self.y[M - 1, N - 1] = 0
        self.y[:, 1] = 0
        self.dw0, self.db0 = torch.randn(N, k_real, generator=g), torch.randn(N, generator=g)
        self.x_r = Region(M, K, pitch=K + 8, off=4, fill=self.x)
        self.dy_r = Region(M, N, pitch=N + 8, off=4, fill=self.dy)
        self.y_r = Region(M, N, pitch=N + 12, off=8, fill=self.y)
        self.wb_r = Region(K, N, pitch=N + 8, off=4, fill=self.w.t())
        self.dx_geom = dict(pitch=K + 8, off=4) if wide_dx else dict(pitch=K, off=0)

    def outputs(self, db=True, dx=True):
        dw_r = Region(self.N, self.k_real, pitch=self.k_real + 5, off=2, fill=self.dw0)         # dw_row > k_real
        db_r = Region(1, self.N, off=1, fill=self.db0[None]) if db else None
        dx_r = Region(self.M, self.K, **self.dx_geom) if dx else None
        return dw_r, db_r, dx_r

    def call(self, act, dw_r, db_r, dx_r, ws=None, ws_bytes=0, with_w=True):
        return _L().lib().s2p_linear_bwd(self.x_r.ptr, self.x_r.pitch, self.dy_r.ptr, self.dy_r.pitch, self.y_r.ptr, self.y_r.pitch, self.M, self.K,
                                         self.k_real, self.N, self.wb_r.ptr if with_w else None, self.wb_r.pitch, act, SLOPE, dw_r.ptr, dw_r.pitch,
                                         _p(db_r), _p(dx_r), dx_r.pitch if dx_r is not None else 0, ws, ws_bytes, _st())

    def ref(self, act, dt):
        L = _L()
        dy, y = self.dy.to(dt), self.y.to(dt)
        if act == L.ACT_LRELU:
            dpre = dy * torch.where(y > 0, 1.0, SLOPE).to(dt)
        elif act == L.ACT_RELU:
            dpre = dy * torch.where(y > 0, 1.0, 0.0).to(dt)
        else:
            dpre = dy
        return (self.dw0.to(dt) + dpre.t() @ self.x[:, :self.k_real].to(dt), self.db0.to(dt) + dpre.sum(0), dpre @ self.w.to(dt))

    def check(self, act, tag, ws=None, ws_bytes=0):
        L = _L()
        dw_r, db_r, dx_r = self.outputs()
        L.check(self.call(act, dw_r, db_r, dx_r, ws, ws_bytes), "s2p_linear_bwd")
        (w64, b64, x64), (w32, b32, x32) = self.ref(act, torch.float64), self.ref(act, torch.float32)
        dx = dx_r.get(tag + " dx")
        _check("backward dw", dw_r.get(tag + " dw"), w64, w32, "%s act %d" % (tag, act))
        _check("backward db", db_r.get(tag + " db")[0], b64, b32, "%s act %d" % (tag, act))
        _check("backward dx", dx, x64, x32, "%s act %d" % (tag, act))
        assert bool((dx[:, self.k_real:] == 0).all())                           # the input padding's gradient is exactly zero
        return dw_r, db_r, dx_r


@pytest.mark.parametrize("M", [1, 5, 65, 130])
@pytest.mark.parametrize("k_real,K,N", [(5, 8, 4), (130, 132, 20), (40, 40, 72)])
def test_backward_accumulates_and_every_optional_output(hip_device, M, k_real, K, N):
    """M = 65 / 130: one row / two rows past the weight gradient's 64-row batch step and the input gradient's 64-row block."""
    L = _L()
    for i, act in enumerate((L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU)):
        c = BwdCase(M, k_real, K, N, seed=100 * M + K + i, wide_dx=(i != 1))       # (relu: dx_pitch == K exactly)
        tag = "M %d k %d/%d N %d" % (M, k_real, K, N)
        dw_r, db_r, dx_r = c.check(act, tag)
        again = c.outputs()
        L.check(c.call(act, *again), "s2p_linear_bwd")
        assert all(torch.equal(a.bits(), b.bits()) for a, b in zip(again, (dw_r, db_r, dx_r)))    # two identical calls: equal bits
        dw2, _, dx2 = c.outputs(db=False)
        L.check(c.call(act, dw2, None, dx2), "s2p_linear_bwd")                  # db == NULL
        assert torch.equal(dw2.bits("dw, no db"), dw_r.bits()) and torch.equal(dx2.bits("dx, no db"), dx_r.bits())
        dw3, db3, _ = c.outputs(dx=False)
        L.check(c.call(act, dw3, db3, None, with_w=False), "s2p_linear_bwd")    # dx == NULL with w_bwd == NULL
        assert torch.equal(dw3.bits("dw, no dx"), dw_r.bits()) and torch.equal(db3.bits("db, no dx"), db_r.bits())
        for r in (c.x_r, c.dy_r, c.y_r, c.wb_r):
            r.get("an input was written")


def _workspace(nbytes):
    """A workspace of exactly `nbytes` between two sentinel bands."""
    n = (nbytes + 3) // 4
    buf = torch.full((2 * BAND + n,), SENT, device="cuda")
    return buf, buf[BAND:].data_ptr()


@pytest.mark.parametrize("N", [2044, 2048, 2052])
def test_split_k_input_gradient_at_its_threshold(hip_device, N):
    """N = 2044: the last unsplit size; 2048: four full splits of 512; 2052: five splits of 448 with a last one of 260.  The workspace
    is exactly s2p_linear_bwd_workspace bytes; a short or missing one is refused before ANY launch: dw and db keep their bits too."""
    L = _L()
    lib = L.lib()
    M, K = 3, 8
    c = BwdCase(M, K, K, N, seed=N)
    need = lib.s2p_linear_bwd_workspace(M, K, N)
    assert (need == 0) == (N < 2048) and (N < 2048 or need == ((N + 511) // 512) * M * K * 4)
    buf, ws = _workspace(need)
    ws = ws if need else None
    dw_r, db_r, dx_r = c.check(L.ACT_LRELU, "split N %d" % N, ws, need)
    torch.cuda.synchronize()
    assert bool((buf[:BAND] == SENT).all()) and bool((buf[BAND + need // 4:] == SENT).all()), "workspace overrun"
    again = c.outputs()
    L.check(c.call(L.ACT_LRELU, *again, ws, need), "s2p_linear_bwd")
    assert all(torch.equal(a.bits(), b.bits()) for a, b in zip(again, (dw_r, db_r, dx_r)))
    if need:
        for bad_ws, bad_bytes in ((ws, need - 1), (None, need), (None, 0)):
            dw2, db2, dx2 = c.outputs()
            assert c.call(L.ACT_LRELU, dw2, db2, dx2, bad_ws, bad_bytes) != 0 and lib.s2p_last_error()
            assert dx2.untouched()
            assert torch.equal(dw2.bits(), c.dw0) and torch.equal(db2.bits()[0], c.db0)    # no launch preceded the refusal
        dw3, db3, _ = c.outputs(dx=False)                                       # without dx no workspace is needed
        L.check(c.call(L.ACT_LRELU, dw3, db3, None, None, 0, with_w=False), "s2p_linear_bwd")
        assert torch.equal(dw3.bits(), dw_r.bits()) and torch.equal(db3.bits(), db_r.bits())


def test_backward_refusals_leave_every_output_alone(hip_device):
    L = _L()
    lib = L.lib()
    c = BwdCase(5, 8, 8, 4, seed=3)
    for act in (L.ACT_TANH, L.ACT_SWISH, 5, -1):
        dw_r, db_r, dx_r = c.outputs()
        assert c.call(act, dw_r, db_r, dx_r) != 0 and lib.s2p_last_error(), act
        assert dx_r.untouched() and torch.equal(dw_r.bits(), c.dw0) and torch.equal(db_r.bits()[0], c.db0), act
    dw_r, db_r, dx_r = c.outputs()
    assert c.call(L.ACT_NONE, dw_r, db_r, dx_r, with_w=False) != 0 and lib.s2p_last_error()      # dx needs w_bwd
    assert dx_r.untouched() and torch.equal(dw_r.bits(), c.dw0) and torch.equal(db_r.bits()[0], c.db0)


# ---- the additive-term entry points against the plain ones, bit for bit ------------------------------------------------------------------
def add_fwd_call(x_r, w_r, b_r, M, K, N, add_r, act, y_r, n_store, slope=SLOPE):
    return _L().lib().s2p_linear_add_fwd(x_r.ptr, M, K, x_r.pitch, w_r.ptr, w_r.pitch, _p(b_r), N, _p(add_r), add_r.pitch if add_r is not None else 0,
                                         act, slope, y_r.ptr, y_r.pitch, n_store, _st())


def _fwd_inputs(M, K, N, seed):
    g = torch.Generator().manual_seed(seed)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5 * 1.5, torch.randn(N, generator=g)
    return Region(M, K, pitch=K + 8, off=4, fill=x), Region(N, K, pitch=K + 8, off=4, fill=w), Region(1, N, off=1, fill=b[None])


@pytest.mark.parametrize("M,K,N,n_store", [(1, 4, 1, 4), (17, 132, 20, 24), (65, 260, 72, 72)])
def test_linear_add_fwd_without_add_equals_linear_fwd_bitwise(hip_device, M, K, N, n_store):
    """slac.py picks s2p_linear_fwd or s2p_linear_add_fwd per layer (ops.linear_fwd_into) and the fused posterior chain promises the
    bits of both: with add == NULL the two entry points return the same bits, zero padding columns included."""
    L = _L()
    x_r, w_r, b_r = _fwd_inputs(M, K, N, seed=7000 + 10 * M + K)
    for act in (L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU, L.ACT_TANH, L.ACT_SWISH):
        for bias in (b_r, None):
            y_r, ya_r = Region(M, n_store, pitch=n_store + 8, off=4), Region(M, n_store, pitch=n_store + 8, off=4)
            L.check(fwd_call(x_r, w_r, bias, M, K, N, act, y_r, n_store), "s2p_linear_fwd")
            L.check(add_fwd_call(x_r, w_r, bias, M, K, N, None, act, ya_r, n_store), "s2p_linear_add_fwd")
            what = "act %d bias %d" % (act, bias is not None)
            assert torch.equal(ya_r.bits("add_fwd " + what), y_r.bits("fwd " + what)), what
    for r in (x_r, w_r, b_r):
        r.get("an input was written")


def test_linear_add_fwd_with_a_zero_add_equals_no_add_bitwise(hip_device):
    """add = +0.0f everywhere: (acc + 0) + bias has the bits of acc + bias (x + 0 = x for every x but -0, and -0 + 0 = +0 differs
    from -0 only until the bias is added: a random bias is never -0)."""
    L = _L()
    M, K, N, n_store = 17, 132, 20, 24
    x_r, w_r, b_r = _fwd_inputs(M, K, N, seed=7777)
    add_r = Region(M, N, pitch=N + 8, off=4, fill=torch.zeros(M, N))
    for act in (L.ACT_NONE, L.ACT_LRELU):
        y0_r, y1_r = Region(M, n_store, pitch=n_store + 8, off=4), Region(M, n_store, pitch=n_store + 8, off=4)
        L.check(add_fwd_call(x_r, w_r, b_r, M, K, N, None, act, y0_r, n_store), "s2p_linear_add_fwd")
        L.check(add_fwd_call(x_r, w_r, b_r, M, K, N, add_r, act, y1_r, n_store), "s2p_linear_add_fwd")
        assert torch.equal(y1_r.bits("zero add, act %d" % act), y0_r.bits("no add, act %d" % act)), act
    for r in (x_r, w_r, b_r, add_r):
        r.get("an input was written")


@pytest.mark.parametrize("wide_dx", [True, False])
@pytest.mark.parametrize("M", [1, 65])
@pytest.mark.parametrize("k_real,K,N", [(5, 8, 4), (130, 132, 20)])
def test_linear_add_bwd_equals_linear_bwd_bitwise(hip_device, M, k_real, K, N, wide_dx):
    """dx_accumulate = 0 and dadd = NULL: s2p_linear_add_bwd is s2p_linear_bwd in dw, db and dx, from the same starting dw / db.
    Both dx geometries of BwdCase: a pitch above K with a column offset, and dx_pitch == K exactly (the rule for how many dx columns
    are written compares K rounded up to 4 with dx_pitch)."""
    L = _L()
    lib = L.lib()
    for i, act in enumerate((L.ACT_NONE, L.ACT_RELU, L.ACT_LRELU)):
        c = BwdCase(M, k_real, K, N, seed=9000 + 100 * M + K + i, wide_dx=wide_dx)
        dw_r, db_r, dx_r = c.outputs()
        L.check(c.call(act, dw_r, db_r, dx_r), "s2p_linear_bwd")
        dwa_r, dba_r, dxa_r = c.outputs()
        L.check(lib.s2p_linear_add_bwd(c.x_r.ptr, c.x_r.pitch, c.dy_r.ptr, c.dy_r.pitch, c.y_r.ptr, c.y_r.pitch, M, K, k_real, N, c.wb_r.ptr,
                                       c.wb_r.pitch, act, SLOPE, dwa_r.ptr, dwa_r.pitch, dba_r.ptr, dxa_r.ptr, dxa_r.pitch, 0, None, 0, _st()),
                "s2p_linear_add_bwd")
        for name, a, b in (("dw", dwa_r, dw_r), ("db", dba_r, db_r), ("dx", dxa_r, dx_r)):
            assert torch.equal(a.bits("add_bwd " + name), b.bits("bwd " + name)), (name, act)
        for r in (c.x_r, c.dy_r, c.y_r, c.wb_r):
            r.get("an input was written")


def test_zz_report_worst_ratios(hip_device):
    print("\nworst deviation / max(ref32_err, 1e-6) per group:", {k: round(v, 3) for k, v in WORST.items()})
    assert WORST and max(WORST.values()) <= K_TOL
