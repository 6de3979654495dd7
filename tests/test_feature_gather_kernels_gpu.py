"""N3g -- s2p_feature_window_gather (csrc/replay.hip) against plain torch indexing: `features[table[win].long()]`,
`create_feature_actions`, `action_[win]`.  The kernel is a copy, so every comparison is `torch.equal` on fp32 bits.  Every output
lives in a sentinel-guarded, NaN-filled region (tests/guard_region.py): a store outside an output, or a pad column left unwritten,
shows."""
import pytest
import torch

from guard_region import Region

pytestmark = pytest.mark.gpu
OUTPUTS = ("feature_", "fa", "next_fa", "action_seq", "action_last", "reward", "terminal")


def _problem(B, T, F, A, n_slots=11, n_windows=7, feat_pitch=None, win=None, seed=0, dev="cuda"):
    g = torch.Generator().manual_seed(100 + seed)
    feat_pitch = F if feat_pitch is None else feat_pitch
    feat = torch.randn(n_slots, feat_pitch, generator=g)
    table = torch.randint(0, n_slots, (n_windows, T), generator=g, dtype=torch.int32)
    win = torch.randint(0, n_windows, (B,), generator=g, dtype=torch.int64) if win is None else torch.tensor(win, dtype=torch.int64)
    action_ = torch.randn(n_windows, T - 1, A, generator=g)
    reward_, done_ = torch.randn(n_windows, T - 1, 1, generator=g), (torch.rand(n_windows, T - 1, 1, generator=g) < 0.5).float()
    return dict(feat=feat, table=table, win=win, action_=action_, reward_=reward_, done_=done_, F=F, A=A, T=T, B=len(win), n_slots=n_slots)


def _want(p):
    """The seven outputs by plain torch indexing on the CPU; a slot outside [0, n_slots) is a zero row."""
    from s2p_amd.slac import create_feature_actions
    rows = p["table"][p["win"]].long()
    ok = (rows >= 0) & (rows < p["n_slots"])
    f = p["feat"][:, :p["F"]][rows.clamp(0, p["n_slots"] - 1)]
    f = torch.where(ok[..., None], f, torch.zeros(()))
    a = p["action_"][p["win"]]
    fa, nfa = create_feature_actions(f, a)
    return dict(feature_=f.reshape(-1, p["F"]), fa=fa, next_fa=nfa, action_seq=a.reshape(len(a), -1), action_last=a[:, -1],
                reward=p["reward_"][p["win"], -1], terminal=p["done_"][p["win"], -1])


def _regions(p, fa_pitch, alp):
    B, T, F, A = p["B"], p["T"], p["F"], p["A"]
    nan = float("nan")
    shapes = dict(feature_=(B * T, F), fa=(B, fa_pitch), next_fa=(B, fa_pitch), action_seq=(B, (T - 1) * A), action_last=(B, alp),
                  reward=(B, 1), terminal=(B, 1))
    return {k: Region(m, w, pitch=w, fill=torch.full((m, w), nan)) for k, (m, w) in shapes.items()}


def _launch(p, regions, fa_pitch, alp, null=()):
    from s2p_amd import _lib
    L = _lib.lib()
    d = {k: v.cuda() for k, v in p.items() if torch.is_tensor(v)}
    o = {k: (None if k in null else regions[k].ptr) for k in OUTPUTS}
    rc = L.s2p_feature_window_gather(d["feat"].data_ptr(), p["n_slots"], p["feat"].shape[1], p["F"], d["table"].data_ptr(), p["T"],
                                     d["win"].data_ptr(), p["B"], d["action_"].data_ptr(), d["reward_"].data_ptr(), d["done_"].data_ptr(),
                                     p["A"], o["feature_"], o["fa"], o["next_fa"], fa_pitch, o["action_seq"], o["action_last"], alp,
                                     o["reward"], o["terminal"], _lib.stream())
    torch.cuda.synchronize()
    return rc


def _check(p, regions, want, fa_pitch, alp, null=()):
    P = want["fa"].shape[1]
    for k in OUTPUTS:
        if k in null:
            assert regions[k].untouched(), k
            continue
        got = regions[k].bits(k)                                                   # (checks the guard bands)
        width = dict(fa=P, next_fa=P, action_last=p["A"]).get(k, got.shape[1])
        assert torch.equal(got[:, :width], want[k].reshape(got.shape[0], width)), k
        assert bool((got[:, width:] == 0).all()), k + ": pad columns"              # exactly 0, not the NaN they held


CASES = {
    "T2_no_action_columns": dict(B=1, T=2, F=4, A=1),
    "production_row": dict(B=3, T=9, F=256, A=6),
    "F_past_one_wave_pass": dict(B=5, T=3, F=260, A=3),
    "wide_fa_pitch": dict(B=2, T=9, F=256, A=7, fa_extra=8, alp_extra=5),
    "repeated_ids": dict(B=4, T=3, F=8, A=2, win=[1, 1, 0, 1]),
    "feat_pitch_above_F": dict(B=3, T=4, F=12, A=2, feat_pitch=20),
}


def _sizes(c, p):
    P = (p["T"] - 1) * p["F"] + (p["T"] - 2) * p["A"]
    return (P + 3) // 4 * 4 + c.get("fa_extra", 0), p["A"] + c.get("alp_extra", 0)


@pytest.mark.parametrize("name", list(CASES))
def test_gather_equals_torch_indexing(hip_device, name):
    c = CASES[name]
    p = _problem(c["B"], c["T"], c["F"], c["A"], feat_pitch=c.get("feat_pitch"), win=c.get("win"))
    fa_pitch, alp = _sizes(c, p)
    regions = _regions(p, fa_pitch, alp)
    assert _launch(p, regions, fa_pitch, alp) == 0
    _check(p, regions, _want(p), fa_pitch, alp)


@pytest.mark.parametrize("null", OUTPUTS)
def test_each_output_nulled_leaves_the_others_unchanged(hip_device, null):
    c = CASES["wide_fa_pitch"]
    p = _problem(c["B"], c["T"], c["F"], c["A"])
    fa_pitch, alp = _sizes(c, p)
    regions = _regions(p, fa_pitch, alp)
    for k in regions:
        if k == null:
            regions[k] = Region(regions[k].M, regions[k].width, pitch=regions[k].width)    # all sentinel: must stay so
    assert _launch(p, regions, fa_pitch, alp, null=(null,)) == 0
    _check(p, regions, _want(p), fa_pitch, alp, null=(null,))


def test_slots_out_of_range_read_as_zero_rows(hip_device):
    p = _problem(3, 4, 8, 2, win=[0, 1, 2])
    p["table"][0, 1], p["table"][1, 0], p["table"][2, 3] = -1, p["n_slots"], p["n_slots"] + 5
    want = _want(p)
    assert bool((want["feature_"].reshape(3, 4, 8)[0, 1] == 0).all()) and bool((want["feature_"].reshape(3, 4, 8)[0, 0] != 0).any())
    fa_pitch, alp = _sizes({}, p)
    regions = _regions(p, fa_pitch, alp)
    assert _launch(p, regions, fa_pitch, alp) == 0
    _check(p, regions, want, fa_pitch, alp)


def test_empty_batch_is_a_no_op_and_all_null_is_refused(hip_device):
    from s2p_amd import _lib
    p = _problem(2, 3, 8, 2)
    fa_pitch, alp = _sizes({}, p)
    regions = _regions(p, fa_pitch, alp)
    before = {k: r.buf.clone() for k, r in regions.items()}
    p0 = dict(p, win=p["win"][:0], B=0)
    assert _launch(p0, regions, fa_pitch, alp) == 0
    assert all(torch.equal(before[k].view(torch.int32), regions[k].buf.view(torch.int32)) for k in regions)
    assert _launch(p, regions, fa_pitch, alp, null=OUTPUTS) != 0
    assert b"null" in _lib.lib().s2p_last_error()
    assert all(torch.equal(before[k].view(torch.int32), regions[k].buf.view(torch.int32)) for k in regions)


def test_ops_wrapper_returns_views_of_pitched_buffers(hip_device):
    from s2p_amd import ops
    p = _problem(3, 9, 256, 6)                                # P = 2090, pitch 2092
    d = {k: v.cuda() for k, v in p.items() if torch.is_tensor(v)}
    got = ops.feature_window_gather(d["feat"], d["table"], d["win"], d["action_"], d["reward_"], d["done_"])
    want = _want(p)
    shapes = dict(feature_=(3, 9, 256), fa=(3, 2090), next_fa=(3, 2090), action_seq=(3, 8, 6), action_last=(3, 6), reward=(3, 1), terminal=(3, 1))
    for k, t in zip(OUTPUTS, got):
        assert tuple(t.shape) == shapes[k] and torch.equal(t.cpu(), want[k].reshape(shapes[k])), k
    assert got[1].stride(0) == 2092 and got[2].stride(0) == 2092


def test_feature_table_offsets_beyond_2_31(hip_device):
    """A 2.2 GB table, uninitialised but for its first and last rows (the precedent: test_gather_offsets_beyond_2_31)."""
    from s2p_amd import ops
    n_slots, F = 2_200_000, 256                                # 2.25e9 bytes: the last row starts beyond 2^31
    assert (n_slots - 1) * F * 4 > 2 ** 31
    g = torch.Generator().manual_seed(29)
    r0, r1 = torch.randn(F, generator=g), torch.randn(F, generator=g)
    feat = torch.empty((n_slots, F), dtype=torch.float32, device=hip_device)
    feat[0].copy_(r0)
    feat[n_slots - 1].copy_(r1)
    table = torch.tensor([[0, n_slots - 1], [n_slots - 1, 0]], dtype=torch.int32, device=hip_device)
    win = torch.tensor([1, 0], dtype=torch.int64, device=hip_device)
    action_ = torch.tensor([[[0.5]], [[-0.25]]], device=hip_device)
    reward_, done_ = torch.tensor([[[1.0]], [[2.0]]], device=hip_device), torch.tensor([[[0.0]], [[1.0]]], device=hip_device)
    feature_, fa, nfa, aseq, alast, rew, term = ops.feature_window_gather(feat, table, win, action_, reward_, done_)
    assert torch.equal(feature_.cpu(), torch.stack([r1, r0, r0, r1]).reshape(2, 2, F))
    assert torch.equal(fa.cpu(), torch.stack([r1, r0])) and torch.equal(nfa.cpu(), torch.stack([r0, r1]))
    assert aseq.cpu().flatten().tolist() == [-0.25, 0.5] and alast.cpu().flatten().tolist() == [-0.25, 0.5]
    assert rew.cpu().flatten().tolist() == [2.0, 1.0] and term.cpu().flatten().tolist() == [1.0, 0.0]
