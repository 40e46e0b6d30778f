"""Intensity-scale block sums on the GPU (csrc/neighbour.hip: adnm_valid_iscale_accum; ops.intensity_scale_sums; Validator(intensity_scale=True)):
exact, integer for integer over the whole table, against reshape(P/s, s, P/s, s).sum((1, 3)) on the thresholded quantised fields on the CPU
(iscale_ref), against the pooled pass the Validator already runs, and end to end through the captured graph.

Shapes: 1 x 1, 1 x 7, 5 x 7 (L < 5: one tile serves every level, most of it padding); 31 x 33, 32 x 32, 33 x 32 (one whole tile; ragged tiles; the
16-byte and the float-by-float loads); 64 x 64 (the first level the fold builds) and 65 x 63; 96 x 40 (P = 128, most of the domain padding) and
128 x 128; 3 x 1024 and 1024 x 3 (L = 10, 32 tiles in a line: every level of the fold's pyramid); 1025 x 1 raises.  The reference of a shape is
made once, for the eight thresholds, and the other threshold sets read their columns of it."""
import ctypes

import numpy as np
import pytest
import torch

import iscale_ref as F
import verify_ref as R
from adnm_hip import lib, ops
from util import guarded_workspaces

pytestmark = pytest.mark.gpu
DEV = "cuda"
THR, SCALE = R.THR, R.SCALE
EIGHT = F.THR_SETS["eight"]
SHAPES = [(1, 1), (1, 7), (5, 7), (31, 33), (32, 32), (33, 32), (64, 64), (65, 63), (96, 40), (128, 128), (3, 1024), (1024, 3)]
SHIFTS = (1, 2, 4, 8, 16)

_cases = {}


def _case(H, W):
    """-> (target, forecast, names, the reference for the eight thresholds), made once and never written to.  One frame per pattern: all-zero;
    all-event; a checkerboard against a zero forecast; a half-plane against itself moved one pixel; pred == target; the target moved by
    1, 2, 4, 8 and 16 px (a clean radar-like frame); noise at 0.1 and 0.5; two radar-like frames with NaN, +-Inf, negatives and values > 1 planted.  The two shapes of
    L = 10 take three of them (their domain has 2^20 pixels a frame on the CPU)."""
    if (H, W) not in _cases:
        rad_t, rad_p = F.radar_fields(2, H, W, 7 + H + W, plant=H * W >= 35)
        zero, one, board, half = np.zeros((1, H, W), np.float32), np.full((1, H, W), 0.9, np.float32), F.checkerboard(1, H, W), F.half_plane(1, H, W)
        n1, n5 = F.noise(1, H, W, 0.1, H), F.noise(1, H, W, 0.5, W)
        frames = [("zero", zero, zero), ("all", one, one), ("board", board, zero), ("half", half, F.shifted(half, 1)), ("same", rad_t[:1], rad_t[:1])]
        clean = R.radar_fields(1, H, W, 7)[0]      # (nothing planted: a lone +Inf pixel is an error of scale 1 wherever it is moved to)
        frames += [(f"shift{px}", clean, F.shifted(clean, px)) for px in SHIFTS]
        frames += [("noise0.1",) + n1, ("noise0.5",) + n5, ("radar0", rad_t[:1], rad_p[:1]), ("radar1", rad_t[1:], rad_p[1:])]
        if max(H, W) > 512:
            frames = [f for f in frames if f[0] in ("all", "noise0.5", "radar1")]
        t, p = (np.concatenate([f[i] for f in frames]) for i in (1, 2))
        ref = F.ref_sums(t, p, EIGHT, SCALE)
        for a in (t, p, ref):
            a.setflags(write=False)
        _cases[(H, W)] = (t, p, [f[0] for f in frames], ref)
    return _cases[(H, W)]


def _columns(thr):
    """the columns of the eight-threshold reference that belong to the thresholds `thr`"""
    return [3 * EIGHT.index(v) + c for v in thr for c in range(3)]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the cached cases are read-only)


def _same(got, ref, what=""):
    assert got.dtype == torch.int64 and tuple(got.shape) == ref.shape, (what, got.dtype, tuple(got.shape), ref.shape)
    got = got.cpu().numpy()
    bad = got != ref
    assert not bad.any(), f"{what}: {int(bad.sum())} of {ref.size} sums differ from the block counts; the first at (frame, level, column) {tuple(np.argwhere(bad)[0])}: " \
                          f"{got[bad][0]} for {ref[bad][0]}"
    return got


# ------------------------------------------------------------------------------------------------ 1. exact against the reference
@pytest.mark.parametrize("thr_name", list(F.THR_SETS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sums_equal_the_block_counts(shape, thr_name):
    H, W = shape
    t, p, names, ref = _case(H, W)
    thr = F.THR_SETS[thr_name]
    P, L = F.levels(H, W)
    assert ops.intensity_scale_levels(H, W) == (P, L) and ref.shape == (len(t), L + 1, 24)
    got = _same(ops.intensity_scale_sums(_dev(t), _dev(p), thr, SCALE), ref[:, :, _columns(thr)], f"{H} x {W} {thr_name}")
    a, f, c = got[:, :, 0::3], got[:, :, 1::3], got[:, :, 2::3]
    i = names.index("all")          # every pixel an event at every threshold below 81: the top level's addend is (H W)^2
    k = [v <= 81 for v in thr]
    assert (got[i, L][np.repeat(k, 3)] == (H * W) ** 2).all() and (a[i, 0][k] == H * W).all()
    if "zero" in names:
        assert (got[names.index("zero")] == 0).all()
        j = names.index("same")
        assert (a[j] == f[j]).all() and (a[j] == c[j]).all(), "pred == target"
        assert (f[names.index("board")] == 0).all() and (a[names.index("board"), 0][k] == (H * W + 1) // 2).all()
    if H * W >= 1024:
        assert (a.sum(axis=0) > 0)[:, [v <= 40 for v in thr]].all(), "a threshold without events: nothing is compared there"


def test_the_yardstick_sees_the_error_move_to_coarser_scales_with_the_shift():
    """on the yardstick alone: the component with the largest MSE does not move to a finer scale as the target is moved by 1, 2, 4, 8, 16 px"""
    t, p, names, ref = _case(128, 128)
    col = _columns([20])
    peak = []
    for px in SHIFTS:
        s = ref[names.index(f"shift{px}")][:, col]
        peak.append(int(F.components(s[:, 0] + s[:, 1] - 2 * s[:, 2], 1, 128).argmax()))
    print("the scale index of the largest component per shift", peak)
    assert all(b >= a for a, b in zip(peak, peak[1:])) and peak[-1] > peak[0]


def test_a_frame_above_the_limit_raises():
    z = torch.zeros(1, 1025, 1, device=DEV)
    with pytest.raises(ValueError, match="1024"):
        ops.intensity_scale_sums(z, z, THR, SCALE)
    with pytest.raises(ValueError, match="1024"):
        ops.intensity_scale_sums(z.transpose(1, 2), z.transpose(1, 2), THR, SCALE)
    with pytest.raises(ValueError, match="thresholds"):
        ops.intensity_scale_sums(z[:, :8], z[:, :8], [], SCALE)


# ------------------------------------------------------------------------------------------------ 2. the same as the kernel we have
@pytest.mark.parametrize("shape", [(96, 40), (65, 63)], ids=["96x40", "65x63"])
def test_the_finest_and_the_coarsest_level_are_the_point_counts(shape):
    """A_0 = TP + FN, F_0 = TP + FP, C_0 = TP of the pooled pass at the (1, 1) pool, and per frame A_L = (TP + FN)^2, F_L = (TP + FP)^2,
    C_L = (TP + FN)(TP + FP): the domain block holds every event"""
    t, p, names, _ = _case(*shape)
    L = F.levels(*shape)[1]
    got = ops.intensity_scale_sums(_dev(t), _dev(p), THR, SCALE)
    cnt = ops.pool_counts(_dev(t), _dev(p), THR, SCALE, ((1, 1),))[:, 0].to(torch.int64).reshape(len(t), len(THR), 4)
    tp, fn, fp = cnt[..., 0], cnt[..., 1], cnt[..., 2]
    assert int(tp.sum()) > 0 and int(fn.sum()) > 0 and int(fp.sum()) > 0
    for c, (fine, coarse) in enumerate(((tp + fn, (tp + fn) ** 2), (tp + fp, (tp + fp) ** 2), (tp, (tp + fn) * (tp + fp)))):
        assert torch.equal(got[:, 0, c::3], fine) and torch.equal(got[:, L, c::3], coarse), "AFC"[c]


# ------------------------------------------------------------------------------------------------ the entry point, called directly
def _table(T, nthr, H, W, fill=0.0):
    n = lib.query("adnm_valid_iscale_block_bytes", T, nthr, H, W) // 8
    assert n == T * (F.levels(H, W)[1] + 1) * 3 * nthr
    return torch.full((n,), fill, dtype=torch.float64, device=DEV)


def _accum(pred_ptr, sample_stride, frame_stride, tgt, table, thr, T, ws=None):
    """tgt: contiguous (frames, H, W) on the device; the forecast by address and strides"""
    frames, H, W = tgt.shape
    nb = lib.query("adnm_valid_iscale_accum_ws_bytes", frames, T, H, W, len(thr))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV) if ws is None else ws
    lib.call("adnm_valid_iscale_accum", pred_ptr, sample_stride, frame_stride, tgt.data_ptr(), table.data_ptr(), (ctypes.c_float * len(thr))(*thr), len(thr), SCALE,
             ws.data_ptr(), nb, frames, T, H, W, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return nb


# ------------------------------------------------------------------------------------------------ 3. accumulation and mapping
def test_rows_are_frame_indices_batches_add_and_two_runs_are_the_same_bits():
    B, T, H, W = 4, 3, 65, 63
    L = F.levels(H, W)[1]
    batches = [F.radar_fields(B * T, H, W, seed, plant=True) for seed in (1, 2)]
    refs = [F.ref_sums(t, p, THR, SCALE).reshape(B, T, L + 1, -1) for t, p in batches]
    assert not (refs[0].sum(0) == refs[0].reshape(T, B, L + 1, -1).sum(1)).all(), "f mod T and f / T coincide on this data: nothing is tested"
    start = np.arange(T * (L + 1) * 3 * len(THR), dtype=np.float64).reshape(T, L + 1, -1) * 3.0      # the table is ADDED to
    tables = []
    for _ in range(2):
        table = _dev(start.ravel().copy())
        for i, (t, p) in enumerate(batches):
            pred = _dev(p)
            _accum(pred.data_ptr(), T * H * W, H * W, _dev(t), table, THR, T)
            want = start + sum(r.sum(0) for r in refs[:i + 1])      # row t: the reference summed over the samples; a second batch adds
            assert (table.view(T, L + 1, -1).cpu().numpy() == want).all(), f"after batch {i}"
        tables.append(table)
    assert torch.equal(tables[0].view(torch.int64), tables[1].view(torch.int64)), "the same calls on a fresh table give other bits"


# ------------------------------------------------------------------------------------------------ 4. addressing
@pytest.mark.parametrize("H,W", [(33, 32), (65, 63)], ids=["quads", "odd"])
def test_a_held_frame_a_slice_of_a_wider_tensor_and_bases_off_by_one_float(H, W):
    B, T, T_in = 2, 3, 2
    L = F.levels(H, W)[1]
    t, p = F.radar_fields(B * T, H, W, 3, plant=True)
    tgt, pred = _dev(t), _dev(p)
    want = _table(T, len(THR), H, W)
    _accum(pred.data_ptr(), T * H * W, H * W, tgt, want, THR, T)
    assert (want.view(T, L + 1, -1).cpu().numpy() == F.ref_sums(t, p, THR, SCALE).reshape(B, T, L + 1, -1).sum(0)).all()
    # persistence: the last input frame, held for every frame index (a frame stride of 0)
    xd = _dev(F.radar_fields(B * T_in, H, W, 4)[1].reshape(B, T_in, H, W))
    a, b = _table(T, len(THR), H, W), _table(T, len(THR), H, W)
    _accum(xd.data_ptr() + 4 * (T_in - 1) * H * W, T_in * H * W, 0, tgt, a, THR, T)
    held = xd[:, -1:].expand(B, T, H, W).contiguous().view(B * T, H, W)
    _accum(held.data_ptr(), T * H * W, H * W, tgt, b, THR, T)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    ref = F.ref_sums(t, held.cpu().numpy(), THR, SCALE).reshape(B, T, L + 1, -1).sum(0)
    assert (a.view(T, L + 1, -1).cpu().numpy() == ref).all() and (ref[:, :, 1::3] > 0).all(), "the held frame"
    # the forecast as frames 1..T of a (B, T + 2, H, W) tensor: a sample stride larger than T*H*W
    wide = torch.full((B, T + 2, H, W), 0.9, dtype=torch.float32, device=DEV)
    wide[:, 1:T + 1] = pred.view(B, T, H, W)
    got = _table(T, len(THR), H, W)
    _accum(wide[:, 1:].data_ptr(), (T + 2) * H * W, H * W, tgt, got, THR, T)
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)), "a slice of a wider tensor"
    # both fields one float into a buffer: 4-byte aligned only, so a W that is a multiple of 4 is read float by float as well
    hold_p, hold_t = (torch.zeros(B * T * H * W + 1, dtype=torch.float32, device=DEV) for _ in range(2))
    off_p, off_t = hold_p[1:].view(B * T, H, W), hold_t[1:].view(B * T, H, W)
    off_p.copy_(pred), off_t.copy_(tgt)
    assert off_p.data_ptr() % 16 == 4 and off_t.data_ptr() % 16 == 4 and pred.data_ptr() % 16 == 0 and tgt.data_ptr() % 16 == 0
    got = _table(T, len(THR), H, W)
    _accum(off_p.data_ptr(), T * H * W, H * W, off_t, got, THR, T)
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)), "bases one float off the 16-byte boundary"


# ------------------------------------------------------------------------------------------------ 5. workspace hygiene
@pytest.mark.parametrize("shape", [(5, 7), (65, 63), (3, 1024)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_guarded_poisoned_workspace_changes_nothing(monkeypatch, shape):
    """every word the fold reads was written by the tile kernel of this call, and nothing outside the queried bytes is touched"""
    t, p, _, ref = _case(*shape)
    with guarded_workspaces(monkeypatch) as g:
        got = ops.intensity_scale_sums(_dev(t), _dev(p), THR, SCALE)
        g.check()
        assert g.calls == 1 and g.records[0][2] == lib.query("adnm_valid_iscale_accum_ws_bytes", len(t), len(t), *shape, len(THR))
    _same(got, ref[:, :, _columns(THR)], f"{shape} under a poisoned workspace")


def test_nothing_behind_the_table_is_written():
    H, W, T = 65, 63, 3
    t, p = F.radar_fields(2 * T, H, W, 5)
    cells = T * (F.levels(H, W)[1] + 1) * 3 * len(THR)
    hold = torch.full((cells + 8,), -7.0, dtype=torch.float64, device=DEV)
    hold[:cells] = 0.0
    pred = _dev(p)
    _accum(pred.data_ptr(), T * H * W, H * W, _dev(t), hold, THR, T)
    assert bool((hold[cells:] == -7.0).all()), "a write behind the table"
    assert (hold[:cells].view(T, -1, 3 * len(THR)).cpu().numpy() == F.ref_sums(t, p, THR, SCALE).reshape(2, T, -1, 3 * len(THR)).sum(0)).all()


# ------------------------------------------------------------------------------------------------ 6. the Validator end to end
class _Drift(torch.nn.Module):
    """a stand-in forecast: the last input frame, moved one pixel more and weakened with every lead"""

    def forward(self, x):
        last = x[:, -1, 0].float()
        return torch.stack([torch.roll(last, t + 1, dims=-1) * (1.0 - 0.02 * t) for t in range(20)], dim=1)


def _strip(res):
    """done()'s dictionary without the intensity-scale entries"""
    out = {k: v for k, v in res.items() if k != "intensity_scale"}
    for name in ("persistence", "advection"):
        out[name] = {k: v for k, v in res[name].items() if k != "intensity_scale"}
    if "per_lead" in out:
        out["per_lead"] = _strip(res["per_lead"])
    return out


def test_validator_through_the_captured_graph_beside_fss_and_both_baselines():
    from adnm_hip.validate import Validator, intensity_scale_entries, iscale_doubles
    from models.loss import RainfallLoss
    from test_tracks_host import _same_tree
    B, T, H, W, n = 2, 20, 64, 64, len(THR)
    rng = np.random.default_rng(11)
    base = 1.2 * R.blobs(rng, 2 * B, H, W, 3) + rng.normal(0.0, 0.004, size=(2 * B, H, W))
    samples = _dev(np.stack([np.roll(base, 2 * j, axis=2) for j in range(5 + T)], axis=1).astype(np.float32))      # the truth moves 2 px a frame
    data = [(samples[i:i + B, :5, None].contiguous(), samples[i:i + B, 5:, None].contiguous()) for i in (0, B)]
    options = dict(fss=(1, 9), persistence=True, advection=True)
    val = Validator(_Drift(), RainfallLoss(), T, SCALE, THR, intensity_scale=True, **options)
    old = Validator(_Drift(), RainfallLoss(), T, SCALE, THR, **options)
    try:
        sums = {"iscale": 0, "persistence/iscale": 0, "advection/iscale": 0}
        for x, tgt in data:
            pred = val.step(x, tgt)
            old.step(x, tgt)
            fields = {"iscale": pred, "persistence/iscale": x[:, -1:, 0].expand(B, T, H, W), "advection/iscale": val.advected(x)}
            for name, field in fields.items():      # the one-shot op on the graph's own fields
                sums[name] = sums[name] + ops.intensity_scale_sums(tgt[:, :, 0], field.contiguous(), THR, SCALE).view(B, T, 7, 3 * n).sum(0)
        parts = {p.name: p for p in val._parts}
        assert [p.name for p in val._parts][-3:] == list(sums) and val._block.numel() == old._block.numel() + sum(iscale_doubles(T, n, (H, W), True, True))
        assert all(e.get("ws_iscale") is None for e in old._fwd._graphs.values()) and all(e["ws_iscale"] is not None for e in val._fwd._graphs.values())
        for name, want in sums.items():
            tab = val._block[parts[name].offset:parts[name].offset + parts[name].size].view(T, 7, 3 * n)
            assert torch.equal(tab.to(torch.int64), want) and torch.equal(tab, want.double()), name
            assert int(want[:, :, 0].min()) > 0 and int(want[:, :, 1].min()) > 0 and int(want[:, :, 9:].sum()) > 0, "no event in a field: nothing is compared"
        assert not torch.equal(sums["iscale"], sums["persistence/iscale"]) and not torch.equal(sums["iscale"], sums["advection/iscale"])
        # the bits in front of the new tables are the other Validator's block
        assert torch.equal(val._block[:old._block.numel()].view(torch.int64), old._block.view(torch.int64))
        res, ref = val.done(per_lead=True), old.done(per_lead=True)
        assert repr(_strip(res)) == repr(ref), "an existing entry moved"
        assert list(res)[-2:] == ["intensity_scale", "per_lead"] and list(res["persistence"])[-1] == "intensity_scale" == list(res["advection"])[-1]
        for name, got, lead in (("iscale", res["intensity_scale"], res["per_lead"]["intensity_scale"]),
                                ("persistence/iscale", res["persistence"]["intensity_scale"], res["per_lead"]["persistence"]["intensity_scale"]),
                                ("advection/iscale", res["advection"]["intensity_scale"], res["per_lead"]["advection"]["intensity_scale"])):
            rows = sums[name].cpu().numpy()
            assert _same_tree(got, intensity_scale_entries(rows.sum(axis=0), 2 * B * T, (H, W), THR)), name
            assert _same_tree(lead, intensity_scale_entries(rows, 2 * B, (H, W), THR)), name
        e = res["intensity_scale"]
        assert e["scale_px"].tolist() == [1, 2, 4, 8, 16, 32, 64] and (e["domain_px"], e["levels"]) == (64, 6)
        m = res["threshold_metrics"][20]
        assert e[20]["mse_total"] == (m["FP"] + m["FN"]) / (2 * B * T * H * W) and abs(e[20]["mse"].sum() - e[20]["mse_total"]) < 1e-15
        print("skill per scale at 20: forecast", e[20]["skill"], "persistence", res["persistence"]["intensity_scale"][20]["skill"])
        # a second epoch replays the graph: the same bits; and a step allocates nothing
        block = val._block.clone()
        val.done(reset=True)
        assert float(val._block.abs().sum()) == 0.0
        for x, tgt in data:
            val.step(x, tgt)
        assert torch.equal(val._block.view(torch.int64), block.view(torch.int64))
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        val.step(*data[0])
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
        # one frame size for the Validator's lifetime
        val.done(reset=True)
        small = torch.zeros(B, 5, 1, 32, 32, device=DEV), torch.zeros(B, T, 1, 32, 32, device=DEV)
        with pytest.raises(RuntimeError, match="intensity_scale=True keeps one frame size"):
            val.step(*small)
    finally:
        val.close()
        old.close()
