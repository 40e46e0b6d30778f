"""Fractions Skill Score sums on the GPU (csrc/neighbour.hip: adnm_valid_fss_accum; ops.fss_sums; Validator(fss=)): exact, integer for
integer, against conv2d with an all-ones kernel on the thresholded quantised fields on the CPU (fss_ref), against the point-wise kernel
the Validator already runs, and end to end through the captured graph.  The floats derived from the sums use the same double expression
on both sides and are compared to 1e-12 relative."""
import ctypes

import numpy as np
import pytest
import torch

import fss_ref as F
import verify_ref as R
from adnm_hip import lib, ops, recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
THR, SCALE = R.THR, R.SCALE
SCALE_SETS = {"1": (1,), "1-5-17-33": (1, 5, 17, 33), "3-9": (3, 9)}

_fields, _refs = {}, {}


def _pair(n, H, W, seed):
    """the CPU fields of a case, made once and never written to"""
    key = (n, H, W, seed)
    if key not in _fields:
        _fields[key] = F.radar_fields(n, H, W, seed)
    return _fields[key]


def _ref(case, thr, scales):
    """the CPU reference of a case, made once and never written to"""
    key = (case, tuple(thr), tuple(scales))
    if key not in _refs:
        t, p = _pair(*case)
        _refs[key] = F.ref_sums(t, p, thr, SCALE, scales)
        _refs[key].setflags(write=False)
    return _refs[key]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check_exact(t, p, thr, scales, ref=None):
    got = ops.fss_sums(_dev(t), _dev(p), thr, SCALE, scales)
    ref = F.ref_sums(t, p, thr, SCALE, scales) if ref is None else ref
    assert got.dtype == torch.float64 and tuple(got.shape) == ref.shape == (len(t), len(scales), 3 * len(thr))
    got = got.cpu().numpy()
    assert (got == ref).all(), f"{int((got != ref).sum())} of {ref.size} sums differ from the window counts on the quantised fields"
    return got


# ------------------------------------------------------------------------------------------------ 1. exact against the reference
@pytest.mark.parametrize("thr_name", list(F.THR_SETS))
@pytest.mark.parametrize("scale_name", list(SCALE_SETS))
@pytest.mark.parametrize("case", F.CASES, ids=lambda c: "x".join(map(str, c[:3])))
def test_fss_sums_equal_the_window_counts(case, scale_name, thr_name):
    """64 x 64 and 128 x 128: whole tiles, 16-byte loads; 33 x 33 and 37 x 53: tile edges, a halo that crosses the frame border on all
    four sides and tile seams inside, float-by-float loads; 5 x 40 and 16 x 16 with n = 33: windows larger than the frame"""
    t, p = _pair(*case)
    thr, scales = F.THR_SETS[thr_name], SCALE_SETS[scale_name]
    ref = _ref(case, thr, scales)
    if thr_name != "eight":
        print("FSS range of the reference", F.assert_dense(ref, f"{case} {scales} {thr_name}"))
    else:
        assert (ref.sum(axis=0) > 0).any()
    got = _check_exact(t, p, thr, scales, ref)
    mine, want = F.fss(got.sum(axis=0)), F.fss(ref.sum(axis=0))
    assert ((np.isnan(mine) & np.isnan(want)) | (np.abs(mine - want) <= 1e-12 * np.abs(want))).all()


def test_the_eight_thresholds_have_empty_cells_and_a_nan_score():
    case = F.CASES[0]
    t, p = _pair(*case)
    got = _check_exact(t, p, F.THR_SETS["eight"], (1, 5, 17, 33), _ref(case, F.THR_SETS["eight"], (1, 5, 17, 33)))
    assert (got[:, :, 22:] == 0).all() and got[:, :, 21].sum() > 0, "threshold 70: the forecast has no event, the target has"
    assert (F.fss(got.sum(axis=0))[:, 7] == 0).all()
    empty = ops.fss_sums(torch.zeros(2, 16, 16, device=DEV), torch.zeros(2, 16, 16, device=DEV), THR, SCALE, (1, 33))
    assert float(empty.abs().sum()) == 0.0 and np.isnan(F.fss(empty.cpu().numpy())).all()


def test_a_full_frame_reaches_the_largest_count():
    """every pixel an event in both fields: the interior of a 70 x 70 frame has c = 33^2 = 1089, the largest count there is, and the
    sums are those of the window areas clipped by the frame"""
    ones = np.ones((1, 70, 70), dtype=np.float32)
    got = _check_exact(ones, ones, [30], (33, 1))
    side = np.minimum(np.arange(70) + 17, 70) - np.maximum(np.arange(70) - 16, 0)
    want = float((np.outer(side, side).astype(np.float64) ** 2).sum())
    assert side.max() == 33 and (got[0, 0] == want).all() and (got[0, 1] == 4900).all()


# ------------------------------------------------------------------------------------------------ the entry point, called directly
def _table(T, nthr, nscale):
    return torch.zeros(lib.query("adnm_valid_fss_block_bytes", T, nthr, nscale) // 8, dtype=torch.float64, device=DEV)


def _accum(pred_ptr, sample_stride, frame_stride, tgt, table, thr, scales, T, ws=None):
    """tgt: contiguous (frames, H, W) on the device; the forecast by address and strides"""
    frames, H, W = tgt.shape
    tab = lib.i64_table(list(scales))
    nb = lib.query("adnm_valid_fss_accum_ws_bytes", frames, T, H, W, len(thr), tab, len(scales))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV) if ws is None else ws
    lib.call("adnm_valid_fss_accum", pred_ptr, sample_stride, frame_stride, tgt.data_ptr(), table.data_ptr(), (ctypes.c_float * len(thr))(*thr), len(thr), SCALE,
             tab, len(scales), ws.data_ptr(), nb, frames, T, H, W, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return nb


def _accum_contig(pred, tgt, table, thr, scales, T):
    frames, H, W = tgt.shape
    assert pred.is_contiguous() and pred.shape == tgt.shape
    _accum(pred.data_ptr(), T * H * W, H * W, tgt, table, thr, scales, T)


# ------------------------------------------------------------------------------------------------ 2. the same as the kernel we have
def test_scale_one_equals_valid_accum_bit_for_bit():
    B, T, H, W, n = 2, 3, 17, 19, len(THR)
    block = torch.zeros(lib.query("adnm_valid_block_bytes", T, n) // 8, dtype=torch.float64, device=DEV)
    table = _table(T, n, 2)
    thr_c = (ctypes.c_float * n)(*THR)
    for seed in (0, 1):
        t, p = (_dev(a) for a in R.radar_fields(B * T, H, W, seed))
        nb = lib.query("adnm_valid_accum_ws_bytes", B * T, T, H * W, n)
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        lib.call("adnm_valid_accum", p.data_ptr(), t.data_ptr(), block.data_ptr(), None, thr_c, n, SCALE, 0.57, 0.25, 0.0, ws.data_ptr(), nb, B * T, T, H * W,
                 torch.cuda.current_stream().cuda_stream)
        _accum_contig(p, t, table, THR, (3, 1), T)
    main = block[4:].view(T, 4 * n + 3)[:, :4 * n].reshape(T, n, 4)        # TP, FN, FP, TN
    want = torch.stack([main[..., 0] + main[..., 1], main[..., 0] + main[..., 2], main[..., 0]], dim=-1).reshape(T, 3 * n).contiguous()
    mine = table.view(T, 2, 3 * n)[:, 1].contiguous()
    assert float(main.sum()) == 2.0 * n * B * T * H * W and float(main[..., 0].sum()) > 0
    assert torch.equal(want.view(torch.int64), mine.view(torch.int64))


# ------------------------------------------------------------------------------------------------ 3. accumulation and mapping
def test_rows_are_frame_indices_and_batches_add():
    B, T, H, W, scales = 3, 4, 37, 53, (1, 9, 33)
    batches = [R.radar_fields(B * T, H, W, seed) for seed in (1, 2)]
    refs = [F.ref_sums(t, p, THR, SCALE, scales).reshape(B, T, len(scales), -1) for t, p in batches]
    assert not (refs[0].sum(0) == refs[0].reshape(T, B, len(scales), -1).sum(1)).all(), "f mod T and f / T coincide on this data: nothing is tested"
    tables = []
    for _ in range(2):
        table = _table(T, len(THR), len(scales))
        for i, (t, p) in enumerate(batches):
            _accum_contig(_dev(p), _dev(t), table, THR, scales, T)
            if not tables:
                want = sum(r.sum(0) for r in refs[:i + 1])      # row t: the reference summed over the samples, a second batch adds
                assert (table.view(T, len(scales), -1).cpu().numpy() == want).all(), f"after batch {i}"
        tables.append(table)
    assert torch.equal(tables[0].view(torch.int64), tables[1].view(torch.int64)), "the same calls on a fresh table give other bits"


# ------------------------------------------------------------------------------------------------ 4. addressing
def test_frame_stride_zero_is_the_expanded_copy():
    B, T, T_in, H, W, scales = 3, 4, 2, 37, 53, (5, 1)
    t, x = R.radar_fields(B * T, H, W, 1)[0], R.radar_fields(B * T_in, H, W, 2)[1].reshape(B, T_in, H, W)
    tgt, xd = _dev(t), _dev(x)
    a, b = _table(T, len(THR), 2), _table(T, len(THR), 2)
    _accum(xd.data_ptr() + 4 * (T_in - 1) * H * W, T_in * H * W, 0, tgt, a, THR, scales, T)          # persistence: the last input frame, held
    held = xd[:, -1:].expand(B, T, H, W).contiguous().view(B * T, H, W)
    _accum_contig(held, tgt, b, THR, scales, T)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    want = F.ref_sums(t, held.cpu().numpy(), THR, SCALE, scales).reshape(B, T, 2, -1).sum(0)
    assert (a.view(T, 2, -1).cpu().numpy() == want).all()
    assert (want[..., 0::3] > 0).all() and (want[..., 1::3] > 0).all() and (want[..., 2::3] > 0).any(), "no event in a field: nothing is compared"


@pytest.mark.parametrize("H,W", [(37, 53), (32, 64)], ids=["odd", "even"])
def test_a_slice_of_a_wider_tensor_and_bases_off_by_one_float(H, W):
    B, T, scales = 2, 3, (1, 7, 33)
    t, p = R.radar_fields(B * T, H, W, 1)
    tgt, pred = _dev(t), _dev(p)
    want = _table(T, len(THR), 3)
    _accum_contig(pred, tgt, want, THR, scales, T)
    assert (want.view(T, 3, -1).cpu().numpy() == F.ref_sums(t, p, THR, SCALE, scales).reshape(B, T, 3, -1).sum(0)).all()
    # the forecast as frames 1..T of a (B, T + 2, H, W) tensor: a sample stride larger than T*H*W
    wide = torch.full((B, T + 2, H, W), 0.9, dtype=torch.float32, device=DEV)
    wide[:, 1:T + 1] = pred.view(B, T, H, W)
    got = _table(T, len(THR), 3)
    _accum(wide[:, 1:].data_ptr(), (T + 2) * H * W, H * W, tgt, got, THR, scales, T)
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)), "a slice of a wider tensor"
    # both fields one float into a buffer: 4-byte aligned only, so an even W too is read float by float
    hold_p, hold_t = (torch.zeros(B * T * H * W + 1, dtype=torch.float32, device=DEV) for _ in range(2))
    off_p, off_t = hold_p[1:].view(B * T, H, W), hold_t[1:].view(B * T, H, W)
    off_p.copy_(pred), off_t.copy_(tgt)
    assert off_p.data_ptr() % 16 == 4 and off_t.data_ptr() % 16 == 4 and pred.data_ptr() % 16 == 0 and tgt.data_ptr() % 16 == 0
    got = _table(T, len(THR), 3)
    _accum(off_p.data_ptr(), T * H * W, H * W, off_t, got, THR, scales, T)
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)), "bases one float off the 16-byte boundary"


# ------------------------------------------------------------------------------------------------ 5. non-finite inputs
def test_nan_never_exceeds_and_infinities_clip():
    n, H, W, scales = 4, 37, 53, (1, 5, 17, 33)
    t, p = (a[:n].copy() for a in _pair(6, H, W, 1))
    rng = np.random.default_rng(5)
    for a in (t, p):
        for value in (np.nan, np.inf, -np.inf):
            a.reshape(-1)[rng.choice(a.size, 40, replace=False)] = value
    t[0, :4, :4], p[0, :4, 4:8] = np.nan, np.nan          # whole windows of NaN: no event
    p[1, 8:12, 8:12], t[1, 20, 20] = -np.inf, np.inf
    t[2, 0, 0], p[2, H - 1, W - 1], t[3, H - 1, 0] = np.inf, np.inf, np.nan       # hand-placed at the frame's corners
    assert np.isnan(t).sum() > 40 and np.isinf(p).sum() > 40
    _check_exact(t, p, THR, scales)


# ------------------------------------------------------------------------------------------------ 6. workspace hygiene
def test_the_workspace_is_fully_written_and_nothing_behind_it_or_the_table_is():
    B, T, H, W, scales, n = 2, 3, 37, 53, (1, 9, 33), len(THR)
    t, p = R.radar_fields(B * T, H, W, 1)
    tgt, pred = _dev(t), _dev(p)
    nb = lib.query("adnm_valid_fss_accum_ws_bytes", B * T, T, H, W, n, lib.i64_table(list(scales)), len(scales))
    cells, guard = T * len(scales) * 3 * n, 64
    results = []
    for fill in (0x00, 0xFF):
        ws = torch.full((nb + guard,), fill, dtype=torch.uint8, device=DEV)
        ws[nb:] = 0xA5
        hold = torch.full((cells + 8,), -7.0, dtype=torch.float64, device=DEV)
        hold[:cells] = 0.0
        assert _accum(pred.data_ptr(), T * H * W, H * W, tgt, hold, THR, scales, T, ws=ws) == nb
        assert bool((ws[nb:] == 0xA5).all()), "a write behind ws_bytes"
        assert bool((hold[cells:] == -7.0).all()), "a write behind the table"
        results.append(hold[:cells].clone())
    assert torch.equal(results[0].view(torch.int64), results[1].view(torch.int64)), "the result depends on what the workspace held"
    assert (results[0].view(T, len(scales), -1).cpu().numpy() == F.ref_sums(t, p, THR, SCALE, scales).reshape(B, T, len(scales), -1).sum(0)).all()


# ------------------------------------------------------------------------------------------------ 7. the Validator end to end
def _model():
    from models.ADNMUNet import create_ADNMUNet
    m = create_ADNMUNet(5, 20, 6, img_size=64)
    recipe.fill_parameters(m)
    return m.to(DEV).eval()


def _drifting_samples(n, seed):
    """(n, 25, 64, 64): frame j of a sample is its blob field moved j pixels along x, scaled into the radar range (thresholds 20..40 of
    255): the target at frame index t is the last input frame displaced by t + 1 pixels"""
    rng = np.random.default_rng(seed)
    base = 0.45 * R.blobs(rng, n, 64, 64, 3) + rng.normal(0.0, 0.004, size=(n, 64, 64))
    return np.stack([np.roll(base, j, axis=2) for j in range(25)], axis=1).astype(np.float32)


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(((np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= 1e-12 * np.abs(b))).all())


def _check_fss(got, lead, rows, scales, what):
    """got: {n: {thr: float}}, lead: {n: {thr: length-T array}}; rows: (T, nscale, 3 * nthr) reference sums"""
    assert list(got) == list(scales) == list(lead)
    total, per = F.fss(rows.sum(axis=0)), F.fss(rows)
    for i, n in enumerate(scales):
        assert list(got[n]) == THR == list(lead[n])
        for k, thr in enumerate(THR):
            assert _close(got[n][thr], total[i, k]), (what, n, thr, got[n][thr], total[i, k])
            assert lead[n][thr].shape == (rows.shape[0],) and _close(lead[n][thr], per[:, i, k]), (what, "per lead", n, thr)


def test_validator_with_fss_pools_and_persistence_end_to_end():
    from adnm_hip.dataio import ResidentDataset
    from adnm_hip.validate import Validator, block_doubles, fss_doubles
    from models.loss import enRainfallLoss
    model, crit, scale, T = _model(), enRainfallLoss(0.57, 0.25, gamma=0.0), 255.0, 20
    pools, scales, n = ((4, 4), (16, 8)), (1, 5, 17), len(THR)      # (n = 33 through the Validator: the next test; the CPU reference of 120 frames is slow there)
    samples = _dev(_drifting_samples(6, 7))
    data = [(samples[i:i + 2, :5, None].contiguous(), samples[i:i + 2, 5:, None].contiguous()) for i in (0, 2, 4)]
    feed = ResidentDataset.from_frames(samples[4:6].contiguous(), 5, 2, DEV, shuffle=False)
    val = Validator(model, crit, T, scale, THR, pools=pools, persistence=True, fss=scales)
    plain = Validator(model, crit, T, scale, THR)
    try:
        def epoch():
            preds = []
            feed.begin_epoch()
            for x, tgt in data[:2]:
                preds.append(val.step(x, tgt).clone())
            preds.append(val.step_from(feed).clone())          # the third batch straight into the graph's static buffers
            return torch.cat(preds).reshape(6 * T, 64, 64).cpu().numpy()
        pred = epoch()
        block = val._block.cpu().numpy().copy()
        res = val.done(per_lead=True)
        short = val.done()
        for x, tgt in data:
            plain.step(x, tgt)
        old = plain.done(reset=True)
        # no existing behaviour moved: the shared keys are the plain Validator's, value for value
        assert set(short) == set(old) | {"pooled", "persistence", "fss", "fss_useful"} and set(res) == set(short) | {"per_lead"}
        assert repr({k: short[k] for k in old}) == repr(old) and repr({k: res[k] for k in short}) == repr(short)
        assert (res["batches"], res["samples"], res["nonfinite"]) == (3, 6, 0)
        # the reference, from the predictions step() returned and from the inputs
        tgt_all = samples[:, 5:].reshape(6 * T, 64, 64).cpu().numpy()
        held = samples[:, 4:5].expand(6, T, 64, 64).reshape(6 * T, 64, 64).cpu().numpy()
        f_ref = F.ref_sums(tgt_all, pred, THR, scale, scales).reshape(6, T, len(scales), -1).sum(0)        # (T, nscale, 3 nthr)
        b_ref = F.ref_sums(tgt_all, held, THR, scale, scales).reshape(6, T, len(scales), -1).sum(0)
        assert (b_ref[:, :, 0::3] > 0).all() and (b_ref[:, :, 1::3] > 0).all() and (b_ref[:, :, 2::3] > 0).any() and \
            (b_ref[:, :, 2::3] < b_ref[:, :, 0::3]).any(), "the baseline scores nothing or everything: the test is vacuous"
        assert (f_ref[:, :, 0::3] > 0).all(), "no observed event: the test is vacuous"
        # the sums behind the scores: the two tables at the end of the one allocation, integer for integer
        at = sum(block_doubles(T, n, pools, True))
        n3, n4 = fss_doubles(T, n, scales, True)
        assert block.shape == (at + n3 + n4,)
        assert (block[at:at + n3].reshape(f_ref.shape) == f_ref).all(), "the forecast's FSS table"
        assert (block[at + n3:].reshape(b_ref.shape) == b_ref).all(), "the baseline's FSS table"
        lead = res["per_lead"]
        _check_fss(res["fss"], lead["fss"], f_ref, scales, "forecast")
        _check_fss(res["persistence"]["fss"], lead["persistence"]["fss"], b_ref, scales, "persistence")
        # the useful-scale line from the main table's observed fraction
        assert list(res["fss_useful"]) == THR
        for thr in THR:
            m = res["threshold_metrics"][thr]
            f_o = (m["TP"] + m["FN"]) / (m["TP"] + m["FN"] + m["FP"] + m["TN"])
            assert m["TP"] + m["FN"] + m["FP"] + m["TN"] == 6 * T * 64 * 64 and _close(res["fss_useful"][thr], 0.5 + f_o / 2)
            # n = 1 is the point-wise score
            assert _close(res["fss"][1][thr], 2 * m["TP"] / (2 * m["TP"] + m["FN"] + m["FP"]))
        # holding the last input frame is a good forecast one frame ahead and a poor one twenty frames ahead; a larger window forgives more
        fss_lead = lead["persistence"]["fss"]
        print("persistence FSS per lead at 20, n = 1", fss_lead[1][20], "n = 17", fss_lead[17][20])
        assert fss_lead[1][20][0] > fss_lead[1][20][T - 1] and fss_lead[17][20][T - 1] > fss_lead[1][20][T - 1]
        # a second epoch replays the graph: the same bits
        val.done(reset=True)
        assert float(val._block.abs().sum()) == 0.0, "done(reset=True) left something in the block or the tables"
        assert (epoch() == pred).all()
        assert (val._block.cpu().numpy().view(np.int64) == block.view(np.int64)).all()
        assert repr(val.done(reset=True, per_lead=True)) == repr(res)
        # once the graph exists a step allocates nothing
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        val.step(*data[0])
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
    finally:
        val.close()
        plain.close()


def test_validator_with_fss_alone_and_the_plain_validator_allocates_nothing_new():
    from adnm_hip.validate import Validator, block_doubles
    from models.loss import RainfallLoss

    class LastFrames(torch.nn.Module):
        def forward(self, x):
            return x[:, -20:, 0].float() * 0.9

    t, p = _pair(*F.CASES[0])
    frames = torch.zeros(2, 25, 1, 64, 64, device=DEV)
    frames[:, 5:, 0] = _dev(np.concatenate([t, t, t, t, t])).view(2, 20, 64, 64)
    x, tgt = frames.clone(), frames[:, 5:].contiguous()
    val = Validator(LastFrames(), RainfallLoss(), 20, SCALE, THR, fss=(33,))
    plain = Validator(LastFrames(), RainfallLoss(), 20, SCALE, THR)
    try:
        val.step(x, tgt)
        plain.step(x, tgt)
        assert plain._block.numel() == block_doubles(20, len(THR))[0] and val._block.numel() == plain._block.numel() + 20 * 3 * len(THR)
        assert all(e.get("ws_fss") is None for e in plain._fwd._graphs.values())
        res, old = val.done(per_lead=True), plain.done(per_lead=True)
        assert set(res) == set(old) | {"fss", "fss_useful"} and "persistence" not in res and set(res["per_lead"]) == set(old["per_lead"]) | {"fss"}
        want = F.ref_sums(tgt.view(40, 64, 64).cpu().numpy(), (tgt.view(40, 64, 64) * 0.9).cpu().numpy(), THR, SCALE, (33,)).reshape(2, 20, 1, -1).sum(0)
        _check_fss(res["fss"], res["per_lead"]["fss"], want, (33,), "fss alone")
    finally:
        val.close()
        plain.close()
