"""The neighbourhood exceedance probability on the GPU (csrc/neighbour.hip: adnm_valid_nprob_accum, adnm_neighbour_prob; ops.neighbour_hist,
ops.neighbour_prob; Validator(nprob=); Forecaster(probability=)): the histogram integer for integer over the whole table against conv2d +
np.bincount on the CPU (nprob_ref), against the FSS, pooled and point-wise kernels it sits beside, and end to end through the captured
graphs; the probability field bit for bit against np.float32(c) / np.float32(n * n)."""
import ctypes

import numpy as np
import pytest
import torch

import nprob_ref as N
from adnm_hip import lib, ops
from util import poisoned_outputs, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALE = 90.0
THR = [20.0, 30.0, 35.0, 40.0]
THR_SETS = {"one": [30.0], "four": THR, "five": [10.0, 20.0, 30.0, 35.0, 40.0], "eight": [5.0, 10.0, 20.0, 30.0, 35.0, 40.0, 50.0, 70.0]}
SCALE_SETS = {"1": (1,), "3": (3,), "33": (33,), "1-5-17-33": (1, 5, 17, 33)}
SHAPES = [(1, 1), (5, 7), (31, 33), (32, 32), (33, 65), (40, 72)]   # tile edges; W % 4 both ways
WIDE = [(64, 64), (70, 70)]                                          # n = 33: the halo crosses tiles and the frame

_fields = {}


def _mixed(H, W):
    """the CPU fields of a shape, made once and never written to: two radar-like sparse frames with NaN, +-Inf, negatives and values > 1
    planted, one frame of noise at 0.1 and one at 0.5 -> (target, forecast), float32 (4, H, W)"""
    if (H, W) not in _fields:
        s, a, b = N.sparse_fields(2, H, W, 11), N.noise_fields(1, H, W, 12, 0.1), N.noise_fields(1, H, W, 13, 0.5)
        _fields[H, W] = tuple(np.concatenate([s[i], a[i], b[i]]) for i in range(2))
        for f in _fields[H, W]:
            f.setflags(write=False)
    return _fields[H, W]


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)      # (a copy: the cached fields are read-only)


def _check_exact(t, p, thr, scales):
    got = ops.neighbour_hist(_dev(t), _dev(p), thr, SCALE, scales)
    ref = N.frame_hist(t, p, thr, SCALE, scales)
    assert got.dtype == torch.int64 and tuple(got.shape) == ref.shape == (len(t), len(thr), ops.nprob_layout(scales)[1])
    got = got.cpu().numpy()
    assert (got == ref).all(), f"{int((got != ref).sum())} of {ref.size} bins differ from the bincount of the window counts"
    return got


# ------------------------------------------------------------------------------------------------ 1. exact against the yardstick
@pytest.mark.parametrize("scale_name", list(SCALE_SETS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_table_equals_the_bincount_of_the_window_counts(shape, scale_name):
    t, p = _mixed(*shape)
    got = _check_exact(t, p, THR, SCALE_SETS[scale_name])
    assert (got.sum(axis=2) == len(SCALE_SETS[scale_name]) * shape[0] * shape[1]).all(), "every pixel is counted once per scale"


@pytest.mark.parametrize("scale_name", ["33", "1-5-17-33"])
@pytest.mark.parametrize("shape", WIDE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_a_halo_that_crosses_tiles_and_the_frame(shape, scale_name):
    t, p = _mixed(*shape)
    got = _check_exact(t, p, THR, SCALE_SETS[scale_name])
    assert (got[:, 0, -1090 + 200:] > 0).any(), "no large count with an observed event: the upper bins are not reached"


@pytest.mark.parametrize("thr_name", list(THR_SETS))
@pytest.mark.parametrize("shape", [(33, 65), (40, 72)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_threshold_count_on_both_sides_of_the_nibble_switch(shape, thr_name):
    t, p = _mixed(*shape)
    got = _check_exact(t, p, THR_SETS[thr_name], (1, 5, 17, 33))
    assert len({got[:, k].tobytes() for k in range(got.shape[1])}) == got.shape[1], "two thresholds give one table: nothing distinguishes them"


def test_equal_and_shifted_forecasts():
    t, _ = _mixed(40, 72)
    got = _check_exact(t, t, THR, (1, 5))
    assert (got[:, :, 1] == 0).all() and (got[:, :, 2] == 0).all() and (got[:, :, 3] > 0).all(), "pred == target at scale 1: no miss, no false alarm"
    _check_exact(t, np.roll(t, 3, axis=2), THR, (1, 5, 33))


def test_all_zero_pairs_sit_in_the_ballot_bin_and_its_count_is_exact():
    for H, W in ((33, 65), (64, 64)):
        z = torch.zeros(3, H, W, device=DEV)
        got = ops.neighbour_hist(z, z, THR_SETS["eight"], SCALE, (1, 5, 17, 33)).cpu().numpy()
        offs, S = ops.nprob_layout((1, 5, 17, 33))
        want = np.zeros((3, 8, S), dtype=np.int64)
        for a0, _ in offs:
            want[:, :, a0] = H * W
        assert (got == want).all()


def test_all_event_pairs_reach_the_largest_count():
    """every pixel an event in both fields: the interior of a 70 x 70 frame has c = 33^2, the border the window clipped by the frame"""
    ones = np.ones((1, 70, 70), dtype=np.float32)
    got = _check_exact(ones, ones, [30.0], (33, 1))
    side = np.minimum(np.arange(70) + 17, 70) - np.maximum(np.arange(70) - 16, 0)
    want = np.bincount(np.outer(side, side).ravel(), minlength=1090)
    assert side.max() == 33 and want[1089] == 38 * 38
    assert (got[0, 0, :1090] == 0).all() and (got[0, 0, 1090:2180] == want).all() and list(got[0, 0, 2180:]) == [0, 0, 0, 4900]


# ------------------------------------------------------------------------------------------------ 2. beside the kernels we have
def test_cross_checks_against_fss_pool_and_point_wise_counts():
    t, p = _mixed(40, 72)
    scales = (1, 5, 17, 33)
    got = ops.neighbour_hist(_dev(t), _dev(p), THR, SCALE, scales).cpu().numpy()
    fss = ops.fss_sums(_dev(t), _dev(p), THR, SCALE, scales).cpu().numpy()                  # (frames, nscale, 3 nthr): A, F, C
    cells = ops.pool_counts(_dev(t), _dev(p), THR, SCALE, ((1, 1),)).cpu().numpy()[:, 0]      # (frames, 4 nthr): TP, FN, FP, TN
    assert cells.sum() == 4 * 4 * 40 * 72 and (cells[:, 0::4].sum(0) > 0).all()
    for i, ((a0, a1), n) in enumerate(zip(ops.nprob_layout(scales)[0], scales)):
        c = np.arange(n * n + 1)
        n0, n1 = got[:, :, a0:a0 + n * n + 1], got[:, :, a1:a1 + n * n + 1]
        assert (((n0 + n1) * c * c).sum(axis=2) == fss[:, i, 1::3]).all(), f"sum c^2 N is not FSS's F at n = {n}"
        assert (n1.sum(axis=2) == cells[:, 0::4] + cells[:, 1::4]).all(), f"sum N[1] is not TP + FN at n = {n}"
    one = got[:, :, :4]                                                                       # scale 1: [o = 0: c = 0, 1][o = 1: c = 0, 1]
    assert (one[:, :, 0] == cells[:, 3::4]).all() and (one[:, :, 1] == cells[:, 2::4]).all(), "TN, FP"
    assert (one[:, :, 2] == cells[:, 1::4]).all() and (one[:, :, 3] == cells[:, 0::4]).all(), "FN, TP"


# ------------------------------------------------------------------------------------------------ the entry point, called directly
def _table(T, nthr, scales, fill=0.0, guard=0):
    n = lib.query("adnm_valid_nprob_block_bytes", T, nthr, lib.i64_table(list(scales)), len(scales)) // 8
    assert n == T * nthr * ops.nprob_layout(scales)[1]
    return torch.full((n + guard,), fill, dtype=torch.float64, device=DEV)


def _accum(pred_ptr, sample_stride, frame_stride, tgt, table, thr, scales, T, override=()):
    """tgt: contiguous (frames, H, W) on the device; the forecast by address and strides; override: arguments replaced by name"""
    frames, H, W = tgt.shape
    tab = lib.i64_table(list(scales))
    assert lib.query("adnm_valid_nprob_accum_ws_bytes", frames, T, H, W, len(thr), tab, len(scales)) == 0, "no workspace is used"
    args = dict(pred=pred_ptr, ss=sample_stride, fs=frame_stride, tgt=tgt.data_ptr(), table=table.data_ptr(), thr=(ctypes.c_float * len(thr))(*thr), nthr=len(thr),
                tab=tab, ns=len(scales))
    args.update(override)
    lib.call("adnm_valid_nprob_accum", args["pred"], args["ss"], args["fs"], args["tgt"], args["table"], args["thr"], args["nthr"], SCALE, args["tab"], args["ns"],
             None, 0, frames, T, H, W, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def test_rows_are_frame_indices_batches_add_and_two_runs_give_the_same_bits():
    B, T, H, W, scales = 2, 3, 37, 53, (1, 9, 33)            # frames = 6, T = 3
    S = ops.nprob_layout(scales)[1]
    batches = [N.sparse_fields(B * T, H, W, seed) for seed in (1, 2)]
    refs = [N.frame_hist(t, p, THR, SCALE, scales).reshape(B, T, len(THR), S) for t, p in batches]
    assert not (refs[0].sum(0) == refs[0].reshape(T, B, len(THR), S).sum(1)).all(), "f mod T and f / T coincide on this data: nothing is tested"
    tables = []
    for _ in range(2):
        table = _table(T, len(THR), scales, fill=5.0, guard=8)   # the table is ADDED to: it starts at 5 everywhere
        table[-8:] = -7.0
        for i, (t, p) in enumerate(batches):
            pred, tgt = _dev(p), _dev(t)
            _accum(pred.data_ptr(), T * H * W, H * W, tgt, table, THR, scales, T)
            want = 5 + sum(r.sum(0) for r in refs[:i + 1])
            assert (table[:-8].view(T, len(THR), S).cpu().numpy() == want).all(), f"after batch {i}"
        assert bool((table[-8:] == -7.0).all()), "a write behind the table"
        tables.append(table)
    assert torch.equal(tables[0].view(torch.int64), tables[1].view(torch.int64)), "the same calls on a fresh table give other bits"


def test_frame_stride_zero_is_the_expanded_copy():
    B, T, T_in, H, W, scales = 3, 4, 2, 37, 53, (5, 1)
    t, x = N.sparse_fields(B * T, H, W, 1)[0], N.sparse_fields(B * T_in, H, W, 2)[1].reshape(B, T_in, H, W)
    tgt, xd = _dev(t), _dev(x)
    a, b = _table(T, len(THR), scales), _table(T, len(THR), scales)
    _accum(xd.data_ptr() + 4 * (T_in - 1) * H * W, T_in * H * W, 0, tgt, a, THR, scales, T)          # the last input frame, held
    held = xd[:, -1:].expand(B, T, H, W).contiguous().view(B * T, H, W)
    _accum(held.data_ptr(), T * H * W, H * W, tgt, b, THR, scales, T)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    want = N.table(t, held.cpu().numpy(), THR, SCALE, scales, T)
    assert (a.view(want.shape).cpu().numpy() == want).all() and (want[:, :, 6:] > 0).any()


@pytest.mark.parametrize("H,W", [(37, 53), (32, 64)], ids=["odd", "even"])
def test_a_slice_of_a_wider_tensor_and_bases_off_by_one_float(H, W):
    B, T, scales = 2, 3, (1, 7, 33)
    t, p = N.sparse_fields(B * T, H, W, 1)
    tgt, pred = _dev(t), _dev(p)
    want = _table(T, len(THR), scales)
    _accum(pred.data_ptr(), T * H * W, H * W, tgt, want, THR, scales, T)
    ref = N.table(t, p, THR, SCALE, scales, T)
    assert (want.view(ref.shape).cpu().numpy() == ref).all()
    wide = torch.full((B, T + 2, H, W), 0.9, dtype=torch.float32, device=DEV)      # frames 1..T of a (B, T + 2, H, W) tensor
    wide[:, 1:T + 1] = pred.view(B, T, H, W)
    got = _table(T, len(THR), scales)
    _accum(wide[:, 1:].data_ptr(), (T + 2) * H * W, H * W, tgt, got, THR, scales, T)
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)), "a slice of a wider tensor"
    hold_p, hold_t = (torch.zeros(B * T * H * W + 1, dtype=torch.float32, device=DEV) for _ in range(2))   # 4-byte aligned only: the scalar path
    off_p, off_t = hold_p[1:].view(B * T, H, W), hold_t[1:].view(B * T, H, W)
    off_p.copy_(pred), off_t.copy_(tgt)
    assert off_p.data_ptr() % 16 == 4 and off_t.data_ptr() % 16 == 4 and pred.data_ptr() % 16 == 0 and tgt.data_ptr() % 16 == 0
    got = _table(T, len(THR), scales)
    _accum(off_p.data_ptr(), T * H * W, H * W, off_t, got, THR, scales, T)
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)), "bases one float off the 16-byte boundary"


def test_the_host_refusals_leave_the_table_alone():
    T, H, W, scales = 3, 16, 16, (1, 5)
    tgt, pred = torch.zeros(T, H, W, device=DEV), torch.zeros(T, H, W, device=DEV)
    table = _table(T, len(THR), scales, fill=3.0)
    base = dict(pred_ptr=pred.data_ptr(), sample_stride=T * H * W, frame_stride=H * W)
    for kw, text in [(dict(pred=None), "null pointer"), (dict(table=None), "null pointer"), (dict(thr=None), "null pointer"), (dict(tab=None), "null pointer"),
                     (dict(table=table.data_ptr() + 4), "8-byte aligned"), (dict(pred=pred.data_ptr() + 2), "4-byte aligned"),
                     (dict(fs=H * W - 1), "pred_frame_stride"), (dict(ss=-1), "pred_sample_stride"),
                     (dict(tab=lib.i64_table([1, 4])), "odd and in 1..33"), (dict(tab=lib.i64_table([35, 1])), "odd and in 1..33"),
                     (dict(tab=lib.i64_table([5, 5])), "given twice"), (dict(ns=0), "1..4 scales"), (dict(nthr=9), "1..8 thresholds")]:
        with pytest.raises(RuntimeError, match="valid_nprob_accum") as e:
            _accum(base["pred_ptr"], base["sample_stride"], base["frame_stride"], tgt, table, THR, scales, T, override=kw)
        assert text in str(e.value), (kw, str(e.value))
    torch.cuda.synchronize()
    assert bool((table == 3.0).all())
    for bad in ((2,), (35,), (5, 5), (1, 3, 5, 7, 9)):
        with pytest.raises(ValueError):
            ops.neighbour_hist(tgt, pred, THR, SCALE, bad)
    with pytest.raises(RuntimeError):
        ops.neighbour_hist(tgt.cpu(), pred.cpu(), THR, SCALE, (1,))


# ------------------------------------------------------------------------------------------------ 3. the probability field
def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("scale", [1, 3, 9, 33])
@pytest.mark.parametrize("shape", SHAPES + WIDE[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_probability_field_bit_for_bit_and_every_element_written(monkeypatch, shape, scale):
    """B = 2, T = 2 of the mixed frames; five thresholds: both nibbles.  Under both fill patterns no element of the output keeps its pattern."""
    H, W = shape
    field = _mixed(H, W)[1].reshape(2, 2, H, W)
    thr = THR_SETS["five"]
    want = N.prob(field.reshape(4, H, W), thr, SCALE, scale).reshape(5, 2, 2, H, W)
    assert want.dtype == np.float32
    x, runs, records = _dev(field), [], []
    for pattern in (0, 1):
        with poisoned_outputs(monkeypatch, pattern) as po:
            runs.append(ops.neighbour_prob(x, thr, SCALE, scale))
        records.append(po.records)
    torch.cuda.synchronize()
    assert unwritten(records[0], records[1]) == {}, "an output element nobody wrote"
    assert any(r[2] == "out" and tuple(r[0].shape) == (5, 2, 2, H, W) for r in records[0]), "the output was not among the allocations"
    for got in runs:
        assert got.dtype == torch.float32 and got.is_contiguous()
        assert (_bits(got.cpu().numpy()) == _bits(want)).all(), "not np.float32(c) / np.float32(n * n)"
    five = ops.neighbour_prob(x[:, :, None], thr, SCALE, scale)                # (B, T, 1, H, W)
    assert torch.equal(five, runs[0])


def test_every_count_divides_as_numpy_divides():
    """5 x 218 blocks of 33 x 33 pixels, block b holding exactly b events: the window centred on a block's centre is the block, so every
    c = 0 .. 1089 is divided at least once; and an all-event frame clipped by its border gives the products a * b, a, b <= 33"""
    n, rows, cols = 33, 5, 218
    f = np.zeros((rows * n, cols * n), dtype=np.float32)
    for b in range(n * n + 1):
        blk = np.zeros(n * n, dtype=np.float32)
        blk[:b] = 0.5
        y0, x0 = (b // cols) * n, (b % cols) * n
        f[y0:y0 + n, x0:x0 + n] = np.random.default_rng(b).permutation(blk).reshape(n, n)
    want = N.prob(f[None], [20.0], SCALE, n)
    centres = np.rint(want[0, 0, 16::n, 16::n] * n * n).astype(np.int64).ravel()
    assert (centres == np.arange(rows * cols)).all() and np.unique(np.rint(want * n * n)).size == n * n + 1, "not every count occurs"
    got = ops.neighbour_prob(_dev(f[None, None]), [20.0], SCALE, n).cpu().numpy().reshape(want.shape)
    assert (_bits(got) == _bits(want)).all()
    ones = np.ones((1, 1, 70, 70), dtype=np.float32)
    got = ops.neighbour_prob(_dev(ones), [20.0], SCALE, n).cpu().numpy()[0, 0, 0]
    side = np.minimum(np.arange(70) + 17, 70) - np.maximum(np.arange(70) - 16, 0)
    assert (_bits(got) == _bits(np.outer(side, side).astype(np.float32) / np.float32(n * n))).all() and got.max() == 1.0


@pytest.mark.parametrize("H,W", [(33, 65), (40, 72)], ids=["odd", "even"])
def test_unaligned_input_and_output_give_the_same_bits(H, W):
    """a 4-byte aligned output (scalar stores at an even W too), a 4-byte aligned input (scalar loads), both; nothing beside the output is written"""
    thr, scale = THR_SETS["eight"], 17
    field = _dev(_mixed(H, W)[1])
    want = ops.neighbour_prob(field.view(2, 2, H, W), thr, SCALE, scale).view(8, 4, H, W)
    assert (_bits(want.cpu().numpy()) == _bits(N.prob(_mixed(H, W)[1], thr, SCALE, scale))).all()
    thr_c = (ctypes.c_float * 8)(*thr)
    hold_in = torch.zeros(field.numel() + 1, dtype=torch.float32, device=DEV)
    off_in = hold_in[1:].view(4, H, W)
    off_in.copy_(field)
    for src in (field, off_in):
        for shift in (0, 1):
            hold = torch.full((want.numel() + 2,), -7.0, dtype=torch.float32, device=DEV)
            out = hold[shift:shift + want.numel()].view(8, 4, H, W)
            assert out.data_ptr() % 16 == 4 * shift and src.data_ptr() % 16 in (0, 4)
            ops.neighbour_prob_into(src, out, thr_c, 8, SCALE, scale)
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (src is field, shift)
            assert bool((hold[:shift] == -7.0).all()) and bool((hold[shift + want.numel():] == -7.0).all()), "a write beside the output"


def test_the_probability_op_refuses():
    x = torch.zeros(1, 2, 8, 8, device=DEV)
    for bad in (4, 35, (3, 5), ()):
        with pytest.raises(ValueError):
            ops.neighbour_prob(x, THR, SCALE, bad)
    with pytest.raises(ValueError):
        ops.neighbour_prob(x, [], SCALE, 3)
    with pytest.raises(ValueError):
        ops.neighbour_prob(x, range(9), SCALE, 3)
    with pytest.raises(RuntimeError):
        ops.neighbour_prob(x.cpu(), THR, SCALE, 3)
    with pytest.raises(RuntimeError):
        ops.neighbour_prob(x[0], THR, SCALE, 3)


# ------------------------------------------------------------------------------------------------ 4. the Validator end to end
class Drift(torch.nn.Module):
    """a stand-in forecast: the last input frame, moved one more pixel to the right and weakened with every lead"""
    def forward(self, x):
        last = x[:, -1, 0].float()
        return torch.stack([torch.roll(last, t + 1, dims=-1) * (1.0 - 0.15 * t) for t in range(3)], dim=1)


def _same_tree(a, b):
    """bitwise: dictionaries key for key in order, arrays and numbers value for value with NaN equal to NaN"""
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same_tree(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is b
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(((a == b) | ((a != a) & (b != b))).all())


def test_validator_with_nprob_beside_the_other_tables():
    from adnm_hip.validate import Validator, nprob_doubles, nprob_entries
    from models.loss import RainfallLoss
    B, T, H, W, thr, scales = 2, 3, 32, 32, [20.0, 30.0], (1, 5, 33)
    seq = N.sparse_fields(2 * B * 5, H, W, 131, plant=False)[0].reshape(2, B, 5, 1, H, W) * 0.7
    data = [(_dev(seq[i, :, :2]), _dev(seq[i, :, 2:])) for i in range(2)]
    kw = dict(fss=scales, joint=True, objects=2, sal=True)
    val = Validator(Drift(), RainfallLoss(), T, SCALE, thr, nprob=True, **kw)
    former = Validator(Drift(), RainfallLoss(), T, SCALE, thr, **kw)
    plain = Validator(Drift(), RainfallLoss(), T, SCALE, thr)
    try:
        n, S = nprob_doubles(T, len(thr), scales), ops.nprob_layout(scales)[1]
        assert n == T * len(thr) * S and val.nprob == scales and former.nprob == ()
        want, batches = np.zeros((T, len(thr), S), dtype=np.int64), []
        for x, tgt in data:            # two steps through the captured graph
            out = val.step(x, tgt)
            rows = ops.neighbour_hist(tgt.view(B * T, H, W), out.view(B * T, H, W).contiguous(), thr, SCALE, scales).cpu().numpy()
            assert (rows == N.frame_hist(tgt.cpu().numpy().reshape(B * T, H, W), out.cpu().numpy().reshape(B * T, H, W), thr, SCALE, scales)).all()
            batches.append(rows.reshape(B, T, len(thr), S).sum(axis=0))     # summed per frame index
            want += batches[-1]
            former.step(x, tgt)
            plain.step(x, tgt)
        assert (want[:, :, 5:].sum(axis=(0, 2)) > 0).all(), "no window with an event: nothing is tested"
        assert val._block.numel() == former._block.numel() + n
        got = val._block[-n:].cpu().numpy().reshape(T, len(thr), S)
        assert (got == want).all() and (got.view(np.int64) == want.astype(np.float64).view(np.int64)).all(), "the table is not the op's rows summed per frame index"
        assert torch.equal(val._block[:-n].view(torch.int64), former._block.view(torch.int64)), "a former offset moved, or a former pass counts differently"
        res, old = val.done(per_lead=True), former.done(per_lead=True)
        assert "nprob" not in old and "nprob" not in old["per_lead"]
        assert list(res) == list(old)[:-1] + ["nprob", "per_lead"] and list(res["per_lead"]) == list(old["per_lead"]) + ["nprob"]
        assert _same_tree({k: res[k] for k in old if k != "per_lead"}, {k: old[k] for k in old if k != "per_lead"}), "a former entry moved"
        assert _same_tree({k: res["per_lead"][k] for k in old["per_lead"]}, old["per_lead"]), "a former per-lead entry moved"
        assert _same_tree(res["nprob"], nprob_entries(want.sum(axis=0), scales, thr)) and _same_tree(res["per_lead"]["nprob"], nprob_entries(want, scales, thr))
        e = res["nprob"][5][20]
        assert e["histogram"].sum() == 2 * B * T * H * W and 0.0 < e["base_rate"] < 1.0 and 0.0 <= e["roc_area"] <= 1.0
        assert abs(e["brier"] - (e["reliability"] - e["resolution"] + e["uncertainty"])) <= 1e-12
        print("nprob end to end, n = 5, threshold 20:", {k: e[k] for k in ("base_rate", "brier", "reliability", "resolution", "uncertainty", "brier_skill", "roc_area")})
        # with every new argument at its default nothing is new: the keys and the block are the plain Validator's
        basic = plain.done(per_lead=True)
        assert list(basic) == ["threshold_metrics", "FAR", "RMSE", "MAE", "MSE", "SSIM", "LPIPS", "loss_sum", "loss_mean", "batches", "samples", "nonfinite", "per_lead"]
        assert list(basic["per_lead"]) == ["RMSE", "MAE", "SSIM", "threshold_metrics"]
        assert plain._block.numel() == 4 + T * (4 * len(thr) + 3) == lib.query("adnm_valid_block_bytes", T, len(thr)) // 8
        # a second epoch after done(reset=True) starts from zero: it holds the second batch alone
        val.done(reset=True)
        assert float(val._block.abs().sum()) == 0.0, "done(reset=True) left something in the block"
        val.step(*data[1])
        assert (val._block[-n:].cpu().numpy().reshape(T, len(thr), S) == batches[1]).all(), "a batch depends on the one before"
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        val.step(*data[0])
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before, "a replay allocated"
    finally:
        val.close()
        former.close()
        plain.close()


# ------------------------------------------------------------------------------------------------ 5. the Forecaster
class Spread(torch.nn.Module):
    """a stand-in model: three output frames from the last input frame, (B, 3, 1, H, W)"""
    def forward(self, x):
        last = x[:, -1].float()
        return torch.stack([torch.roll(last, 2 * t, dims=-1) * (1.0 - 0.2 * t) for t in range(3)], dim=1)


def test_forecaster_probability_is_the_op_on_its_forecast():
    from adnm_hip.forecast import Forecaster, Palette
    pal = Palette([0.0, 0.25, 0.5, 0.75, 1.01], np.array([[0, 0, 0, 0], [0, 0, 255, 255], [0, 255, 0, 255], [255, 0, 0, 255]], dtype=np.uint8))
    xs = [_dev(N.sparse_fields(2 * 5, 64, 64, seed, plant=False)[0].reshape(2, 5, 1, 64, 64)) for seed in (3, 4)]
    fc = Forecaster(Spread(), pal, pixel_scale=SCALE, probability=dict(thresholds=(20, 40), scale=9))
    plain = Forecaster(Spread(), pal, pixel_scale=SCALE)
    try:
        seen = []
        for x in xs + xs[:1]:
            res = fc(x)
            assert res.prob.dtype == torch.float32 and tuple(res.prob.shape) == (2, 2, 3, 64, 64) and res.prob[1].is_contiguous()
            want = ops.neighbour_prob(res.pred, (20, 40), SCALE, 9)
            assert torch.equal(res.prob.view(torch.int32), want.view(torch.int32))
            assert (_bits(want.cpu().numpy()) == _bits(N.prob(res.pred.cpu().numpy().reshape(6, 64, 64), [20.0, 40.0], SCALE, 9).reshape(2, 2, 3, 64, 64))).all()
            assert 0.0 < float(res.prob.max()) <= 1.0 and float(res.prob[0].sum()) > float(res.prob[1].sum()) > 0.0
            seen.append(res.prob.clone())
            old = plain(x)
            assert old.prob is None and torch.equal(old.fields, res.fields) and torch.equal(old.strip, res.strip) and torch.equal(old.pred, res.pred)
        assert not torch.equal(seen[0], seen[1]) and torch.equal(seen[0], seen[2]) and fc(xs[0]).prob.data_ptr() == fc(xs[1]).prob.data_ptr()
        assert all(e.get("prob") is None for e in plain._fwd._graphs.values()), "the plain Forecaster allocated a probability buffer"
        # prob[k] is a (B, T, H, W) field in [0, 1]: the render colours it with no pixel scale (the float itself is binned)
        fields, strip = ops.forecast_render(fc(xs[0]).prob[0], pal.edges, pal.colours, 0.0, gap=0)
        assert tuple(fields.shape) == (2, 3, 64, 64) and int(fields.max()) == 3
    finally:
        fc.close()
        plain.close()
