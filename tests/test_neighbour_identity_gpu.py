"""The two neighbourhood scores share one tile stager (csrc/neighbour.hip: stage_pair_bits), so they are tied to each other here: a pool
of (1, 1) and an FSS scale of 1 look at single pixels, hence on the same pair, for every frame and threshold,
    A = TP + FN,   F = TP + FP,   C = TP,   TP + FN + FP + TN = H * W,
integer for integer.  Each shape runs alone with the identity rows and again with the largest pools and scales in the same calls, so that
the staged margin is at its widest while the identity is read off the same rows; and in two forms: a contiguous forecast through
ops.pool_counts / ops.fss_sums, and a held frame (pred_frame_stride = 0) read from a buffer one float in, which forces the scalar path.
The CPU yardsticks of the two scores are not rerun here: test_verify_gpu.py and test_fss_gpu.py do that."""
import ctypes

import numpy as np
import pytest
import torch

from adnm_hip import lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
THR, SCALE = [20.0, 30.0, 35.0, 40.0], 90.0
FRAMES, T = 4, 2
# 1 x 1: the identity rows only; 5 x 7: scalar path, one partial tile; 33 x 36: 16-byte path, a second tile of one row and four columns;
# 37 x 53: scalar path, four partial tiles; 64 x 64: 16-byte path, full tiles
SHAPES = [(1, 1), (5, 7), (33, 36), (37, 53), (64, 64)]
POOLS, SCALES = ((4, 4), (16, 8)), (5, 33)


def _fields(H, W):
    """(target, forecast) as float32 (FRAMES, H, W): about 90 % zeros, quantised values on both sides of every threshold, and NaN, +-Inf,
    a negative and a value above 1 planted in both"""
    rng = np.random.default_rng(1000 * H + W)

    def field():
        q = rng.integers(15, 46, (FRAMES, H, W))                        # thresholds 20 .. 40 lie inside
        return ((q + 0.5) / SCALE * (rng.random((FRAMES, H, W)) < 0.1)).astype(np.float32)
    tgt = field()
    pred = np.where(rng.random((FRAMES, H, W)) < 0.5, tgt, field())     # half of the forecast is the target: hits as well as misses
    n = tgt.size
    if n == FRAMES:      # 1 x 1, one pixel per frame: a hit, a miss and a false alarm in the contiguous and in the held form
        tgt.reshape(-1)[:] = (0.5, 0.4, 0.4, np.nan)
        pred.reshape(-1)[:] = (0.5, -0.5, np.inf, 1.5)
    else:
        for k, v in enumerate((np.nan, np.inf, -np.inf, -0.5, 1.5)):
            tgt.reshape(-1)[(7 * k) % n] = v
            pred.reshape(-1)[(11 * k + 3) % n] = v
    return [tgt, pred]


def _fitting(H, W):
    """the runs of a shape: the identity rows alone, then with every pool that fits the frame and the widest scales beside them"""
    if (H, W) == (1, 1):
        return [(((1, 1),), (1,))]
    return [(((1, 1),), (1,)), (((1, 1),) + tuple(p for p in POOLS if p[0] <= min(H, W)), (1,) + SCALES)]


def _check_identity(pool, fss, pixels, what):
    """pool: (rows, 4 * nthr) of the (1, 1) pool, fss: (rows, 3 * nthr) of scale 1, as int64"""
    tp, fn, fp, tn = (pool[:, j::4] for j in range(4))
    a, f, c = (fss[:, j::3] for j in range(3))
    assert (a == tp + fn).all() and (f == tp + fp).all() and (c == tp).all(), what
    assert (tp + fn + fp + tn == pixels).all(), what
    assert tp.sum() > 0 and fn.sum() > 0 and fp.sum() > 0, f"{what}: no event of some kind, nothing is compared"


def _exact_int(x):
    v = x.cpu().numpy()
    assert (v == np.rint(v)).all()
    return v.astype(np.int64)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_contiguous_pair(shape):
    H, W = shape
    tgt, pred = (torch.from_numpy(a).to(DEV) for a in _fields(H, W))
    first = None
    for pools, scales in _fitting(H, W):
        pool = _exact_int(ops.pool_counts(tgt, pred, THR, SCALE, pools))[:, 0]       # (frames, 4 * nthr)
        fss = _exact_int(ops.fss_sums(tgt, pred, THR, SCALE, scales))[:, 0]          # (frames, 3 * nthr)
        _check_identity(pool, fss, H * W, f"{H} x {W} pools {pools} scales {scales}")
        if first is None:
            first = (pool, fss)
        else:
            assert (pool == first[0]).all() and (fss == first[1]).all(), "the identity rows moved when wider windows were staged beside them"


def _accum(entry, block, pred_ptr, ss, fs, tgt, small, nsmall):
    """one direct call of a neighbourhood entry point with T = 2 -> its table as int64 (T, nsmall, cols)"""
    frames, H, W = tgt.shape
    thr = (ctypes.c_float * len(THR))(*THR)
    table = torch.zeros(lib.query(block, T, len(THR), nsmall) // 8, dtype=torch.float64, device=DEV)
    nb = lib.query(entry + "_ws_bytes", frames, T, H, W, len(THR), small, nsmall)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    lib.call(entry, pred_ptr, ss, fs, tgt.data_ptr(), table.data_ptr(), thr, len(THR), SCALE, small, nsmall, ws.data_ptr(), nb, frames, T, H, W,
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return _exact_int(table).reshape(T, nsmall, -1)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_held_frame_one_float_in(shape):
    """sample b's T frames are all the frame at buffer + 1 + b * H * W: 4-byte aligned only, frame stride 0"""
    H, W = shape
    hw, B = H * W, FRAMES // T
    t_np, p_np = _fields(H, W)
    tgt = torch.from_numpy(t_np).to(DEV)
    buf = torch.zeros(1 + B * hw, dtype=torch.float32, device=DEV)
    buf[1:] = torch.from_numpy(p_np[:B].reshape(-1)).to(DEV)
    held = buf[1:]
    assert held.data_ptr() % 16 == 4
    spread = held.view(B, 1, H, W).expand(B, T, H, W).reshape(FRAMES, H, W).contiguous()   # what the strides mean, written out
    first = None
    for pools, scales in _fitting(H, W):
        pool_all = _accum("adnm_valid_pool_accum", "adnm_valid_pool_block_bytes", held.data_ptr(), hw, 0, tgt, ops.pool_table(pools), len(pools))
        fss_all = _accum("adnm_valid_fss_accum", "adnm_valid_fss_block_bytes", held.data_ptr(), hw, 0, tgt, ops.fss_table(scales), len(scales))
        pool, fss = pool_all[:, 0], fss_all[:, 0]                                          # (T, 4 * nthr), (T, 3 * nthr): summed over the samples
        _check_identity(pool, fss, B * hw, f"held {H} x {W} pools {pools} scales {scales}")
        # the same numbers as the contiguous form gives on the written-out forecast, row t = the sum over the samples' frames b * T + t
        want_pool = _exact_int(ops.pool_counts(tgt, spread, THR, SCALE, pools)).reshape(B, T, len(pools), -1).sum(0)
        want_fss = _exact_int(ops.fss_sums(tgt, spread, THR, SCALE, scales)).reshape(B, T, len(scales), -1).sum(0)
        assert (pool_all == want_pool).all() and (fss_all == want_fss).all()
        if first is None:
            first = (pool, fss)
        else:
            assert (pool == first[0]).all() and (fss == first[1]).all(), "the identity rows moved when wider windows were staged beside them"
