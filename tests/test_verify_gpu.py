"""Pooled contingency counts on the GPU (csrc/neighbour.hip: adnm_valid_pool_accum; ops.pool_counts; Validator(pools=, persistence=)):
exact, integer for integer, against max_pool2d on the quantised fields on the CPU (verify_ref), against the point-wise kernel the
Validator already runs, and end to end through the captured graph."""
import ctypes

import numpy as np
import pytest
import torch

import verify_ref as R
from adnm_hip import lib, ops, recipe
from adnm_hip.evaluator import contingency_metrics

pytestmark = pytest.mark.gpu
DEV = "cuda"
THR, SCALE = R.THR, R.SCALE

# (frames, H, W, seed): the first three are DENSE (verify_ref.assert_dense holds for every pool used below at the default thresholds)
GENERAL = [(8, 64, 64, 1),       # two tiles a side; this seed's forecast leaves [0, 1] on both sides
           (6, 37, 53, 1),       # odd, no multiple of 4 (the float-by-float path), ragged at every pool, an edge tile 5 x 21
           (4, 128, 128, 0)]     # 16 tiles: windows of (16, 8) straddle every tile seam
POOL_SETS = {"point": ((1, 1),), "4-16": (4, 16), "mixed": ((4, 2), (16, 8), (3, 2), (1, 1))}
SPECIAL = [(1, 16, 16, 0, (16,)),         # one window
           (3, 5, 40, 0, ((5, 1),)),      # a frame one window high, two tiles wide
           (2, 33, 33, 0, ((32, 1),))]    # the largest window, four positions, each reaching 31 pixels past its origin

_fields = {}


def _pair(n, H, W, seed):
    """the CPU fields of a case, made once and never written to"""
    key = (n, H, W, seed)
    if key not in _fields:
        _fields[key] = R.radar_fields(n, H, W, seed)
    return _fields[key]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check_exact(t, p, thr, pools, dense=False):
    got = ops.pool_counts(_dev(t), _dev(p), thr, SCALE, pools)
    ref = R.ref_counts(t, p, thr, SCALE, pools)
    if dense:
        print("smallest cell of the reference", R.assert_dense(ref, f"{t.shape} {pools}"))
    assert got.dtype == torch.float64 and tuple(got.shape) == ref.shape
    got = got.cpu().numpy()
    assert (got == ref).all(), f"{int((got != ref).sum())} of {ref.size} cells differ from max_pool2d on the quantised fields"
    H, W = t.shape[-2:]
    for i, pool in enumerate(R.pairs(pools)):
        assert (got[:, i].reshape(len(t), len(thr), 4).sum(-1) == R.windows(H, W, pool)).all(), f"pool {pool}: the cells do not sum to the window count"
    return got


# ------------------------------------------------------------------------------------------------ 1. exact against the reference
@pytest.mark.parametrize("thr_name", list(R.THR_SETS))
@pytest.mark.parametrize("pool_name", list(POOL_SETS))
@pytest.mark.parametrize("case", GENERAL, ids=lambda c: "x".join(map(str, c[:3])))
def test_pool_counts_equal_max_pool2d(case, pool_name, thr_name):
    t, p = _pair(*case)
    _check_exact(t, p, R.THR_SETS[thr_name], POOL_SETS[pool_name], dense=thr_name == "default")


@pytest.mark.parametrize("thr_name", list(R.THR_SETS))
@pytest.mark.parametrize("case", SPECIAL, ids=lambda c: "x".join(map(str, c[:3])))
def test_pool_counts_at_the_window_limits(case, thr_name):
    t, p = _pair(*case[:4])
    got = _check_exact(t, p, R.THR_SETS[thr_name], case[4])
    assert got[..., :3].sum() > 0, "no event in this case: nothing is compared"


# ------------------------------------------------------------------------------------------------ the entry point, called directly
def _table(T, nthr, npool):
    return torch.zeros(lib.query("adnm_valid_pool_block_bytes", T, nthr, npool) // 8, dtype=torch.float64, device=DEV)


def _accum(pred_ptr, sample_stride, frame_stride, tgt, table, thr, pools, T):
    """tgt: contiguous (frames, H, W) on the device; the forecast by address and strides"""
    frames, H, W = tgt.shape
    pools = R.pairs(pools)
    tab = lib.i64_table([v for p in pools for v in p])
    nb = lib.query("adnm_valid_pool_accum_ws_bytes", frames, T, H, W, len(thr), tab, len(pools))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    lib.call("adnm_valid_pool_accum", pred_ptr, sample_stride, frame_stride, tgt.data_ptr(), table.data_ptr(), (ctypes.c_float * len(thr))(*thr), len(thr), SCALE,
             tab, len(pools), ws.data_ptr(), nb, frames, T, H, W, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def _accum_contig(pred, tgt, table, thr, pools, T):
    frames, H, W = tgt.shape
    assert pred.is_contiguous() and pred.shape == tgt.shape
    _accum(pred.data_ptr(), T * H * W, H * W, tgt, table, thr, pools, T)


# ------------------------------------------------------------------------------------------------ 2. the same as the kernel we have
def test_point_pool_equals_valid_accum_bit_for_bit():
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
        _accum_contig(p, t, table, THR, ((3, 1), (1, 1)), T)
    main = block[4:].view(T, 4 * n + 3)[:, :4 * n].contiguous()
    mine = table.view(T, 2, 4 * n)[:, 1].contiguous()
    assert float(main.sum()) == 2.0 * n * B * T * H * W and float(main[:, 0::4].sum()) > 0
    assert torch.equal(main.view(torch.int64), mine.view(torch.int64))


# ------------------------------------------------------------------------------------------------ 3. accumulation and mapping
def test_rows_are_frame_indices_and_batches_add():
    B, T, H, W, pools = 3, 4, 37, 53, ((4, 2), (16, 8), (1, 1))
    batches = [R.radar_fields(B * T, H, W, seed) for seed in (1, 2)]
    refs = [R.ref_counts(t, p, THR, SCALE, pools).reshape(B, T, len(pools), -1) for t, p in batches]
    assert not (refs[0].sum(0) == refs[0].reshape(T, B, len(pools), -1).sum(1)).all(), "f mod T and f / T coincide on this data: nothing is tested"
    tables = []
    for _ in range(2):
        table = _table(T, len(THR), len(pools))
        for i, (t, p) in enumerate(batches):
            _accum_contig(_dev(p), _dev(t), table, THR, pools, T)
            if not tables:
                want = sum(r.sum(0) for r in refs[:i + 1])      # row t: the reference summed over the samples, a second batch adds
                assert (table.view(T, len(pools), -1).cpu().numpy() == want).all(), f"after batch {i}"
        tables.append(table)
    assert torch.equal(tables[0].view(torch.int64), tables[1].view(torch.int64)), "the same calls on a fresh table give other bits"


# ------------------------------------------------------------------------------------------------ 4. addressing
def test_frame_stride_zero_is_the_expanded_copy():
    B, T, T_in, H, W, pools = 3, 4, 2, 37, 53, ((4, 2), (1, 1))
    t, x = R.radar_fields(B * T, H, W, 1)[0], R.radar_fields(B * T_in, H, W, 2)[1].reshape(B, T_in, H, W)
    tgt, xd = _dev(t), _dev(x)
    a, b = _table(T, len(THR), 2), _table(T, len(THR), 2)
    _accum(xd.data_ptr() + 4 * (T_in - 1) * H * W, T_in * H * W, 0, tgt, a, THR, pools, T)          # persistence: the last input frame, held
    held = xd[:, -1:].expand(B, T, H, W).contiguous().view(B * T, H, W)
    _accum_contig(held, tgt, b, THR, pools, T)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    want = R.ref_counts(t, held.cpu().numpy(), THR, SCALE, pools).reshape(B, T, 2, -1).sum(0)
    assert (a.view(T, 2, -1).cpu().numpy() == want).all() and want[:, :, 1].sum() > 0 and want[:, :, 2].sum() > 0


@pytest.mark.parametrize("H,W", [(37, 53), (32, 64)], ids=["odd", "even"])
def test_a_slice_of_a_wider_tensor_and_bases_off_by_one_float(H, W):
    B, T, pools = 2, 3, ((4, 2), (16, 8), (1, 1))
    t, p = R.radar_fields(B * T, H, W, 1)
    tgt, pred = _dev(t), _dev(p)
    want = _table(T, len(THR), 3)
    _accum_contig(pred, tgt, want, THR, pools, T)
    assert (want.view(T, 3, -1).cpu().numpy() == R.ref_counts(t, p, THR, SCALE, pools).reshape(B, T, 3, -1).sum(0)).all()
    # the forecast as frames 1..T of a (B, T + 2, H, W) tensor: a sample stride larger than T*H*W
    wide = torch.full((B, T + 2, H, W), 0.9, dtype=torch.float32, device=DEV)
    wide[:, 1:T + 1] = pred.view(B, T, H, W)
    got = _table(T, len(THR), 3)
    _accum(wide[:, 1:].data_ptr(), (T + 2) * H * W, H * W, tgt, got, THR, pools, T)
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)), "a slice of a wider tensor"
    # both fields one float into a buffer: 4-byte aligned only
    hold_p, hold_t = (torch.zeros(B * T * H * W + 1, dtype=torch.float32, device=DEV) for _ in range(2))
    off_p, off_t = hold_p[1:].view(B * T, H, W), hold_t[1:].view(B * T, H, W)
    off_p.copy_(pred), off_t.copy_(tgt)
    assert off_p.data_ptr() % 16 == 4 and off_t.data_ptr() % 16 == 4 and pred.data_ptr() % 16 == 0 and tgt.data_ptr() % 16 == 0
    got = _table(T, len(THR), 3)
    _accum(off_p.data_ptr(), T * H * W, H * W, off_t, got, THR, pools, T)
    assert torch.equal(got.view(torch.int64), want.view(torch.int64)), "bases one float off the 16-byte boundary"


# ------------------------------------------------------------------------------------------------ 5. the ragged edge
@pytest.mark.parametrize("pool", [(16, 16), (4, 2)], ids=["16", "4-2"])
def test_pixels_no_window_covers_take_no_part(pool):
    n, H, W = 6, 37, 53
    t, p = _pair(n, H, W, 1)
    s, d = pool
    ch, cw = ((H - s) // d) * d + s, ((W - s) // d) * d + s       # the covered rows and columns
    assert ch < H and cw < W
    t2, p2 = t.copy(), p.copy()
    for a in (t2, p2):
        a[:, ch:, :] = 1.0
        a[:, :, cw:] = 1.0
    base = ops.pool_counts(_dev(t), _dev(p), THR, SCALE, [pool])
    moved = ops.pool_counts(_dev(t2), _dev(p2), THR, SCALE, [pool, (1, 1)])
    assert torch.equal(base[:, 0].contiguous().view(torch.int64), moved[:, 0].contiguous().view(torch.int64)), "the counts moved"
    assert float(moved[:, 1, 0].sum()) >= n * (H * W - ch * cw), "the planted pixels are events of the point-wise count"
    assert (base.cpu().numpy() == R.ref_counts(t, p, THR, SCALE, [pool])).all()


# ------------------------------------------------------------------------------------------------ 6. non-finite inputs
def test_nan_never_exceeds_and_infinities_clip():
    n, H, W, pools = 4, 37, 53, ((4, 2), (16, 8), (3, 2), (1, 1))
    t, p = (a.copy() for a in _pair(6, H, W, 1))
    t, p = t[:n], p[:n]
    rng = np.random.default_rng(5)
    for a in (t, p):
        for value in (np.nan, np.inf, -np.inf):
            a.reshape(-1)[rng.choice(a.size, 40, replace=False)] = value
    t[0, :4, :4], p[0, :4, 4:8] = np.nan, np.nan          # whole windows of NaN: no event
    p[1, 8:12, 8:12], t[1, 20, 20] = -np.inf, np.inf
    assert np.isnan(t).sum() > 40 and np.isinf(p).sum() > 40
    _check_exact(t, p, THR, pools)


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
    return bool(((np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= 1e-12)).all())


def _check_scores(got, counts, what):
    """got: {"threshold_metrics", "FAR"} of done(); counts: (4 * nthr) reference counts"""
    m, far = contingency_metrics(counts, THR)
    for thr in THR:
        for k in ("TP", "FN", "FP", "TN"):
            assert got["threshold_metrics"][thr][k] == m[thr][k], (what, thr, k, got["threshold_metrics"][thr][k], m[thr][k])
        for k in ("CSI", "POD", "HSS"):
            assert _close(got["threshold_metrics"][thr][k], m[thr][k]), (what, thr, k)
    assert _close(got["FAR"], float(np.mean(far))), what


def _check_lead(got, rows, what):
    """got: {thr: {name: length-T array}}; rows: (T, 4 * nthr) reference counts"""
    m, far = contingency_metrics(rows.T, THR)
    for i, thr in enumerate(THR):
        for k in ("TP", "FN", "FP", "TN"):
            assert (got[thr][k] == m[thr][k]).all(), (what, thr, k)
        for k in ("CSI", "POD", "HSS"):
            assert _close(got[thr][k], m[thr][k]), (what, thr, k)
        assert _close(got[thr]["FAR"], far[i]), what


def test_validator_with_pools_and_persistence_end_to_end():
    from adnm_hip.dataio import ResidentDataset
    from adnm_hip.validate import Validator
    from models.loss import enRainfallLoss
    model, crit, scale, T = _model(), enRainfallLoss(0.57, 0.25, gamma=0.0), 255.0, 20
    pools = ((4, 4), (16, 16), (16, 8))
    base = ((1, 1),) + pools
    samples = _dev(_drifting_samples(6, 7))
    data = [(samples[i:i + 2, :5, None].contiguous(), samples[i:i + 2, 5:, None].contiguous()) for i in (0, 2, 4)]
    feed = ResidentDataset.from_frames(samples[4:6].contiguous(), 5, 2, DEV, shuffle=False)
    val = Validator(model, crit, T, scale, THR, pools=(4, 16, (16, 8)), persistence=True)
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
        res = val.done(per_lead=True)
        short = val.done()
        for x, tgt in data:
            plain.step(x, tgt)
        old = plain.done(reset=True)
        # no existing behaviour moved: the shared keys are the plain Validator's, value for value
        assert set(short) == set(old) | {"pooled", "persistence"} and set(res) == set(short) | {"per_lead"}
        assert repr({k: short[k] for k in old}) == repr(old) and repr({k: res[k] for k in short}) == repr(short)
        assert (res["batches"], res["samples"], res["nonfinite"]) == (3, 6, 0)
        # the reference, from the predictions step() returned and from the inputs
        tgt_all = samples[:, 5:].reshape(6 * T, 64, 64).cpu().numpy()
        held = samples[:, 4:5].expand(6, T, 64, 64).reshape(6 * T, 64, 64).cpu().numpy()
        f_ref = R.ref_counts(tgt_all, pred, THR, scale, base).reshape(6, T, len(base), -1).sum(0)        # (T, 1 + npool, 4 nthr), (1, 1) first
        b_ref = R.ref_counts(tgt_all, held, THR, scale, base).reshape(6, T, len(base), -1).sum(0)
        print("events (TP + FN at 20): forecast windows", f_ref[:, :, 0].sum(0) + f_ref[:, :, 1].sum(0), "persistence TP", b_ref[:, :, 0].sum(0))
        assert b_ref[:, :, 0].sum() > 0 and b_ref[:, :, 1].sum() > 0 and b_ref[:, :, 2].sum() > 0, "the baseline scores nothing: the test is vacuous"
        lead = res["per_lead"]
        _check_scores(res, f_ref[:, 0].sum(0), "point-wise")
        _check_lead(lead["threshold_metrics"], f_ref[:, 0], "per-lead point-wise")
        _check_scores(res["persistence"], b_ref[:, 0].sum(0), "persistence")
        _check_lead(lead["persistence"]["threshold_metrics"], b_ref[:, 0], "per-lead persistence")
        assert list(res["pooled"]) == list(pools) == list(res["persistence"]["pooled"])
        for i, p in enumerate(pools, start=1):
            _check_scores(res["pooled"][p], f_ref[:, i].sum(0), f"pooled {p}")
            _check_scores(res["persistence"]["pooled"][p], b_ref[:, i].sum(0), f"persistence pooled {p}")
            _check_lead(lead["pooled"][p]["threshold_metrics"], f_ref[:, i], f"per-lead pooled {p}")
            _check_lead(lead["persistence"]["pooled"][p]["threshold_metrics"], b_ref[:, i], f"per-lead persistence pooled {p}")
        assert lead["RMSE"].shape == lead["MAE"].shape == lead["SSIM"].shape == (T,)
        assert abs(float(np.mean(lead["RMSE"])) - res["RMSE"]) <= 1e-12 and abs(float(np.mean(lead["SSIM"])) - res["SSIM"]) <= 1e-12
        # holding the last input frame is a good forecast one frame ahead and a poor one twenty frames ahead
        csi = lead["persistence"]["threshold_metrics"][20]["CSI"]
        print("persistence CSI per lead at 20", csi)
        assert csi[0] >= csi[T - 1] and csi[0] > 0
        # a second epoch replays the graph: the same bits
        val.done(reset=True)
        assert float(val._block.abs().sum()) == 0.0, "done(reset=True) left something in the block or the pooled tables"
        assert (epoch() == pred).all()
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


def test_validator_refuses_what_the_pooled_pass_cannot_take():
    from adnm_hip.validate import Validator
    from models.loss import RainfallLoss
    x, tgt = torch.zeros(2, 20, 1, 16, 16, device=DEV) + 0.5, torch.zeros(2, 20, 1, 16, 16, device=DEV) + 0.5
    val = Validator(torch.nn.Identity(), RainfallLoss(), 20, 255.0, pools=(4, 32))
    with pytest.raises(RuntimeError, match="no window larger than the frame"):       # at the first batch of the shape, in open()
        val.step(x, tgt)
    val.close()

    class LastFrames(torch.nn.Module):
        def forward(self, x):
            return x[:, -20:].float()

    val = Validator(LastFrames(), RainfallLoss(), 20, 255.0, persistence=True)
    with pytest.raises(RuntimeError, match="persistence needs"):
        val.step(torch.zeros(2, 25, 1, 16, 16, device=DEV, dtype=torch.float64), tgt)
    with pytest.raises(RuntimeError, match="persistence needs"):
        val.step(torch.zeros(2, 25, 1, 16, 8, device=DEV), tgt)
    assert not torch.cuda.is_current_stream_capturing()
    # and the accepted case on the same object: a perfect forecast; persistence alone scores the baseline at (1, 1)
    val.step(torch.zeros(2, 25, 1, 16, 16, device=DEV) + 0.5, tgt)
    res = val.done()
    assert "pooled" not in res and res["persistence"]["pooled"] == {} and res["persistence"]["threshold_metrics"][20]["TP"] == 2 * 20 * 16 * 16
    val.close()
