"""Connected-component labelling and the object scores on the GPU (csrc/objects.hip: adnm_valid_objects_accum, adnm_label_objects;
ops.object_stats, ops.label_objects; Validator(objects=)) against scipy.ndimage.label on the CPU (objects_ref).  Every comparison is integer
for integer and, for the labels, pixel for pixel; there is no tolerance anywhere.  Frames of 192 x 200 are the largest whose words live in
LDS, 200 x 200 the first that use the workspace, 256 x 256 the limit."""
import ctypes

import numpy as np
import pytest
import torch

import objects_ref as R
from adnm_hip import lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALE, HALF = 90.0, (45.0,)
SIZES = [(1, 1), (1, 7), (5, 3), (16, 16), (31, 33), (64, 64), (128, 128), (192, 200), (200, 200), (256, 256)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _shift(a, dy, dx):
    """the field moved by (dy, dx) >= 0, zeros coming in"""
    out = np.zeros_like(a)
    H, W = a.shape[-2:]
    out[..., dy:, dx:] = a[..., :H - dy, :W - dx]
    return out


def _check(t, p, thr=HALF, scale=SCALE, min_area=1, labels=True):
    """(frames, H, W) numpy fields: the statistics of both fields integer for integer, the labels of both pixel for pixel -> the statistics"""
    t, p = np.asarray(t, dtype=np.float32), np.asarray(p, dtype=np.float32)
    td, pd = _dev(t), _dev(p)
    got = ops.object_stats(td, pd, thr, scale, min_area)
    assert got.dtype == torch.int64 and tuple(got.shape) == (t.shape[0], 2, len(thr), 23) and got.device.type == "cuda"
    got = got.cpu().numpy()
    want = R.frame_stats(t, p, thr, scale, min_area)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"(frame, field, threshold, column) {bad[:8].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
    if labels:
        for v in thr:
            for name, host, dev in (("target", t, td), ("forecast", p, pd)):
                lab = ops.label_objects(dev, v, scale, min_area)
                assert lab.dtype == torch.int32 and lab.shape == dev.shape
                assert (lab.cpu().numpy() == R.label_field(host, v, scale, min_area)).all(), f"labels of the {name} at {v}"
    return got


def _pattern(name, H, W):
    if name == "empty":
        return np.zeros((H, W), dtype=np.float32)
    if name == "full":
        return np.ones((H, W), dtype=np.float32)
    if name == "diagonal":
        return np.eye(H, W, dtype=np.float32)
    return getattr(R, name)(H, W)


# ------------------------------------------------------------------------------------------------ 1. sizes and patterns
@pytest.mark.parametrize("name", ["empty", "full", "checkerboard", "lattice", "diagonal", "comb", "serpentine"])
@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
def test_patterns_at_every_size(H, W, name):
    """one frame; the forecast is the pattern one pixel down and two to the right"""
    t = _pattern(name, H, W)[None]
    got = _check(t, _shift(t, min(1, H - 1), min(2, W - 1)))[0, 0, 0]
    if name == "empty":
        assert (got == 0).all()
    if name == "full":
        assert got[:4].tolist() == [1, H * W, (H * W) ** 2, H * W] and got[6 + int(np.log2(H * W))] == 1
        if (H, W) == (256, 256):
            assert got[6 + 16] == 1 and got[2] == 1 << 32, "the last bin and the largest addend"
    if name == "lattice":
        assert got[0] == got[1] == ((H + 1) // 2) * ((W + 1) // 2) == got[6], "the most objects a frame can hold"
    if name in ("comb", "serpentine", "diagonal") or (name == "checkerboard" and min(H, W) > 1):
        assert got[0] == 1, "one object under 8-connectivity"


@pytest.mark.parametrize("n", [32, 128, 256])
def test_a_spiral_is_one_object(n):
    t = R.spiral(n)[None]
    got = _check(t, t[:, ::-1].copy())
    assert got[0, :, 0, 0].tolist() == [1, 1] and got[0, 0, 0, 1] == int(t.sum())


def test_a_frame_above_the_limit_raises():
    z = torch.zeros(1, 257, 256, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="65536"):
        ops.object_stats(z, z, HALF, SCALE)
    with pytest.raises(RuntimeError, match="65536"):
        ops.label_objects(z, 45.0, SCALE)
    with pytest.raises(ValueError, match="min_area"):
        ops.object_stats(z[:, :8, :8].contiguous(), z[:, :8, :8].contiguous(), HALF, SCALE, min_area=0)


# ------------------------------------------------------------------------------------------------ 2. tangled shapes
@pytest.mark.parametrize("density", [0.1, 0.41, 0.6])
@pytest.mark.parametrize("H,W", [(31, 33), (128, 128), (200, 200)], ids=lambda v: str(v))
def test_uniform_noise_around_the_percolation_point(H, W, density):
    t = np.stack([R.noise(H, W, density, 11), R.noise(H, W, density, 12)])
    p = np.stack([R.noise(H, W, density, 13), _shift(t[1], 0, 1)])
    got = _check(t, p)
    assert got[:, :, 0, 0].min() >= 1 and abs(got[0, 0, 0, 1] / (H * W) - density) < 0.05


def test_a_radar_like_field_with_planted_values_at_four_thresholds():
    """NaN, +-Inf, negatives and values > 1 planted; threshold 0 makes every pixel an event, 91 none"""
    thr = (0.0, 20.0, 40.0, 91.0)
    t, p = R.radar(2, 64, 64, 31, plant=True), R.radar(2, 64, 64, 32, plant=True)
    assert np.isnan(t).any() and np.isinf(p).any() and (t < 0).any() and (p > 1).any() and 0.85 < (t == 0).mean() < 0.95
    got = _check(t, p, thr)
    assert (got[:, :, 0, :4] == [1, 4096, 4096 ** 2, 4096]).all() and (got[:, :, 0, 4:6] == [1, 4096]).all(), "threshold 0: one object, matched"
    assert (got[:, :, 3] == 0).all(), "nothing reaches 91"
    assert (got[:, :, 1, 0] >= 1).all()
    _check(t, p, (20.0, 35.5), 89.5)          # a fractional scale and a fractional threshold


def test_a_late_merge_at_an_odd_size():
    t = np.stack([R.comb(37, 45), R.comb(37, 45)[::-1].copy()])          # merged in the last row, and in the first
    _check(t, np.stack([R.serpentine(37, 45), R.checkerboard(37, 45)]))


# ------------------------------------------------------------------------------------------------ 3. min_area
@pytest.mark.parametrize("min_area", [1, 2, 9, 11])
def test_min_area_drops_small_objects_from_every_column(min_area):
    f = np.zeros((1, 24, 24), dtype=np.float32)
    f[0, 1, 1] = 1                      # area 1
    f[0, 4, 2:10] = 1                   # area 8
    f[0, 8:11, 3:6] = 1                 # area 9
    f[0, 14:16, 2:7] = 1                # area 10
    other = np.zeros_like(f)
    other[0, 1, 1] = other[0, 9, 4] = other[0, 15, 6] = 1          # touches the objects of area 1, 9 and 10
    got = _check(f, other, min_area=min_area)[0, 0, 0]
    areas = [a for a in (1, 8, 9, 10) if a >= min_area]
    matched = [a for a in (1, 9, 10) if a >= min_area]
    assert got[:6].tolist() == [len(areas), sum(areas), sum(a * a for a in areas), max(areas, default=0), len(matched), sum(matched)]
    assert got[6:10].tolist() == [int(1 in areas), 0, 0, len([a for a in areas if a >= 8])]


# ------------------------------------------------------------------------------------------------ 4. matching
def test_matching_equal_shifted_and_zero_forecasts():
    t = R.radar(2, 48, 52, 41)
    same = _check(t, t.copy(), (20.0, 40.0))
    assert (same[:, 0] == same[:, 1]).all() and (same[..., 4] == same[..., 0]).all() and (same[..., 5] == same[..., 1]).all(), "everything matched"
    assert same[..., 0].sum() > 4
    blocks = np.zeros((1, 40, 40), dtype=np.float32)
    for y, x in ((2, 2), (2, 20), (20, 2), (20, 20), (30, 30)):
        blocks[0, y:y + 4, x:x + 4] = 1
    moved = blocks.copy()
    moved[0, 2:6, 20:24] = 0
    moved[0, 2:6, 30:34] = 1          # one block jumps away: it and its old place stay unmatched
    moved = _shift(moved, 2, 2)        # the others move by half their size: still touching
    got = _check(blocks, moved)[0, :, 0]
    assert got[:, 0].tolist() == [5, 5] and got[:, 4].tolist() == [4, 4] and got[:, 5].tolist() == [64, 64]
    none = _check(t, np.zeros_like(t), (20.0, 40.0))
    assert (none[:, 1] == 0).all() and (none[:, 0, :, 4:6] == 0).all() and (none[:, 0, :, :4] == same[:, 0, :, :4]).all()


# ------------------------------------------------------------------------------------------------ 5. the raw entry points: sources, accumulation
def _accum(pred_ptr, sample_stride, frame_stride, tgt, table, thr, T, scale=SCALE, min_area=1, ws=None):
    frames, H, W = tgt.shape
    nb = lib.query("adnm_valid_objects_accum_ws_bytes", frames, T, H, W, len(thr))
    assert nb >= 0
    if ws is None and nb:
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    lib.call("adnm_valid_objects_accum", pred_ptr, sample_stride, frame_stride, tgt.data_ptr(), table.data_ptr(), (ctypes.c_float * len(thr))(*thr), len(thr), scale,
             min_area, None if ws is None else ws.data_ptr(), nb, frames, T, H, W, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return nb


def _table(T, nthr, tail=0):
    n = lib.query("adnm_valid_objects_block_bytes", T, nthr) // 8
    assert n == T * 2 * nthr * 23
    return torch.zeros(n + tail, dtype=torch.float64, device=DEV)


def _whole(table, T, nthr):
    h = table[:T * 2 * nthr * 23].cpu().numpy()
    assert (h == np.rint(h)).all() and (h >= 0).all(), "an entry is not a count"
    return h.astype(np.int64).reshape(T, 2, nthr, 23)


def test_a_held_frame_is_the_materialised_repeat():
    B, T, T_in, H, W, thr = 2, 3, 2, 20, 28, (20.0, 40.0)
    tn, xn = R.radar(B * T, H, W, 51), R.radar(B * T_in, H, W, 52)
    t, x = _dev(tn), _dev(xn).view(B, T_in, H, W)
    a, b = _table(T, 2), _table(T, 2)
    _accum(x.data_ptr() + 4 * (T_in - 1) * H * W, T_in * H * W, 0, t, a, thr, T)          # the last input frame, held over the horizon
    held = x[:, -1:].expand(B, T, H, W).contiguous().view(B * T, H, W)
    _accum(held.data_ptr(), T * H * W, H * W, t, b, thr, T)
    assert torch.equal(_bits(a), _bits(b))
    assert (_whole(a, T, 2) == R.table(tn, held.cpu().numpy(), thr, SCALE, T)).all()
    lab = torch.empty(B * T, H, W, dtype=torch.int32, device=DEV)
    lib.call("adnm_label_objects", x.data_ptr() + 4 * (T_in - 1) * H * W, T_in * H * W, 0, lab.data_ptr(), 20.0, SCALE, 1, None, 0, B * T, T, H, W,
             torch.cuda.current_stream().cuda_stream)
    assert (lab.cpu().numpy() == R.label_field(held.cpu().numpy(), 20.0, SCALE)).all()


def test_a_source_at_a_4_byte_aligned_address():
    B, T, H, W, thr = 2, 2, 17, 23, (20.0,)
    tn, pn = R.radar(B * T, H, W, 61), R.radar(B * T, H, W, 62)
    hold_p, hold_t = (torch.zeros(B * T * H * W + 1, dtype=torch.float32, device=DEV) for _ in range(2))
    off_p, off_t = hold_p[1:].view(B * T, H, W), hold_t[1:].view(B * T, H, W)
    off_p.copy_(_dev(pn)), off_t.copy_(_dev(tn))
    assert off_p.data_ptr() % 16 == 4 and off_t.data_ptr() % 16 == 4
    got = _table(T, 1)
    _accum(off_p.data_ptr(), T * H * W, H * W, off_t, got, thr, T)
    assert (_whole(got, T, 1) == R.table(tn, pn, thr, SCALE, T)).all()
    assert (ops.label_objects(off_t, 20.0, SCALE).cpu().numpy() == R.label_field(tn, 20.0, SCALE)).all()


def test_two_calls_add_and_two_runs_give_equal_bits():
    B, T, H, W, thr = 2, 2, 32, 36, (20.0, 30.0, 40.0)
    batches = [(R.radar(B * T, H, W, s), R.radar(B * T, H, W, s + 1)) for s in (71, 73)]
    one = [R.table(t, p, thr, SCALE, T) for t, p in batches]
    tables = []
    for _ in range(2):
        table = _table(T, 3)
        for i, (t, p) in enumerate(batches):
            pd = _dev(p)
            _accum(pd.data_ptr(), T * H * W, H * W, _dev(t), table, thr, T)
            assert (_whole(table, T, 3) == sum(one[:i + 1])).all(), f"after batch {i}"
        tables.append(table)
    assert torch.equal(_bits(tables[0]), _bits(tables[1])), "the same calls on a fresh table give other bits"
    again = [ops.object_stats(_dev(batches[0][0]), _dev(batches[0][1]), thr, SCALE) for _ in range(2)]
    assert torch.equal(again[0], again[1])
    four = ops.object_stats(_dev(batches[0][0]).view(B, T, H, W), _dev(batches[0][1]).view(B, T, H, W), thr, SCALE)
    assert torch.equal(four, again[0]), "(B, T, H, W) is (frames, H, W)"


def test_more_frames_than_workgroups_in_the_workspace_route():
    """200 x 200 frames keep their words in the workspace, which has 512 slices: 130 frames at 4 thresholds make 520 items, so eight
    workgroups label a second item in their slice"""
    frames, H, W, thr = 130, 200, 200, (10.0, 20.0, 30.0, 40.0)
    one = R.radar(2, H, W, 81)
    t = np.zeros((frames, H, W), dtype=np.float32)
    t[0], t[1], t[128], t[129] = one[0], one[1], one[1], R.checkerboard(H, W)
    got = ops.object_stats(_dev(t), _dev(t), thr, SCALE).cpu().numpy()
    want = R.frame_stats(t[[0, 1, 128, 129]], t[[0, 1, 128, 129]], thr, SCALE)
    assert (got[[0, 1, 128, 129]] == want).all() and (got[2:128] == 0).all() and got[129, 0, 0, 0] == 1


# ------------------------------------------------------------------------------------------------ 6. the counts the project already has
def test_the_event_counts_are_those_of_the_pooled_pass():
    frames, H, W, thr = 3, 48, 52, (20.0, 30.0, 35.0, 27.5)
    t, p = R.radar(frames, H, W, 91, plant=True), R.radar(frames, H, W, 92, plant=True)
    td, pd = _dev(t), _dev(p)
    st = ops.object_stats(td, pd, thr, SCALE).cpu().numpy()
    counts = ops.pool_counts(td, pd, thr, SCALE, pools=((1, 1),)).cpu().numpy()[:, 0]          # (frames, 4 * nthr): TP, FN, FP, TN per threshold
    for k in range(len(thr)):
        assert (st[:, 0, k, 1] == counts[:, 4 * k] + counts[:, 4 * k + 1]).all(), "target events = TP + FN"
        assert (st[:, 1, k, 1] == counts[:, 4 * k] + counts[:, 4 * k + 2]).all(), "forecast events = TP + FP"
        assert st[:, :, k, 1].sum() > 0, "no event: nothing is compared"


# ------------------------------------------------------------------------------------------------ 7. the workspace contract
@pytest.mark.parametrize("H,W", [(64, 64), (200, 200), (256, 256)], ids=lambda v: str(v))
def test_the_workspace_and_what_lies_behind_it_and_behind_the_table(H, W):
    """the workspace at exactly the queried size between canaries; the result does not depend on what it held"""
    frames, T, thr = 1, 1, (20.0, 40.0)
    tn, pn = R.radar(frames, H, W, 101), R.radar(frames, H, W, 102)
    tgt, pred = _dev(tn), _dev(pn)
    nb = lib.query("adnm_valid_objects_accum_ws_bytes", frames, T, H, W, len(thr))
    assert (nb == 0) == (H * W <= 38400)
    cells, guard = T * 2 * len(thr) * 23, 4096
    results, labels = [], []
    for fill in (0x00, 0xFF):
        hold_ws = torch.full((guard + nb + guard,), 0xA5, dtype=torch.uint8, device=DEV)
        ws = hold_ws[guard:guard + nb]
        ws.fill_(fill)
        hold = torch.full((cells + 64,), -7.0, dtype=torch.float64, device=DEV)
        hold[:cells] = 0.0
        assert _accum(pred.data_ptr(), T * H * W, H * W, tgt, hold, thr, T, ws=ws if nb else None) == nb
        assert bool((hold_ws[:guard] == 0xA5).all()) and bool((hold_ws[guard + nb:] == 0xA5).all()), "a write outside the workspace"
        assert bool((hold[cells:] == -7.0).all()), "a write behind the table"
        results.append(hold[:cells].clone())
        lnb = lib.query("adnm_label_objects_ws_bytes", frames, T, H, W)
        lws = torch.full((guard + lnb + guard,), 0xA5, dtype=torch.uint8, device=DEV)
        lws[guard:guard + lnb] = fill
        lab = torch.full((frames * H * W + 64,), -7, dtype=torch.int32, device=DEV)
        lib.call("adnm_label_objects", tgt.data_ptr(), H * W, H * W, lab.data_ptr(), 20.0, SCALE, 1, lws[guard:].data_ptr() if lnb else None, lnb, frames, T, H, W,
                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool((lws[:guard] == 0xA5).all()) and bool((lws[guard + lnb:] == 0xA5).all()) and bool((lab[frames * H * W:] == -7).all())
        labels.append(lab[:frames * H * W].clone())
    assert torch.equal(_bits(results[0]), _bits(results[1])), "the result depends on what the workspace held"
    assert torch.equal(labels[0], labels[1])
    assert (_whole(results[0], T, len(thr)) == R.table(tn, pn, thr, SCALE, T)).all()
    assert (labels[0].cpu().numpy().reshape(frames, H, W) == R.label_field(tn, 20.0, SCALE)).all()


# ------------------------------------------------------------------------------------------------ 8. the Validator end to end
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


def test_validator_with_objects_end_to_end():
    from adnm_hip.validate import Validator, object_entries, objects_doubles
    from models.loss import RainfallLoss
    B, T, H, W, thr, min_area = 2, 3, 32, 32, [20, 30.5, 40], 2
    seq = R.radar(2 * B * 5, H, W, 111).reshape(2, B, 5, 1, H, W) * 0.7
    data = [(_dev(seq[i, :, :2]), _dev(seq[i, :, 2:])) for i in range(2)]
    kw = dict(pools=(4,), fss=(5,), joint=True)
    val = Validator(Drift(), RainfallLoss(), T, SCALE, thr, objects=min_area, **kw)
    former = Validator(Drift(), RainfallLoss(), T, SCALE, thr, objects=None, **kw)
    try:
        n = objects_doubles(T, len(thr), min_area)
        assert n == T * 2 * len(thr) * 23
        want = np.zeros((T, 2, len(thr), 23), dtype=np.int64)
        for x, tgt in data:            # two steps through the captured graph
            out = val.step(x, tgt)
            want += R.table(tgt.cpu().numpy().reshape(B * T, H, W), out.cpu().numpy().reshape(B * T, H, W), thr, SCALE, T, min_area)
            former.step(x, tgt)
        assert want[:, :, 0, 0].min() > 0 and (want[:, 1, 0] != want[:, 0, 0]).any(), "no objects, or a forecast equal to the target: nothing is tested"
        # with objects=None nothing is there: the old length, no workspace, no key
        assert val._block.numel() == former._block.numel() + n and former.objects is None
        assert all(e.get("ws_objects") is None for e in former._fwd._graphs.values())
        assert (_whole(val._block[-n:], T, len(thr)) == want).all(), "the table at the end of the one allocation"
        assert torch.equal(_bits(val._block[:-n]), _bits(former._block)), "a former offset moved, or a former pass counts differently"
        res, old = val.done(per_lead=True), former.done(per_lead=True)
        assert "objects" not in old and "objects" not in old["per_lead"]
        assert list(res) == list(old)[:-1] + ["objects", "per_lead"] and list(res["per_lead"]) == list(old["per_lead"]) + ["objects"]
        assert list(res)[-3:] == ["joint", "objects", "per_lead"]
        assert _same_tree({k: res[k] for k in old if k != "per_lead"}, {k: old[k] for k in old if k != "per_lead"}), "a former entry moved"
        assert _same_tree({k: res["per_lead"][k] for k in old["per_lead"]}, old["per_lead"]), "a former per-lead entry moved"
        assert (res["samples"], res["batches"]) == (2 * B, 2)
        assert _same_tree(res["objects"], object_entries(want.sum(axis=0), 2 * B * T, thr, min_area))
        assert _same_tree(res["per_lead"]["objects"], object_entries(want, 2 * B, thr, min_area))
        assert res["objects"]["min_area"] == 2 and res["objects"][20]["target"]["count"] == int(want[:, 0, 0, 0].sum())
        print("objects end to end at 20:", {k: v for k, v in res["objects"][20].items() if not isinstance(v, (dict, np.ndarray))})
        # once the graph exists a step allocates nothing
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        val.step(*data[0])
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == before
        val.reset()
        assert float(val._block.abs().sum()) == 0.0, "reset() zeroes the tail"
    finally:
        val.close()
        former.close()


def test_validator_raises_at_the_first_step_on_a_frame_above_the_limit():
    from adnm_hip.validate import Validator
    from models.loss import RainfallLoss

    class Last(torch.nn.Module):
        def forward(self, x):
            return x[:, -1:, 0].float()
    val = Validator(Last(), RainfallLoss(), 1, SCALE, [20], ssim=False, objects=True)
    try:
        x = torch.zeros(1, 1, 1, 257, 256, device=DEV)
        with pytest.raises(RuntimeError, match="65536"):
            val.step(x, x.clone())
    finally:
        val.close()
