"""Space-time tracks on the GPU (csrc/tracks.hip: adnm_valid_tracks_accum, adnm_label_tracks; ops.track_stats, ops.label_tracks;
Validator(tracks=)) against scipy.ndimage.label with the full 3 x 3 x 3 structure on the CPU (tracks_ref).  Every comparison is integer for
integer over the whole table and voxel for voxel over the label volume; there is no tolerance anywhere.  Frames of 192 x 200 are the largest
whose labelling words live in LDS, 193 x 200 the first that are labelled in the workspace, 256 x 256 the limit."""
import ctypes

import numpy as np
import pytest
import torch

import objects_ref as O
import tracks_ref as R
from adnm_hip import lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALE, HALF = 90.0, (45.0,)
SHAPES = [(1, 1, 1), (2, 1, 1), (3, 1, 5), (2, 3, 3), (3, 8, 8), (4, 7, 9), (3, 33, 65), (5, 31, 67), (2, 64, 64), (20, 16, 16), (2, 192, 200), (2, 193, 200),
          (3, 256, 256)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _later(a, n=1):
    """the (B, T, H, W) field n frames later, zeros coming in"""
    out = np.zeros_like(a)
    if n < a.shape[1]:
        out[:, n:] = a[:, :a.shape[1] - n]
    return out


def _check(t, p, thr=HALF, scale=SCALE, min_volume=1, labels=True):
    """(B, T, H, W) numpy fields: the table of both fields integer for integer, the labels of both voxel for voxel -> the statistics"""
    t, p = np.asarray(t, dtype=np.float32), np.asarray(p, dtype=np.float32)
    B, T = t.shape[:2]
    td, pd = _dev(t), _dev(p)
    got = ops.track_stats(td, pd, thr, scale, min_volume)
    assert got.dtype == torch.int64 and tuple(got.shape) == (B, 2, len(thr), 7 + 4 * T) and got.device.type == "cuda"
    got = got.cpu().numpy()
    want = R.sample_stats(t, p, thr, scale, min_volume)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"(sample, field, threshold, column) {bad[:8].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
    for row in got.reshape(-1, 7 + 4 * T):
        assert R.identities(row, T)
    if labels:
        for v in thr:
            for name, host, dev in (("target", t, td), ("forecast", p, pd)):
                lab = ops.label_tracks(dev, v, scale, min_volume)
                assert lab.dtype == torch.int32 and lab.shape == dev.shape
                ref = R.label_field(host, v, scale, min_volume)
                wrong = np.argwhere(lab.cpu().numpy() != ref)
                assert wrong.size == 0, f"labels of the {name} at {v}: {len(wrong)} voxels differ, the first at {wrong[0].tolist()}"
    return got


# ------------------------------------------------------------------------------------------------ 1. shapes and patterns
@pytest.mark.parametrize("name", ["empty", "full", "lattice", "noise"])
@pytest.mark.parametrize("T,H,W", SHAPES, ids=lambda v: str(v))
def test_patterns_at_every_shape(T, H, W, name):
    """one sample; the forecast is the pattern one frame later"""
    t = {"empty": np.zeros((T, H, W), np.float32), "full": np.ones((T, H, W), np.float32), "lattice": R.lattice3(T, H, W),
         "noise": R.noise3(T, H, W, 0.08, T * H + W)}[name][None]
    got = _check(t, _later(t))[0, 0, 0]
    if name == "empty":
        assert (got == 0).all()
    if name == "full":
        n = T * H * W
        assert got[:7].tolist() == [1, n, n * n, T, int(T > 1), n if T > 1 else 0, 1] and got[7] == got[7 + 2 * T - 1] == got[7 + 4 * T - 1] == 1
    if name == "lattice":
        n = ((T + 1) // 2) * ((H + 1) // 2) * ((W + 1) // 2)
        assert got[0] == got[1] == got[2] == got[3] == n == got[7 + 3 * T], "every record in use: tracks of one voxel"


def test_the_flagship_volume():
    t = R.discs(1, 20, 128, 128, 5)
    t = np.maximum(t, 0.6 * R.noise3(20, 128, 128, 0.03, 9)[None])
    got = _check(t, _later(t, 2), (20.0, 50.0))
    assert got[0, 0, 0, 0] > 50 and got[0, 0, 0, 6] >= 0 and got[0, 0, 0, 3] > got[0, 0, 0, 0], "many tracks, some of more than one frame"


def test_a_volume_above_the_limits_raises():
    z = torch.zeros(1, 2, 257, 256, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="65536"):
        ops.track_stats(z, z, HALF, SCALE)
    with pytest.raises(RuntimeError, match="65536"):
        ops.label_tracks(z, 45.0, SCALE)
    z = torch.zeros(1, 65, 256, 256, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="4194304"):
        ops.track_stats(z, z, HALF, SCALE)
    with pytest.raises(RuntimeError, match="4194304"):
        ops.label_tracks(z, 45.0, SCALE)
    s = torch.zeros(1, 2, 8, 8, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="min_volume"):
        ops.track_stats(s, s, HALF, SCALE, min_volume=0)
    with pytest.raises(ValueError, match="thresholds"):
        ops.track_stats(s, s, list(range(9)), SCALE)


# ------------------------------------------------------------------------------------------------ 2. motion
def test_a_voxel_moving_one_pixel_is_one_track_and_two_pixels_a_track_per_frame():
    T, H, W = 4, 9, 9
    slow = np.stack([R.mover(T, H, W, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    got = _check(slow, slow)
    assert (got[:, :, 0, :7] == [1, T, T * T, T, 1, T, 1]).all(), "one spanning track of T voxels in every direction and standing still"
    fast = np.stack([R.mover(T, H, W, dy, dx, step=2) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx])
    got = _check(fast, slow[:8])
    assert (got[:, 0, 0, :4] == [T, T, T, T]).all() and (got[:, 0, 0, 6] == 0).all(), "T tracks of one voxel and one frame"


def test_long_union_chains_and_a_fork_in_time():
    s, sp = R.serpentine3(4, 16, 16), R.spiral3(4, 16)
    got = _check(np.stack([s, sp]), np.stack([sp, s[::-1].copy()]))
    assert (got[:, :, 0, 0] == 1).all() and got[0, 0, 0, 1] == int(s.sum()) and got[1, 0, 0, 1] == int(sp.sum())
    y = R.fork(6, 8, 12)[None]
    got = _check(y, _later(y))
    assert got[0, 0, 0, :7].tolist() == [2, 22, 242, 12, 2, 22, 2], "two cells that merge are one track; one that splits is one track"
    _check(np.stack([R.serpentine3(3, 37, 45)]), np.stack([R.lattice3(3, 37, 45)]))


@pytest.mark.parametrize("density", [0.03, 0.08, 0.2])
def test_noise_below_and_above_the_percolation_threshold(density):
    T, H, W = 5, 33, 65
    t = np.stack([R.noise3(T, H, W, density, 11), R.noise3(T, H, W, density, 12)])
    p = np.stack([R.noise3(T, H, W, density, 13), _later(t[1:2])[0]])
    got = _check(t, p)
    events = got[:, 0, 0, 1]
    assert (abs(events / (T * H * W) - density) < 0.02).all()
    if density == 0.2:
        assert (got[:, 0, 0, 2] > (events // 2) ** 2).all() and (got[:, 0, 0, 0] < 200).all(), "one giant track plus dust"
    else:
        assert (got[:, 0, 0, 0] > 50).all(), "many tracks"


# ------------------------------------------------------------------------------------------------ 3. parameters
@pytest.mark.parametrize("min_volume", [1, 2, 9])
@pytest.mark.parametrize("nthr", [1, 4, 8])
def test_moving_discs_with_planted_values(nthr, min_volume):
    """NaN, +-Inf, negatives and values > 1 planted; threshold 0 makes every voxel an event, 91 none"""
    thr = (20.0, 0.0, 40.0, 91.0, 30.5, 60.0, 75.0, 89.0)[:nthr]
    t, p = R.discs(3, 6, 24, 28, 31, plant=True), R.discs(3, 6, 24, 28, 32, plant=True)
    got = _check(t, p, thr, min_volume=min_volume)
    assert got[:, :, 0, 0].sum() >= 1
    if nthr >= 4:
        n = 6 * 24 * 28
        assert (got[:, :, 1, :7] == [1, n, n * n, 6, 1, n, 1]).all() and (got[:, :, 3] == 0).all()
    if nthr == 1:
        _check(t[:1], p[:1], (20.0, 35.5), 89.5, min_volume)          # a fractional scale and a fractional threshold


def test_min_volume_drops_small_tracks_from_every_column():
    f = np.zeros((1, 4, 12, 12), dtype=np.float32)
    f[0, 0, 1, 1] = 1                     # 1 voxel
    f[0, 1:3, 5, 2:6] = 1                 # 8 voxels in 2 frames
    f[0, :, 9, 9] = 1                     # 4 voxels in 4 frames, plus 5 in the last: 9
    f[0, 3, 9:11, 8:11] = 1
    other = np.zeros_like(f)
    other[0, 0, 1, 1] = other[0, 3, 10, 8] = 1
    for mv, (n, v, m) in ((1, (3, 18, 2)), (2, (2, 17, 1)), (9, (1, 9, 1)), (10, (0, 0, 0))):
        got = _check(f, other, min_volume=mv)[0, 0, 0]
        assert (got[0], got[1], got[4]) == (n, v, m), mv


def test_samples_never_connect():
    """the last frame of one sample and the first of the next are both full: B tracks, not one"""
    B, T, H, W = 3, 2, 5, 7
    t = np.ones((B, T, H, W), dtype=np.float32)
    got = _check(t, t)
    assert (got[:, :, 0, 0] == 1).all() and (got[:, :, 0, 1] == T * H * W).all()
    lab = ops.label_tracks(_dev(t), 45.0, SCALE).cpu().numpy()
    assert (lab == 1).all(), "every sample's track starts at its own voxel 0"


def test_equal_shifted_and_zero_forecasts():
    t = R.discs(2, 5, 20, 24, 41)
    same = _check(t, t.copy(), (20.0, 60.0))
    assert (same[:, 0] == same[:, 1]).all() and (same[..., 4] == same[..., 0]).all() and (same[..., 5] == same[..., 1]).all(), "everything matched"
    assert same[..., 0].sum() > 4
    _check(t, _later(t, 2), (20.0, 60.0))
    none = _check(t, np.zeros_like(t), (20.0, 60.0))
    assert (none[:, 1] == 0).all() and (none[:, 0, :, 4:6] == 0).all() and (none[:, 0, :, :4] == same[:, 0, :, :4]).all()


# ------------------------------------------------------------------------------------------------ 4. the raw entry points
def _accum(pred_ptr, sample_stride, frame_stride, tgt, table, thr, scale=SCALE, min_volume=1, ws=None, nb=None):
    B, T, H, W = tgt.shape
    need = lib.query("adnm_valid_tracks_accum_ws_bytes", B * T, T, H, W, len(thr))
    assert need > 0
    nb = need if nb is None else nb
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    lib.call("adnm_valid_tracks_accum", pred_ptr, sample_stride, frame_stride, tgt.data_ptr(), table.data_ptr(), (ctypes.c_float * len(thr))(*thr), len(thr), scale,
             min_volume, ws.data_ptr(), nb, B * T, T, H, W, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return need


def _table(T, nthr, tail=0):
    n = lib.query("adnm_valid_tracks_block_bytes", T, nthr) // 8
    assert n == 2 * nthr * (7 + 4 * T)
    return torch.zeros(n + tail, dtype=torch.float64, device=DEV)


def _whole(table, T, nthr):
    h = table[:2 * nthr * (7 + 4 * T)].cpu().numpy()
    assert (h == np.rint(h)).all() and (h >= 0).all(), "an entry is not a count"
    return h.astype(np.int64).reshape(2, nthr, 7 + 4 * T)


def test_a_held_frame_gives_only_spanning_tracks():
    B, T, T_in, H, W, thr = 2, 3, 2, 20, 28, (20.0, 40.0)
    tn, xn = O.radar(B * T, H, W, 51).reshape(B, T, H, W), O.radar(B * T_in, H, W, 52)
    t, x = _dev(tn), _dev(xn).view(B, T_in, H, W)
    a, b = _table(T, 2), _table(T, 2)
    _accum(x.data_ptr() + 4 * (T_in - 1) * H * W, T_in * H * W, 0, t, a, thr)          # the last input frame, held over the horizon
    held = x[:, -1:].expand(B, T, H, W).contiguous()
    _accum(held.data_ptr(), T * H * W, H * W, t, b, thr)
    assert torch.equal(_bits(a), _bits(b))
    got = _whole(a, T, 2)
    assert (got == R.table(tn, held.cpu().numpy(), thr, SCALE)).all()
    frame = ops.object_stats(x[:, -1].contiguous(), x[:, -1].contiguous(), thr, SCALE).cpu().numpy().sum(axis=0)[1]          # (nthr, 23)
    f = got[1]
    assert (f[:, 0] == frame[:, 0]).all() and (f[:, 6] == f[:, 0]).all() and (f[:, 1] == T * frame[:, 1]).all() and (f[:, 2] == T * T * frame[:, 2]).all()
    assert (f[:, 3] == T * f[:, 0]).all() and f[:, 0].min() > 0, "every track spans, v = T * area, the counts are the frame's objects"
    lab = torch.empty(B, T, H, W, dtype=torch.int32, device=DEV)
    nb = lib.query("adnm_label_tracks_ws_bytes", B * T, T, H, W)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    lib.call("adnm_label_tracks", x.data_ptr() + 4 * (T_in - 1) * H * W, T_in * H * W, 0, lab.data_ptr(), 20.0, SCALE, 1, ws.data_ptr(), nb, B * T, T, H, W,
             torch.cuda.current_stream().cuda_stream)
    assert (lab.cpu().numpy() == R.label_field(held.cpu().numpy(), 20.0, SCALE)).all()


def test_a_source_at_a_4_byte_aligned_address():
    B, T, H, W, thr = 2, 3, 17, 23, (20.0,)
    tn, pn = R.discs(B, T, H, W, 61), R.discs(B, T, H, W, 62)
    hold_p, hold_t = (torch.zeros(B * T * H * W + 1, dtype=torch.float32, device=DEV) for _ in range(2))
    off_p, off_t = hold_p[1:].view(B, T, H, W), hold_t[1:].view(B, T, H, W)
    off_p.copy_(_dev(pn)), off_t.copy_(_dev(tn))
    assert off_p.data_ptr() % 16 == 4 and off_t.data_ptr() % 16 == 4
    got = _table(T, 1)
    _accum(off_p.data_ptr(), T * H * W, H * W, off_t, got, thr)
    assert (_whole(got, T, 1) == R.table(tn, pn, thr, SCALE)).all()
    assert (ops.label_tracks(off_t, 20.0, SCALE).cpu().numpy() == R.label_field(tn, 20.0, SCALE)).all()


def test_the_table_is_added_to_and_two_runs_give_equal_bits():
    B, T, H, W, thr = 2, 4, 32, 36, (20.0, 30.0, 40.0)
    batches = [(R.discs(B, T, H, W, s), R.discs(B, T, H, W, s + 1)) for s in (71, 73)]
    one = [R.table(t, p, thr, SCALE) for t, p in batches]
    fill = np.arange(2 * 3 * (7 + 4 * T), dtype=np.int64).reshape(2, 3, -1) * 7 + 3
    tables = []
    for _ in range(2):
        table = _table(T, 3, tail=8)
        table[:fill.size] = torch.from_numpy(fill.ravel().astype(np.float64)).to(DEV)
        table[fill.size:] = -7.0
        for i, (t, p) in enumerate(batches):
            pd = _dev(p)
            _accum(pd.data_ptr(), T * H * W, H * W, _dev(t), table, thr)
            assert (_whole(table, T, 3) == fill + sum(one[:i + 1])).all(), f"after batch {i}"
        assert bool((table[fill.size:] == -7.0).all()), "a write behind the table"
        tables.append(table)
    assert torch.equal(_bits(tables[0]), _bits(tables[1])), "the same calls give other bits"
    again = [ops.track_stats(_dev(batches[0][0]), _dev(batches[0][1]), thr, SCALE) for _ in range(2)]
    assert torch.equal(again[0], again[1]) and (again[0].sum(dim=0).cpu().numpy() == one[0]).all()


def test_labels_keep_nothing_of_what_the_memory_held():
    B, T, H, W = 2, 3, 33, 65
    f = R.discs(B, T, H, W, 81)
    fd, want = _dev(f), R.label_field(f, 20.0, SCALE, 2)
    nb = lib.query("adnm_label_tracks_ws_bytes", B * T, T, H, W)
    for pattern in (0x5A5A5A5A, -0x5A5A5A5B):
        lab = torch.full((B * T * H * W + 16,), pattern, dtype=torch.int32, device=DEV)
        ws = torch.full((nb // 4,), pattern, dtype=torch.int32, device=DEV)
        lib.call("adnm_label_tracks", fd.data_ptr(), T * H * W, H * W, lab.data_ptr(), 20.0, SCALE, 2, ws.data_ptr(), nb, B * T, T, H, W,
                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool((lab[B * T * H * W:] == pattern).all()), "a write behind the labels"
        assert (lab[:B * T * H * W].cpu().numpy().reshape(f.shape) == want).all()


@pytest.mark.parametrize("T,H,W", [(3, 33, 65), (2, 193, 200)], ids=lambda v: str(v))
def test_a_guarded_poisoned_workspace_gives_the_plain_bits(T, H, W, monkeypatch):
    from util import guarded_workspaces
    thr = (20.0, 40.0)
    t, p = R.discs(2, T, H, W, 91), R.discs(2, T, H, W, 92)
    td, pd = _dev(t), _dev(p)
    plain, plain_lab = ops.track_stats(td, pd, thr, SCALE), ops.label_tracks(td, 20.0, SCALE)
    with guarded_workspaces(monkeypatch) as g:
        got, lab = ops.track_stats(td, pd, thr, SCALE), ops.label_tracks(td, 20.0, SCALE)
        g.check()
        assert g.calls == 2
        assert [r[2] for r in g.records] == [lib.query("adnm_valid_tracks_accum_ws_bytes", T, T, H, W, 2), lib.query("adnm_label_tracks_ws_bytes", 2 * T, T, H, W)]
    assert torch.equal(got, plain) and torch.equal(lab, plain_lab)
    assert (got.cpu().numpy() == R.sample_stats(t, p, thr, SCALE)).all()


def test_a_workspace_four_bytes_short_is_refused_before_any_launch():
    B, T, H, W, thr = 1, 2, 8, 8, (20.0,)
    t = _dev(R.discs(B, T, H, W, 95))
    table = _table(T, 1)
    need = lib.query("adnm_valid_tracks_accum_ws_bytes", B * T, T, H, W, 1)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match=f"workspace {need - 4} < {need} bytes"):
        _accum(t.data_ptr(), T * H * W, H * W, t, table, thr, ws=ws, nb=need - 4)
    assert float(table.abs().sum()) == 0.0
    lnb = lib.query("adnm_label_tracks_ws_bytes", B * T, T, H, W)
    lab = torch.zeros(B, T, H, W, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match=f"workspace {lnb - 4} < {lnb} bytes"):
        lib.call("adnm_label_tracks", t.data_ptr(), T * H * W, H * W, lab.data_ptr(), 20.0, SCALE, 1, ws.data_ptr(), lnb - 4, B * T, T, H, W,
                 torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ 5. the code that exists
def test_one_frame_volumes_are_the_object_scores():
    frames, H, W, thr = 3, 48, 52, (20.0, 40.0)
    t, p = O.radar(frames, H, W, 101, plant=True), O.radar(frames, H, W, 102, plant=True)
    td, pd = _dev(t), _dev(p)
    for min_size in (1, 3):
        tr = ops.track_stats(td.view(frames, 1, H, W), pd.view(frames, 1, H, W), thr, SCALE, min_size).cpu().numpy()
        ob = ops.object_stats(td, pd, thr, SCALE, min_size).cpu().numpy()
        assert (tr[..., [0, 1, 2, 4, 5]] == ob[..., [0, 1, 2, 4, 5]]).all() and (tr[..., 3] == tr[..., 0]).all() and (tr[..., 6] == tr[..., 0]).all()
        assert tr[..., 0].sum() > 0
        assert torch.equal(ops.label_tracks(td.view(frames, 1, H, W), 20.0, SCALE, min_size).view(frames, H, W), ops.label_objects(td, 20.0, SCALE, min_size))


def test_the_event_counts_are_those_of_the_pooled_pass():
    B, T, H, W, thr = 2, 3, 24, 28, (20.0, 30.0, 35.0, 27.5)
    t, p = R.discs(B, T, H, W, 111, plant=True), R.discs(B, T, H, W, 112, plant=True)
    td, pd = _dev(t), _dev(p)
    st = ops.track_stats(td, pd, thr, SCALE).cpu().numpy()
    counts = ops.pool_counts(td, pd, thr, SCALE, pools=((1, 1),)).cpu().numpy()[:, 0].reshape(B, T, -1).sum(axis=1)          # TP, FN, FP, TN per threshold
    for k in range(len(thr)):
        assert (st[:, 0, k, 1] == counts[:, 4 * k] + counts[:, 4 * k + 1]).all(), "target events = TP + FN"
        assert (st[:, 1, k, 1] == counts[:, 4 * k] + counts[:, 4 * k + 2]).all(), "forecast events = TP + FP"
        assert st[:, :, k, 1].sum() > 0, "no event: nothing is compared"


# ------------------------------------------------------------------------------------------------ 6. the Validator end to end
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


def test_validator_with_tracks_end_to_end():
    from adnm_hip.dataio import ResidentDataset
    from adnm_hip.validate import Validator, track_entries, tracks_doubles
    from models.loss import RainfallLoss
    B, T, H, W, thr, mv = 2, 3, 32, 32, [20, 30.5, 40], 2
    seq = (R.discs(3 * B, 5, H, W, 121) * 0.7).reshape(3, B, 5, 1, H, W)
    data = [(_dev(seq[i, :, :2]), _dev(seq[i, :, 2:])) for i in range(3)]
    kw = dict(pools=(4,), persistence=True, objects=2, sal=True, nprob=(1, 5))
    val = Validator(Drift(), RainfallLoss(), T, SCALE, thr, tracks=dict(min_volume=mv), **kw)
    former = Validator(Drift(), RainfallLoss(), T, SCALE, thr, **kw)
    try:
        n = tracks_doubles(T, len(thr), mv)
        assert n == 2 * len(thr) * (7 + 4 * T)

        def epoch(batches):
            want = np.zeros((2, len(thr), 7 + 4 * T), dtype=np.int64)
            for x, tgt in batches:            # through the captured graph
                out = val.step(x, tgt)
                want += ops.track_stats(tgt[:, :, 0].contiguous(), out.contiguous(), thr, SCALE, mv).sum(dim=0).cpu().numpy()
            return want
        want = epoch(data[:2])
        for x, tgt in data[:2]:
            former.step(x, tgt)
        host = R.table(np.concatenate([seq[i, :, 2:, 0] for i in range(2)]), np.concatenate([Drift()(d[0]).cpu().numpy() for d in data[:2]]), thr, SCALE, mv)
        assert (want == host).all() and want[:, 0, 0].min() > 0 and (want[1] != want[0]).any(), "no tracks, or a forecast equal to the target: nothing is tested"
        # with tracks=None nothing is there: the old length, no workspace, no key
        assert val._block.numel() == former._block.numel() + n and former.tracks is None
        assert all(e.get("ws_tracks") is None for e in former._fwd._graphs.values())
        assert (_whole(val._block[-n:], T, len(thr)) == want).all(), "the table at the end of the one allocation"
        assert torch.equal(_bits(val._block[:-n]), _bits(former._block)), "a former offset moved, or a former pass counts differently"
        res, old = val.done(per_lead=True, reset=True), former.done(per_lead=True)
        assert "tracks" not in old and list(res) == list(old)[:-1] + ["tracks", "per_lead"] and list(res["per_lead"]) == list(old["per_lead"])
        assert _same_tree({k: res[k] for k in old if k != "per_lead"}, {k: old[k] for k in old if k != "per_lead"}), "a former entry moved"
        assert _same_tree(res["per_lead"], old["per_lead"]), "a former per-lead entry moved"
        assert (res["samples"], res["batches"]) == (2 * B, 2)
        assert _same_tree(res["tracks"], track_entries(want, 2 * B, thr, T, mv)) and res["tracks"]["min_volume"] == mv
        assert res["tracks"][20]["target"]["count"] == int(want[0, 0, 0])
        print("tracks end to end at 20:", {k: v for k, v in res["tracks"][20].items() if not isinstance(v, dict)})
        # a second epoch is independent of the first
        assert float(val._block.abs().sum()) == 0.0, "reset zeroes the tail"
        second = epoch(data[2:])
        assert (second != want).any() and _same_tree(val.done(reset=True)["tracks"], track_entries(second, B, thr, T, mv))
        # step_from a ResidentDataset: the same batches fetched by the feed's kernel into the graph's static buffers
        feed = ResidentDataset.from_frames(torch.from_numpy(seq.reshape(3 * B, 5, H, W)), 2, B, DEV, shuffle=False)
        feed.begin_epoch()
        for _ in range(2):
            val.step_from(feed)
        assert _same_tree(val.done(reset=True)["tracks"], res["tracks"])
    finally:
        val.close()
        former.close()


def test_validator_raises_at_the_first_step_on_a_volume_above_the_limit():
    from adnm_hip.validate import Validator
    from models.loss import RainfallLoss

    class Last(torch.nn.Module):
        def forward(self, x):
            return x[:, -1:, 0].float()
    val = Validator(Last(), RainfallLoss(), 1, SCALE, [20], ssim=False, tracks=True)
    try:
        x = torch.zeros(1, 1, 1, 257, 256, device=DEV)
        with pytest.raises(RuntimeError, match="65536"):
            val.step(x, x.clone())
    finally:
        val.close()
