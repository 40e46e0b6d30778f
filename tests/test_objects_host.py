"""The object scores without a GPU: the yardstick (objects_ref) on hand-made masks with written-out expectations, ops.objects_spec,
validate.block_parts with the new row, validate.object_entries on a hand-made table, validate.aggregate reading the objects table at its own
offset, and the entry points at the C boundary (declared, exported, the queries pure host functions that refuse every limit)."""
import ctypes
import inspect
import math

import numpy as np
import pytest
from scipy import ndimage

import objects_ref as R
from adnm_hip import lib, ops

NEW = ("adnm_valid_objects_block_bytes", "adnm_valid_objects_accum_ws_bytes", "adnm_valid_objects_accum", "adnm_label_objects_ws_bytes", "adnm_label_objects")


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or (a.dtype.kind in "iu") != (b.dtype.kind in "iu"):
        return False
    if a.dtype.kind in "iu":
        return bool((a == b).all())
    return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def _same_tree(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same_tree(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is b
    return _eq(a, b)


def _four(mask):
    return ndimage.label(mask)[1]   # scipy's default structure: 4-connectivity


# ------------------------------------------------------------------------------------------------ the yardstick on hand-made masks
def test_a_diagonal_is_one_object_under_8_connectivity():
    m = np.eye(5, dtype=bool)
    assert _four(m) == 5
    assert (R.canonical(m) == np.eye(5, dtype=np.int32)).all(), "one object whose first pixel is index 0: label 1 everywhere on the diagonal"
    anti = m[:, ::-1]
    assert (R.canonical(anti) == 5 * anti).all(), "the anti-diagonal starts at (0, 4): label 5"
    r = R.row(m, np.zeros_like(m))
    assert r.tolist() == [1, 5, 25, 5, 0, 0] + [0, 0, 1] + [0] * 14   # floor(log2(5)) = 2


def test_two_blobs_that_touch_at_a_corner_are_one_object():
    m = np.zeros((6, 7), dtype=bool)
    m[1:3, 1:3] = True          # 4 pixels, first pixel (1, 1) = index 8
    m[3:5, 3:6] = True          # 6 pixels, touching the first at the corner (2, 2) / (3, 3)
    m[0, 6] = True              # an isolated pixel, index 6
    assert _four(m) == 3
    lab = R.canonical(m)
    assert sorted(set(lab.ravel().tolist())) == [0, 7, 9] and (lab[m & (lab != 7)] == 9).all() and lab[0, 6] == 7
    other = np.zeros_like(m)
    other[4, 5] = True          # touches the big object only
    r = R.row(m, other)
    assert r[:6].tolist() == [2, 11, 1 + 100, 10, 1, 10]
    assert r[6:].tolist() == [1, 0, 0, 1] + [0] * 13          # areas 1 and 10: bins 0 and 3
    assert R.row(m, other, min_area=2)[:6].tolist() == [1, 10, 100, 10, 1, 10]
    assert R.row(m, other, min_area=11)[:6].tolist() == [0] * 6
    assert (R.canonical(m, min_area=2) == np.where(lab == 9, 9, 0)).all()
    back = R.row(other, m)      # the other way round: one object of one pixel, matched
    assert back[:6].tolist() == [1, 1, 1, 1, 1, 1] and back[6] == 1


def test_the_patterns_are_what_their_names_say():
    for H, W in ((32, 32), (7, 9), (128, 128)):
        s = R.serpentine(H, W) > 0
        assert ndimage.label(s, structure=R.EIGHT)[1] == 1 and _four(s) == 1
        assert (ndimage.convolve(s.astype(int), np.ones((3, 3), int), mode="constant")[s] <= 5).all(), "a path, not a blob: a joint sees itself, two pixels of each row"
        assert ndimage.label(R.comb(H, W) > 0, structure=R.EIGHT)[1] == 1
        assert ndimage.label(R.comb(H, W)[:-1] > 0, structure=R.EIGHT)[1] == (W + 1) // 2, "the teeth meet only in the last row"
        assert ndimage.label(R.lattice(H, W) > 0, structure=R.EIGHT)[1] == ((H + 1) // 2) * ((W + 1) // 2)
        c = R.checkerboard(H, W) > 0
        assert ndimage.label(c, structure=R.EIGHT)[1] == 1 and _four(c) == c.sum()
    for n in (32, 128):
        sp = R.spiral(n) > 0
        assert ndimage.label(sp, structure=R.EIGHT)[1] == 1 and _four(sp) == 1 and n * n // 3 < sp.sum() < 2 * n * n // 3
    f = R.radar(2, 64, 64, 1)
    assert 0.85 < (f == 0).mean() < 0.95
    p = R.radar(2, 64, 64, 1, plant=True)
    assert np.isnan(p).any() and np.isinf(p).any() and (p < 0).any() and (p > 1).any()


def test_quantisation_of_the_yardstick():
    v = np.array([np.nan, -np.inf, -1.0, 0.0, 0.5, 1.0, 7.0, np.inf], dtype=np.float32)
    assert R.quantise(v, 90.0).tolist() == [0, 0, 0, 0, 45, 90, 90, 90]
    assert R.quantise(v, 89.5).tolist() == [0, 0, 0, 0, 44, 89, 89, 89]
    assert R.events(v, 0, 90.0).all() and not R.events(v, 91, 90.0).any()


def test_table_folds_frames_by_frame_index():
    t, p = R.radar(6, 16, 16, 4), R.radar(6, 16, 16, 5)
    st = R.frame_stats(t, p, (20, 40), 90.0)
    tab = R.table(t, p, (20, 40), 90.0, 3)
    assert (tab == st[:3] + st[3:]).all() and st[:, :, 0, 0].sum() > 0


# ------------------------------------------------------------------------------------------------ objects_spec
def test_objects_spec():
    assert ops.objects_spec(None) is None and ops.objects_spec(False) is None
    assert ops.objects_spec(True) == 1 and ops.objects_spec(1) == 1 and ops.objects_spec(9) == 9 and ops.objects_spec(np.int64(4)) == 4
    assert isinstance(ops.objects_spec(np.int64(4)), int)
    for bad in (0, -1, 2.0, "3", (1,), [2], 1.5, float("nan")):
        with pytest.raises(ValueError, match="objects"):
            ops.objects_spec(bad)
    assert (ops.OBJ_COLS, ops.OBJ_BINS) == (23, 17) == (R.COLS, R.BINS) and "65536" in ops.OBJECTS_LIMITS


# ------------------------------------------------------------------------------------------------ block_parts
def test_block_parts_holds_the_new_row_last():
    from adnm_hip.validate import HEADER, block_parts, objects_doubles
    assert list(inspect.signature(block_parts).parameters)[-1] == "objects" and inspect.signature(block_parts).parameters["objects"].default is None
    T, n = 3, 2
    for kw in (dict(), dict(pools=((4, 4),), persistence=True, fss=(1, 5), advection=True, spectrum=(16, 32), joint=7)):
        off, off_n = block_parts(T, n, **kw)
        for none in (None, False, 0):
            assert block_parts(T, n, objects=none, **kw) == (off, off_n), "the same parts as without the keyword"
        on, on_n = block_parts(T, n, objects=1, **kw)
        assert on[:-1] == off and on_n == off_n + T * 2 * n * 23
        last = on[-1]
        assert tuple(last) == ("objects", "objects", "pred", (), (T, 2, n, 23), off_n) and last.size == T * 2 * n * 23
        assert block_parts(T, n, objects=9, **kw) == (on, on_n), "min_area does not change the table"
    assert block_parts(T, n)[0][0].size == HEADER + T * (4 * n + 3)
    assert objects_doubles(T, n) == objects_doubles(T, n, None) == objects_doubles(T, n, False) == 0
    assert objects_doubles(T, n, True) == objects_doubles(T, n, 5) == T * 2 * n * 23 and objects_doubles(20, 4, True) == 20 * 2 * 4 * 23
    with pytest.raises(ValueError, match="objects"):
        objects_doubles(T, n, 0)


# ------------------------------------------------------------------------------------------------ object_entries
def _hand_table():
    """(2, 2, 23): threshold 20 with objects in both fields, threshold 30.5 with none in the forecast"""
    r = np.zeros((2, 2, 23), dtype=np.int64)
    # target at 20: 4 objects of areas 1, 3, 4, 16 over 2 frames (largest 16 and 3); 3 matched (3, 4, 16)
    r[0, 0, :6] = (4, 24, 1 + 9 + 16 + 256, 19, 3, 23)
    r[0, 0, 6:11] = (1, 1, 1, 0, 1)
    # forecast at 20: 2 objects of areas 8 and 20 (largest 20 and 8); 1 matched (20)
    r[1, 0, :6] = (2, 28, 64 + 400, 28, 1, 20)
    r[1, 0, 6:11] = (0, 0, 0, 1, 1)
    # target at 30.5: 1 object of area 2, unmatched; the forecast has none
    r[0, 1, :6] = (1, 2, 4, 2, 0, 0)
    r[0, 1, 7] = 1
    return r


def test_object_entries_on_a_hand_made_table():
    from adnm_hip.validate import object_entries
    e = object_entries(_hand_table(), 2, [20, 30.5], min_area=1)
    assert list(e) == ["min_area", 20, 30.5] and e["min_area"] == 1
    a = e[20]
    assert list(a) == ["target", "forecast", "count_bias", "size_bias", "object_POD", "object_FAR", "object_CSI", "size_bin_edges"]
    o, f = a["target"], a["forecast"]
    assert list(o) == ["count", "per_frame", "area", "mean_area", "weighted_area", "mean_largest", "matched", "matched_area", "size_histogram"]
    assert (o["count"], o["per_frame"], o["area"], o["mean_area"], o["weighted_area"], o["mean_largest"], o["matched"], o["matched_area"]) == \
        (4, 2.0, 24, 6.0, 282 / 24, 9.5, 3, 23)
    assert (f["count"], f["per_frame"], f["area"], f["mean_area"], f["weighted_area"], f["mean_largest"], f["matched"], f["matched_area"]) == \
        (2, 1.0, 28, 14.0, 464 / 28, 14.0, 1, 20)
    assert isinstance(o["count"], int) and isinstance(o["mean_area"], float)
    assert o["size_histogram"].dtype == np.int64 and o["size_histogram"].tolist() == [1, 1, 1, 0, 1] + [0] * 12
    assert a["count_bias"] == 0.5 and a["size_bias"] == (464 / 28) / (282 / 24) and a["object_POD"] == 0.75 and a["object_FAR"] == 0.5
    assert a["object_CSI"] == 3 / (4 + 2 - 1)
    assert a["size_bin_edges"].dtype == np.int64 and a["size_bin_edges"].tolist() == [2 ** k for k in range(17)]
    b = e[30.5]
    assert b["forecast"]["count"] == 0 and b["forecast"]["per_frame"] == 0.0 and b["forecast"]["mean_largest"] == 0.0
    assert all(math.isnan(b["forecast"][k]) for k in ("mean_area", "weighted_area")), "0 / 0 is NaN"
    assert b["count_bias"] == 0.0 and math.isnan(b["size_bias"]) and b["object_POD"] == 0.0 and math.isnan(b["object_FAR"]) and b["object_CSI"] == 0.0
    empty = object_entries(np.zeros((2, 1, 23)), 0, [20])[20]
    assert all(math.isnan(empty[k]) for k in ("count_bias", "size_bias", "object_POD", "object_FAR", "object_CSI"))
    assert math.isnan(empty["target"]["per_frame"]) and empty["target"]["count"] == 0


def test_object_entries_keeps_a_leading_axis_and_checks_its_rows():
    import torch
    from adnm_hip.validate import object_entries
    one = _hand_table()
    lead = object_entries(np.stack([one, 2 * one, 0 * one]).astype(np.float64), 2, [20, 30.5], min_area=3)
    assert lead["min_area"] == 3
    for i, mult in enumerate((1, 2, 0)):
        want = object_entries(mult * one, 2, [20, 30.5], min_area=3)
        for thr in (20, 30.5):
            got = {k: ({kk: vv[i] for kk, vv in v.items()} if isinstance(v, dict) else (v if k == "size_bin_edges" else v[i])) for k, v in lead[thr].items()}
            assert _same_tree(got, want[thr]), (i, thr)
    assert lead[20]["target"]["count"].dtype == np.int64 and lead[20]["target"]["size_histogram"].shape == (3, 17) and lead[20]["object_CSI"].shape == (3,)
    assert _same_tree(object_entries(torch.from_numpy(one), 2, [20, 30.5]), object_entries(one, 2, [20, 30.5]))
    for bad in (np.zeros((2, 3, 23)), np.zeros((2, 2, 22)), np.zeros((23,)), np.full((2, 2, 23), 0.5), np.full((2, 2, 23), np.nan), np.zeros((2, 2, 23), dtype=bool)):
        with pytest.raises(ValueError, match="objects"):
            object_entries(bad, 2, [20, 30.5])


# ------------------------------------------------------------------------------------------------ aggregate
T, THR, POOLS, FSS, FRAME, L = 3, [20, 30.5], ((4, 4), (16, 8)), (1, 5), (16, 32), 7
HW, AREA = FRAME[0] * FRAME[1], (FRAME[0] - 10) * (FRAME[1] - 10)
ALL = dict(pools=POOLS, persistence=True, fss=FSS, advection=True, spectrum=FRAME, joint=L)


@pytest.fixture(scope="module")
def full():
    """the block with every option on, integers (no two tables alike), and what aggregate makes of it"""
    from adnm_hip.validate import HEADER, aggregate, block_parts
    parts, total = block_parts(T, len(THR), objects=2, **ALL)
    blk = np.random.default_rng(23).integers(1, 1000, total).astype(np.float64)
    blk[:HEADER] = (12.5, 6, 12, 1)
    blk.setflags(write=False)
    return blk, {p.name: p for p in parts}, aggregate(blk, THR, T, HW, AREA, per_lead=True, objects=2, **ALL)


def test_aggregate_reads_the_objects_table_at_its_own_offset(full):
    from adnm_hip.validate import aggregate, block_parts, object_entries
    blk, whole, res = full
    assert list(inspect.signature(aggregate).parameters)[-2:] == ["objects", "joint"] and inspect.signature(aggregate).parameters["objects"].default is None
    me = whole["objects"]
    assert me.offset + me.size == blk.size, "the last part of the one allocation"
    tab = blk[me.offset:].reshape(T, 2, len(THR), 23)
    assert _same_tree(res["objects"], object_entries(tab.sum(axis=0), 12 * T, THR, 2)) and res["objects"]["min_area"] == 2
    assert _same_tree(res["per_lead"]["objects"], object_entries(tab, 12, THR, 2))
    assert res["objects"][20]["target"]["count"] == int(tab[:, 0, 0, 0].sum()) and res["objects"][30.5]["forecast"]["area"] == int(tab[:, 1, 1, 1].sum())
    assert (res["per_lead"]["objects"][20]["forecast"]["size_histogram"] == tab[:, 1, 0, 6:]).all()
    # cut down to main plus the objects table: the same entries, so nothing of them is read from another table
    parts, total = block_parts(T, len(THR), objects=2)
    cut = np.zeros(total)
    for p in parts:
        cut[p.offset:p.offset + p.size] = blk[whole[p.name].offset:whole[p.name].offset + p.size]
    alone = aggregate(cut, THR, T, HW, AREA, per_lead=True, objects=2)
    assert _same_tree(alone["objects"], res["objects"]) and _same_tree(alone["per_lead"]["objects"], res["per_lead"]["objects"])
    # and every former entry is what it is without the objects table
    former = aggregate(blk[:me.offset], THR, T, HW, AREA, per_lead=True, **ALL)
    assert list(res) == list(former)[:-1] + ["objects", "per_lead"] and list(res["per_lead"]) == list(former["per_lead"]) + ["objects"]
    assert list(res)[-3:] == ["joint", "objects", "per_lead"]
    assert _same_tree({k: res[k] for k in former if k != "per_lead"}, {k: former[k] for k in former if k != "per_lead"})
    assert _same_tree({k: res["per_lead"][k] for k in former["per_lead"]}, former["per_lead"])
    short = aggregate(blk, THR, T, HW, AREA, objects=2, **ALL)
    assert "per_lead" not in short and _same_tree(short["objects"], res["objects"])


def test_aggregate_refuses_a_block_of_another_length(full):
    from adnm_hip.validate import aggregate
    blk = full[0]
    with pytest.raises(ValueError, match="objects"):
        aggregate(blk[:-1], THR, T, HW, AREA, objects=2, **ALL)
    with pytest.raises(ValueError):
        aggregate(blk, THR, T, HW, AREA, **ALL)            # the block has an objects table, the options do not
    with pytest.raises(ValueError, match="objects"):
        aggregate(blk, THR, T, HW, AREA, objects=0.5, **ALL)


def test_validator_arguments():
    import torch
    from adnm_hip.validate import Validator
    from models.loss import enRainfallLoss
    sig = inspect.signature(Validator.__init__).parameters
    assert "objects" in sig and sig["objects"].default is None
    model, crit = torch.nn.Identity(), enRainfallLoss()
    plain = Validator(model, crit, 20, 90.0)
    assert plain.objects is None and [p.name for p in plain._parts] == ["main"]
    assert Validator(model, crit, 20, 90.0, objects=False).objects is None
    val = Validator(model, crit, 20, 90.0, objects=True)
    assert val.objects == 1 and [p.name for p in val._parts] == ["main", "objects"] and val._parts[-1].shape == (20, 2, 4, 23)
    assert Validator(model, crit, 20, 255.0, objects=9).objects == 9          # no limit on value_scale
    for bad in (0, -3, 1.5, "yes"):
        with pytest.raises(ValueError, match="objects"):
            Validator(model, crit, 20, 90.0, objects=bad)


def test_the_one_shot_wrappers_refuse_what_is_not_a_gpu_tensor():
    import torch
    a = torch.zeros(2, 8, 8)
    with pytest.raises(RuntimeError):
        ops.object_stats(a, a, (20,), 90.0)
    with pytest.raises(RuntimeError):
        ops.label_objects(a, 20, 90.0)
    with pytest.raises(RuntimeError):
        ops.label_objects(a.numpy(), 20, 90.0)


# ------------------------------------------------------------------------------------------------ the C boundary
def test_new_prototypes_are_declared_and_exported():
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/adnm_hip.h"
        assert hasattr(so, name), f"{name} declared but not exported"
    assert protos["adnm_valid_objects_block_bytes"] == ("int64_t", ["int64_t", "int64_t"])
    assert protos["adnm_valid_objects_accum_ws_bytes"] == ("int64_t", ["int64_t"] * 5)
    assert protos["adnm_label_objects_ws_bytes"] == ("int64_t", ["int64_t"] * 4)
    assert protos["adnm_valid_objects_accum"] == ("int", ["const float*", "int64_t", "int64_t", "const float*", "void*", "const float*", "int64_t", "float", "int64_t",
                                                          "void*", "int64_t", "int64_t", "int64_t", "int64_t", "int64_t", "adnm_stream_t"])
    assert protos["adnm_label_objects"] == ("int", ["const float*", "int64_t", "int64_t", "void*", "float", "float", "int64_t", "void*", "int64_t", "int64_t",
                                                    "int64_t", "int64_t", "int64_t", "adnm_stream_t"])


def test_the_queries_are_pure_host_functions_with_the_limits():
    """no GPU here: they answer all the same.  A frame of 65 536 pixels is inside, one of 65 537 outside."""
    q = lib.query
    blk, ws, lws = "adnm_valid_objects_block_bytes", "adnm_valid_objects_accum_ws_bytes", "adnm_label_objects_ws_bytes"
    assert q(blk, 20, 4) == 8 * 20 * 2 * 4 * 23 and q(blk, 1, 1) == 8 * 46 and q(blk, 3, 8) == 8 * 3 * 2 * 8 * 23
    assert [q(blk, *bad) for bad in ((0, 4), (-1, 4), (20, 0), (20, 9), (65536, 1))] == [-1] * 5
    for H, W in ((256, 256), (1, 65536), (65536, 1), (128, 512)):
        assert q(ws, 1, 1, H, W, 4) == 4 * 65536 * 4 and q(lws, 1, 1, H, W) == 4 * 65536, "the words of a frame at the limit live in the workspace"
    assert q(ws, 80, 20, 256, 256, 4) == 4 * 65536 * 320 and q(ws, 80, 20, 256, 256, 8) == 4 * 65536 * 512, "at most 512 workgroups"
    for H, W in ((65537, 1), (1, 65537), (257, 256), (256, 257), (0, 8), (8, 0), (-1, -1), (1 << 40, 1 << 40)):
        assert q(ws, 1, 1, H, W, 4) == -1 and q(lws, 1, 1, H, W) == -1, (H, W)
    for H, W in ((1, 1), (1, 7), (5, 3), (16, 16), (31, 33), (64, 64), (128, 128), (192, 200)):
        assert q(ws, 80, 20, H, W, 4) == 0 and q(lws, 80, 20, H, W) == 0, "the words of such a frame live in LDS"
    assert q(ws, 2, 1, 200, 200, 4) == 4 * 40000 * 8 and q(lws, 2, 1, 200, 200) == 4 * 40000 * 2
    for bad in ((0, 1), (3, 2), (65536, 1), (4, 0), (4, -2)):          # frames, T
        assert q(ws, *bad, 16, 16, 4) == -1 and q(lws, *bad, 16, 16) == -1, bad
    assert q(ws, 65535, 1, 16, 16, 8) == 0 and q(ws, 4, 2, 16, 16, 0) == -1 and q(ws, 4, 2, 16, 16, 9) == -1


def test_bad_arguments_are_refused_before_any_launch():
    """every check comes before the first launch, so the refusals can be seen without a GPU (the pointers are never followed)"""
    so = lib.load()
    thr = (ctypes.c_float * 2)(20.0, 30.0)
    ok = dict(pred=64, ss=256, fs=256, tgt=128, table=192, thr=thr, nthr=2, scale=90.0, min_area=1, ws=None, ws_bytes=0, frames=2, T=2, H=16, W=16)

    def accum(**kw):
        a = dict(ok, **kw)
        return so.adnm_valid_objects_accum(a["pred"], a["ss"], a["fs"], a["tgt"], a["table"], a["thr"], a["nthr"], a["scale"], a["min_area"], a["ws"], a["ws_bytes"],
                                           a["frames"], a["T"], a["H"], a["W"], None)
    for kw in (dict(pred=None), dict(tgt=None), dict(table=None), dict(thr=None), dict(pred=66), dict(tgt=130), dict(table=196), dict(ws=4), dict(nthr=0),
               dict(nthr=9), dict(min_area=0), dict(min_area=-5), dict(frames=3), dict(T=0), dict(frames=65536, T=1), dict(H=0), dict(W=0),
               dict(H=257, W=256), dict(fs=255), dict(fs=-256), dict(ss=-1), dict(H=256, W=256, fs=65536, ss=131072), dict(H=256, W=256, fs=65536, ss=131072, ws=256, ws_bytes=1023)):
        assert accum(**kw) != 0, kw
        assert "valid_objects_accum" in lib.last_error(), kw

    def label(**kw):
        a = dict(ok, **kw)
        return so.adnm_label_objects(a["pred"], a["ss"], a["fs"], a["table"], 20.0, a["scale"], a["min_area"], a["ws"], a["ws_bytes"], a["frames"], a["T"], a["H"],
                                     a["W"], None)
    for kw in (dict(pred=None), dict(table=None), dict(pred=66), dict(table=194), dict(ws=4), dict(min_area=0), dict(frames=3), dict(T=0), dict(H=0),
               dict(H=257, W=256), dict(fs=255), dict(ss=-1), dict(H=256, W=256, fs=65536, ss=131072)):
        assert label(**kw) != 0, kw
        assert "label_objects" in lib.last_error(), kw
