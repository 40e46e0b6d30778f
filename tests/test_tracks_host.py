"""The track scores without a GPU: the yardstick (tracks_ref) on a 3 x 3 x 3 volume worked by hand, ops.tracks_spec and ops.track_cols,
validate.block_layout with the new row (and block_parts with the parameter list it had), validate.track_entries on a hand-made table with
its identities, validate.aggregate reading the tracks table at its own offset, and the entry points at the C boundary (declared, exported,
every limit refused on the host with its message)."""
import ctypes
import inspect
import math

import numpy as np
import pytest

import tracks_ref as R
from adnm_hip import lib, ops

NEW = ("adnm_valid_tracks_block_bytes", "adnm_valid_tracks_accum_ws_bytes", "adnm_valid_tracks_accum", "adnm_label_tracks_ws_bytes", "adnm_label_tracks")


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
    return _eq(a, b)


# ------------------------------------------------------------------------------------------------ the yardstick, by hand
def test_the_yardstick_on_a_volume_worked_by_hand():
    """a = (0,0,0) and b = (1,0,1) are neighbours (dt 1, dy 0, dx 1): one track of two voxels, label 1, frames 0..1.  d = (0,2,0) is two rows
    from both and c = (2,2,2) two rows from b and two frames from d: tracks of one voxel, labels 1 + 6 and 1 + 26.  The other field has an event
    at b only."""
    m = np.zeros((3, 3, 3), dtype=bool)
    m[0, 0, 0] = m[1, 0, 1] = m[0, 2, 0] = m[2, 2, 2] = True
    other = np.zeros_like(m)
    other[1, 0, 1] = True
    want = np.zeros((3, 3, 3), dtype=np.int32)
    want[0, 0, 0] = want[1, 0, 1] = 1
    want[0, 2, 0], want[2, 2, 2] = 7, 27
    assert (R.canonical(m) == want).all()
    assert (R.canonical(m, 2) == np.where(want == 1, 1, 0)).all()
    #                          N  v  v2 d  m  mv span  births     deaths     deaths0    hist
    assert R.row(m, other).tolist() == [3, 4, 6, 4, 1, 2, 0] + [2, 0, 1] + [1, 1, 1] + [1, 1, 0] + [2, 1, 0]
    assert R.row(m, other, 2).tolist() == [1, 2, 4, 2, 1, 2, 0] + [1, 0, 0] + [0, 1, 0] + [0, 1, 0] + [0, 1, 0]
    assert R.row(m, other, 3).tolist() == [0] * 19
    assert R.row(other, m).tolist() == [1, 1, 1, 1, 1, 1, 0] + [0, 1, 0] + [0, 1, 0] + [0, 0, 0] + [1, 0, 0]
    full = np.ones((3, 3, 3), dtype=bool)
    assert R.row(full, other).tolist() == [1, 27, 729, 3, 1, 27, 1] + [1, 0, 0] + [0, 0, 1] + [0, 0, 1] + [0, 0, 1]
    for r in (R.row(m, other), R.row(m, other, 2), R.row(full, other), R.row(other, m)):
        assert R.identities(r, 3)
    # with the centre voxel everything in a 3 x 3 x 3 volume is one track
    m[1, 1, 1] = True
    assert R.row(m, other)[:4].tolist() == [1, 5, 25, 3]


def test_the_patterns_are_what_their_names_say():
    from scipy import ndimage
    n = lambda v: ndimage.label(v > 0, structure=R.FULL)[1]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            assert n(R.mover(4, 9, 9, dy, dx)) == 1, "1 px per frame: one track"
            if dy or dx:
                assert n(R.mover(4, 9, 9, dy, dx, step=2)) == 4, "2 px per frame: a track per frame"
    assert n(R.serpentine3(4, 16, 16)) == 1 and n(R.spiral3(4, 16)) == 1
    assert n(R.lattice3(5, 7, 9)) == 3 * 4 * 5 and R.lattice3(5, 7, 9).sum() == 60
    assert n(R.fork(6, 8, 12)) == 2
    assert n(R.noise3(5, 33, 65, 0.2, 1)) < n(R.noise3(5, 33, 65, 0.08, 1))
    p = R.discs(2, 6, 24, 28, 3, plant=True)
    assert np.isnan(p).any() and np.isinf(p).any() and (p < 0).any() and (p > 1).any() and 0.5 < (R.discs(2, 6, 24, 28, 3) == 0).mean() < 0.99


# ------------------------------------------------------------------------------------------------ tracks_spec, track_cols
def test_tracks_spec():
    assert ops.tracks_spec(None) is None and ops.tracks_spec(False) is None
    assert ops.tracks_spec(True) == 1 and ops.tracks_spec(1) == 1 and ops.tracks_spec(9) == 9 and ops.tracks_spec(np.int64(4)) == 4
    assert isinstance(ops.tracks_spec(np.int64(4)), int)
    assert ops.tracks_spec(dict(min_volume=7)) == 7 and ops.tracks_spec({}) == 1
    for bad in (0, -1, 2.0, "3", (1,), [2], 1.5, float("nan"), dict(min_volume=0), dict(min_volume=True), dict(min_area=2), dict(min_volume=2.0)):
        with pytest.raises(ValueError, match="tracks"):
            ops.tracks_spec(bad)
    assert "65536" in ops.TRACK_LIMITS and "4194304" in ops.TRACK_LIMITS


def test_track_cols():
    C, at = ops.track_cols(20)
    assert C == 87 == R.cols(20)
    assert at == {"count": 0, "volume": 1, "volume2": 2, "duration": 3, "matched": 4, "matched_volume": 5, "spanning": 6, "births": 7, "deaths": 27,
                  "deaths0": 47, "duration_histogram": 67}
    assert ops.track_cols(1) == (11, dict(at, deaths=8, deaths0=9, duration_histogram=10))
    for bad in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="track_cols"):
            ops.track_cols(bad)


# ------------------------------------------------------------------------------------------------ the parts table
def test_the_row_is_absent_by_default_and_last_when_present():
    from adnm_hip.validate import HEADER, Part, block_layout, block_parts, tracks_doubles
    params = list(inspect.signature(block_parts).parameters)
    assert params[:8] == ["T", "nthr", "pools", "persistence", "fss", "advection", "spectrum", "joint"] and params[-1] == "objects"
    assert set(params[8:]) == {"sal", "nprob", "objects"}, "block_parts keeps the parameter list it had"
    lay = inspect.signature(block_layout).parameters
    assert list(lay)[:8] == params[:8] and list(lay)[-1] == "objects" and set(list(lay)[8:]) == {"sal", "nprob", "tracks", "objects"}
    assert lay["tracks"].default is None
    T, n = 5, 3
    sal = ops.sal_spec(True)
    for kw in (dict(), dict(nprob=(3, 1)), dict(pools=((4, 4),), persistence=True, fss=(1, 5), advection=True, spectrum=(16, 32), joint=7, objects=2, sal=sal,
                                                nprob=(1, 5))):
        base = block_parts(T, n, **kw)
        assert block_layout(T, n, **kw) == base
        for none in (None, False, 0):
            assert block_layout(T, n, tracks=none, **kw) == base, "the same parts as without the keyword"
        on, total = block_layout(T, n, tracks=1, **kw)
        assert on[:-1] == base[0], "a part moved"
        assert on[-1] == Part("tracks", "tracks", "pred", (), (2, n, 27), base[1]) and total == base[1] + 2 * n * 27
        assert block_layout(T, n, tracks=9, **kw) == (on, total), "min_volume does not change the table"
    assert block_layout(T, n)[0][0].size == HEADER + T * (4 * n + 3)
    assert tracks_doubles(T, n) == tracks_doubles(T, n, None) == tracks_doubles(T, n, False) == 0
    assert tracks_doubles(T, n, True) == tracks_doubles(T, n, dict(min_volume=4)) == 2 * n * 27 and tracks_doubles(20, 4, 5) == 2 * 4 * 87
    with pytest.raises(ValueError, match="tracks"):
        tracks_doubles(T, n, 0)


# ------------------------------------------------------------------------------------------------ track_entries
def _hand_table():
    """(2, 2, 19) for T = 3.  Threshold 20, target: tracks A (frames 0..2, 10 voxels, matched), B (frame 0, 1 voxel) and C (frames 1..2,
    4 voxels, matched); forecast: D (frames 0..1, 6 voxels, matched) and E (frame 2, 2 voxels).  Threshold 30.5: the target has one track
    (frame 1, 2 voxels), the forecast none."""
    r = np.zeros((2, 2, 19), dtype=np.int64)
    r[0, 0] = [3, 15, 117, 6, 2, 14, 1] + [2, 1, 0] + [1, 0, 2] + [1, 0, 1] + [1, 1, 1]
    r[1, 0] = [2, 8, 40, 3, 1, 6, 0] + [1, 0, 1] + [0, 1, 1] + [0, 1, 0] + [1, 1, 0]
    r[0, 1] = [1, 2, 4, 1, 0, 0, 0] + [0, 1, 0] + [0, 1, 0] + [0, 0, 0] + [1, 0, 0]
    return r


def test_the_hand_made_table_keeps_the_identities():
    r = _hand_table()
    for row in r.reshape(-1, 19):
        assert R.identities(row, 3)
    assert R.identities(r.sum(axis=(0, 1)), 3), "they are linear: sums of rows keep them"
    broken = r[0, 0].copy()
    broken[7] += 1
    assert not R.identities(broken, 3)


def test_track_entries_on_a_hand_made_table():
    from adnm_hip.validate import track_entries
    e = track_entries(_hand_table(), 2, [20, 30.5], 3, min_volume=1)
    assert list(e) == ["min_volume", 20, 30.5] and e["min_volume"] == 1
    a = e[20]
    assert list(a) == ["target", "forecast", "count_bias", "duration_bias", "survival_bias", "track_POD", "track_FAR", "track_CSI"]
    o, f = a["target"], a["forecast"]
    assert list(o) == ["count", "per_sample", "volume", "mean_volume", "weighted_volume", "mean_duration", "duration_histogram", "births", "deaths", "alive",
                       "initial", "survival", "spanning", "matched", "matched_volume"]
    assert (o["count"], o["per_sample"], o["volume"], o["mean_volume"], o["weighted_volume"], o["mean_duration"], o["initial"], o["spanning"], o["matched"],
            o["matched_volume"]) == (3, 1.5, 15, 5.0, 117 / 15, 2.0, 2, 1, 2, 14)
    assert (f["count"], f["per_sample"], f["volume"], f["mean_volume"], f["weighted_volume"], f["mean_duration"], f["initial"], f["spanning"], f["matched"],
            f["matched_volume"]) == (2, 1.0, 8, 4.0, 5.0, 1.5, 1, 0, 1, 6)
    assert isinstance(o["count"], int) and isinstance(o["mean_volume"], float)
    assert o["births"].tolist() == [2, 1, 0] and o["deaths"].tolist() == [1, 0, 2] and o["duration_histogram"].tolist() == [1, 1, 1]
    assert o["alive"].tolist() == [2, 2, 2] and f["alive"].tolist() == [1, 1, 1] and o["alive"].dtype == np.int64 == o["births"].dtype
    assert o["survival"].tolist() == [1.0, 0.5, 0.5] and f["survival"].tolist() == [1.0, 1.0, 0.0]
    assert a["count_bias"] == 2 / 3 and a["duration_bias"] == 0.75 and a["survival_bias"].tolist() == [1.0, 2.0, 0.0]
    assert a["track_POD"] == 2 / 3 and a["track_FAR"] == 0.5 and a["track_CSI"] == 2 / (3 + 2 - 1)
    b = e[30.5]
    assert b["forecast"]["count"] == 0 and b["forecast"]["per_sample"] == 0.0 and b["forecast"]["alive"].tolist() == [0, 0, 0]
    assert all(math.isnan(b["forecast"][k]) for k in ("mean_volume", "weighted_volume", "mean_duration")), "0 / 0 is NaN"
    assert np.isnan(b["forecast"]["survival"]).all() and np.isnan(b["target"]["survival"]).all(), "no initial track: NaN"
    assert b["target"]["initial"] == 0 and b["target"]["alive"].tolist() == [0, 1, 0]
    assert b["count_bias"] == 0.0 and math.isnan(b["duration_bias"]) and np.isnan(b["survival_bias"]).all()
    assert b["track_POD"] == 0.0 and math.isnan(b["track_FAR"]) and b["track_CSI"] == 0.0
    empty = track_entries(np.zeros((2, 1, 19)), 0, [20], 3)[20]
    assert all(math.isnan(empty[k]) for k in ("count_bias", "duration_bias", "track_POD", "track_FAR", "track_CSI")) and math.isnan(empty["target"]["per_sample"])


def test_track_entries_checks_its_rows():
    import torch
    from adnm_hip.validate import track_entries
    one = _hand_table()
    assert _same_tree(track_entries(torch.from_numpy(one), 2, [20, 30.5], 3), track_entries(one.astype(np.float64), 2, [20, 30.5], 3))
    for bad in (np.zeros((2, 3, 19)), np.zeros((2, 2, 18)), np.zeros((3, 2, 2, 19)), np.full((2, 2, 19), 0.5), np.full((2, 2, 19), np.nan),
                np.zeros((2, 2, 19), dtype=bool)):
        with pytest.raises(ValueError, match="tracks"):
            track_entries(bad, 2, [20, 30.5], 3)
    with pytest.raises(ValueError):
        track_entries(one, 2, [20, 30.5], 4)


# ------------------------------------------------------------------------------------------------ aggregate
T, THR, FRAME = 3, [20, 30.5], (16, 32)
HW, AREA = FRAME[0] * FRAME[1], (FRAME[0] - 10) * (FRAME[1] - 10)
ALL = dict(pools=((4, 4), (16, 8)), persistence=True, fss=(1, 5), advection=True, spectrum=FRAME, joint=7, objects=2, nprob=(1, 3))


def test_aggregate_reads_the_tracks_table_at_its_own_offset():
    from adnm_hip.validate import HEADER, aggregate, block_layout, track_entries
    sig = inspect.signature(aggregate).parameters
    assert list(sig)[-2:] == ["objects", "joint"] and sig["tracks"].default is None
    parts, total = block_layout(T, len(THR), tracks=2, **ALL)
    blk = np.random.default_rng(29).integers(1, 1000, total).astype(np.float64)
    blk[:HEADER] = (12.5, 6, 12, 1)
    me = parts[-1]
    assert me.name == "tracks" and me.offset + me.size == total, "the last part of the one allocation"
    blk[me.offset:] = np.stack([_hand_table(), 3 * _hand_table()]).sum(axis=0).ravel()
    res = aggregate(blk, THR, T, HW, AREA, per_lead=True, tracks=2, **ALL)
    assert _same_tree(res["tracks"], track_entries(4 * _hand_table(), 12, THR, T, 2)) and res["tracks"]["min_volume"] == 2
    former = aggregate(blk[:me.offset], THR, T, HW, AREA, per_lead=True, **ALL)
    assert list(res) == list(former)[:-1] + ["tracks", "per_lead"], "behind every other option's entries"
    assert list(res["per_lead"]) == list(former["per_lead"]), "the arrays are per lead time already: per_lead adds nothing for tracks"
    assert repr({k: res[k] for k in former}) == repr(former), "every former entry is what it is without the tracks table"
    with pytest.raises(ValueError, match="tracks"):
        aggregate(blk[:-1], THR, T, HW, AREA, tracks=2, **ALL)
    with pytest.raises(ValueError):
        aggregate(blk, THR, T, HW, AREA, **ALL)            # the block has a tracks table, the options do not
    with pytest.raises(ValueError, match="tracks"):
        aggregate(blk, THR, T, HW, AREA, tracks=0.5, **ALL)


def test_validator_arguments():
    import torch
    from adnm_hip.validate import Validator
    from models.loss import enRainfallLoss
    sig = inspect.signature(Validator.__init__).parameters
    assert "tracks" in sig and sig["tracks"].default is None
    model, crit = torch.nn.Identity(), enRainfallLoss()
    plain = Validator(model, crit, 20, 90.0)
    assert plain.tracks is None and [p.name for p in plain._parts] == ["main"]
    assert Validator(model, crit, 20, 90.0, tracks=False).tracks is None
    val = Validator(model, crit, 20, 90.0, tracks=True, objects=True)
    assert val.tracks == 1 and [p.name for p in val._parts] == ["main", "objects", "tracks"] and val._parts[-1].shape == (2, 4, 87)
    assert Validator(model, crit, 20, 255.0, tracks=dict(min_volume=9)).tracks == 9
    for bad in (0, -3, 1.5, "yes", dict(volume=3)):
        with pytest.raises(ValueError, match="tracks"):
            Validator(model, crit, 20, 90.0, tracks=bad)


def test_the_one_shot_wrappers_refuse_what_is_not_a_gpu_tensor():
    import torch
    a = torch.zeros(2, 3, 8, 8)
    with pytest.raises(RuntimeError):
        ops.track_stats(a, a, (20,), 90.0)
    with pytest.raises(RuntimeError):
        ops.label_tracks(a, 20, 90.0)
    with pytest.raises(RuntimeError):
        ops.label_tracks(a.numpy(), 20, 90.0)


# ------------------------------------------------------------------------------------------------ the C boundary
def test_new_prototypes_are_declared_and_exported_and_the_abi_version_stays():
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/adnm_hip.h"
        assert hasattr(so, name), f"{name} declared but not exported"
    assert protos["adnm_valid_tracks_block_bytes"] == ("int64_t", ["int64_t", "int64_t"])
    assert protos["adnm_valid_tracks_accum_ws_bytes"] == protos["adnm_valid_objects_accum_ws_bytes"]
    assert protos["adnm_label_tracks_ws_bytes"] == protos["adnm_label_objects_ws_bytes"]
    assert protos["adnm_valid_tracks_accum"] == protos["adnm_valid_objects_accum"], "the argument list is adnm_valid_objects_accum's"
    assert protos["adnm_label_tracks"] == protos["adnm_label_objects"]
    assert lib.load().adnm_abi_version() == 11


def _bytes(frames, hw, fields):
    return fields * frames * 4 * (3 * hw + 2 * ((hw + 63) // 64))


def test_the_queries_are_pure_host_functions_with_the_limits():
    q = lib.query
    blk, ws, lws = "adnm_valid_tracks_block_bytes", "adnm_valid_tracks_accum_ws_bytes", "adnm_label_tracks_ws_bytes"
    assert q(blk, 20, 4) == 8 * 2 * 4 * 87 and q(blk, 1, 1) == 8 * 2 * 11 and q(blk, 3, 8) == 8 * 2 * 8 * 19
    assert [q(blk, *bad) for bad in ((0, 4), (-1, 4), (20, 0), (20, 9), (65536, 1))] == [-1] * 5
    # three words a voxel and a bit plane a frame, padded to whole ballots, per chain; all thresholds at once while that stays within 256 MB
    assert q(ws, 80, 20, 128, 128, 4) == 4 * _bytes(80, 16384, 2) == 127139840 and q(lws, 80, 20, 128, 128) == _bytes(80, 16384, 1)
    assert q(ws, 80, 20, 256, 256, 4) == 2 * _bytes(80, 65536, 2) <= 256 << 20 < 3 * _bytes(80, 65536, 2), "two thresholds per chunk"
    assert q(ws, 80, 20, 256, 256, 1) == _bytes(80, 65536, 2) and q(ws, 640, 64, 256, 256, 8) == _bytes(640, 65536, 2), "at least one threshold"
    assert q(ws, 3, 3, 33, 65, 2) == 2 * _bytes(3, 2145, 2) and q(lws, 6, 3, 1, 1) == 6 * 4 * 5
    for H, W in ((65537, 1), (1, 65537), (257, 256), (256, 257), (0, 8), (8, 0), (-1, -1), (1 << 40, 1 << 40)):
        assert q(ws, 1, 1, H, W, 4) == -1 and q(lws, 1, 1, H, W) == -1, (H, W)
    assert q(ws, 64, 64, 256, 256, 4) > 0 and q(lws, 64, 64, 256, 256) > 0, "T * H * W = 2^22 is inside"
    assert q(ws, 65, 65, 256, 256, 4) == -1 and q(lws, 65, 65, 256, 256) == -1 and q(ws, 130, 65, 256, 256, 4) == -1, "2^22 + H * W is outside"
    assert q(ws, 65, 1, 256, 256, 4) > 0, "the limit is on a sample's volume, not on the batch"
    for bad in ((0, 1), (3, 2), (65536, 1), (4, 0), (4, -2)):          # frames, T
        assert q(ws, *bad, 16, 16, 4) == -1 and q(lws, *bad, 16, 16) == -1, bad
    assert q(ws, 65535, 1, 16, 16, 8) > 0 and q(ws, 4, 2, 16, 16, 0) == -1 and q(ws, 4, 2, 16, 16, 9) == -1


def test_every_limit_is_refused_on_the_host_with_its_message():
    """every check comes before the first launch, so the refusals can be seen without a GPU (the pointers are never followed)"""
    so = lib.load()
    thr = (ctypes.c_float * 9)(*range(10, 19))
    ok = dict(pred=64, ss=512, fs=256, tgt=128, table=192, thr=thr, nthr=2, scale=90.0, min_volume=1, ws=256, ws_bytes=1 << 40, frames=4, T=2, H=16, W=16)

    def accum(**kw):
        a = dict(ok, **kw)
        return so.adnm_valid_tracks_accum(a["pred"], a["ss"], a["fs"], a["tgt"], a["table"], a["thr"], a["nthr"], a["scale"], a["min_volume"], a["ws"], a["ws_bytes"],
                                          a["frames"], a["T"], a["H"], a["W"], None)
    need = lib.query("adnm_valid_tracks_accum_ws_bytes", 4, 2, 16, 16, 2)
    named = ((dict(H=257, W=256, fs=65792, ss=131584), ("1 <= H * W <= 65536", "H 257 W 256")),
             (dict(frames=65, T=65, H=256, W=256, fs=65536, ss=65 * 65536), ("T * H * W <= 4194304", "T 65 H 256 W 256")),
             (dict(nthr=9), ("1..8 thresholds", "nthr 9")),
             (dict(min_volume=0), ("min_volume >= 1", "min_volume 0")),
             (dict(frames=5), ("T >= 1 must divide frames", "frames 5 T 2")),
             (dict(ws_bytes=need - 4), (f"workspace {need - 4} < {need} bytes",)),
             (dict(ws=None), ("workspace",)))
    for kw, words in named:
        assert accum(**kw) != 0, kw
        assert lib.last_error().startswith("valid_tracks_accum: ") and all(w in lib.last_error() for w in words), (kw, lib.last_error())
    for kw in (dict(pred=None), dict(tgt=None), dict(table=None), dict(thr=None), dict(pred=66), dict(tgt=130), dict(table=196), dict(ws=260), dict(nthr=0),
               dict(min_volume=-5), dict(T=0), dict(frames=65536, T=1), dict(H=0), dict(W=0), dict(fs=255), dict(fs=-256), dict(ss=-1), dict(ws_bytes=0)):
        assert accum(**kw) != 0, kw
        assert "valid_tracks_accum" in lib.last_error(), kw

    def label(**kw):
        a = dict(ok, **kw)
        return so.adnm_label_tracks(a["pred"], a["ss"], a["fs"], a["table"], 20.0, a["scale"], a["min_volume"], a["ws"], a["ws_bytes"], a["frames"], a["T"], a["H"],
                                    a["W"], None)
    lneed = lib.query("adnm_label_tracks_ws_bytes", 4, 2, 16, 16)
    for kw, words in ((dict(H=257, W=256, fs=65792, ss=131584), ("1 <= H * W <= 65536", "H 257 W 256")),
                      (dict(frames=65, T=65, H=256, W=256, fs=65536, ss=65 * 65536), ("T * H * W <= 4194304", "T 65")),
                      (dict(min_volume=0), ("min_volume >= 1", "got 0")), (dict(frames=5), ("T >= 1 must divide frames", "frames 5 T 2")),
                      (dict(ws_bytes=lneed - 4), (f"workspace {lneed - 4} < {lneed} bytes",))):
        assert label(**kw) != 0, kw
        assert lib.last_error().startswith("label_tracks: ") and all(w in lib.last_error() for w in words), (kw, lib.last_error())
    for kw in (dict(pred=None), dict(table=None), dict(ws=None), dict(pred=66), dict(table=194), dict(ws=260), dict(T=0), dict(H=0), dict(fs=255), dict(ss=-1)):
        assert label(**kw) != 0, kw
        assert "label_tracks" in lib.last_error(), kw
