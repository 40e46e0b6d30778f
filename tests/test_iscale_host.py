"""The intensity-scale skill score without a GPU: the yardstick (iscale_ref) on a 4 x 4 pair worked by hand and its routes against one another,
ops.intensity_scale_levels, validate.block_tables with the three new rows in front of the tracks (block_layout and block_parts as they were),
validate.intensity_scale_entries on a hand-made table with its identities, validate.aggregate reading the tables at their own offsets, the
entry points at the C boundary (declared, exported, every limit refused on the host with its message) and the Validator's argument."""
import ctypes
import inspect
import math

import numpy as np
import pytest

import iscale_ref as R
from adnm_hip import lib, ops
from test_tracks_host import _same_tree   # bitwise, NaN equal to NaN, the keys in order

NEW = ("adnm_valid_iscale_block_bytes", "adnm_valid_iscale_accum_ws_bytes", "adnm_valid_iscale_accum")
KEYS = ["mse", "skill", "mse_share", "mse_total", "mse_random", "base_rate", "bias", "energy_target", "energy_forecast", "energy_rel_diff"]


# ------------------------------------------------------------------------------------------------ the yardstick, by hand
def _hand_pair():
    """4 x 4, P = 4, L = 2.  The target: the top-left 2 x 2 block and the pixel (3, 3); the forecast: the block moved two pixels to the right."""
    t, p = np.zeros((1, 4, 4), dtype=np.float32), np.zeros((1, 4, 4), dtype=np.float32)
    t[0, :2, :2], t[0, 3, 3], p[0, :2, 2:] = 0.9, 0.9, 0.9
    return t, p


def test_the_yardstick_on_a_pair_worked_by_hand():
    """level 0: 5 and 4 events, none in common.  Level 1 (2 x 2 blocks): the target's counts are 4, 0, 0, 1, the forecast's 0, 4, 0, 0.  Level 2
    (the domain): 5 and 4.  So D = A + F - 2 C = (9, 33, 1), and with N = 16 the components are (4*9 - 33) / 64, (4*33 - 1) / 256 and 4 / 1024:
    nearly all the error sits at scale 2, the distance the block was moved."""
    t, p = _hand_pair()
    assert R.levels(4, 4) == (4, 2) and R.levels(1, 1) == (1, 0) and R.levels(5, 7) == (8, 3) and R.levels(33, 32) == (64, 6) and R.levels(3, 1024) == (1024, 10)
    s = R.ref_sums(t, p, [30], 90.0)
    assert s.dtype == np.int64 and s.tolist() == [[[5, 4, 0], [17, 16, 0], [25, 16, 20]]]
    e = R.entries(s[0], 1, (4, 4), [30])[30]
    assert e["mse"].tolist() == [3 / 64, 131 / 256, 1 / 256] and e["mse_total"] == 9 / 16 == e["mse"].sum()
    assert e["energy_target"].tolist() == [3 / 64, 43 / 256, 25 / 256] and e["energy_target"].sum() == 5 / 16 == e["base_rate"]
    assert e["energy_forecast"].tolist() == [0.0, 48 / 256, 16 / 256] and e["bias"] == 0.8
    assert e["mse_random"] == 0.8 * (5 / 16) * (11 / 16) + (5 / 16) * (1 - 0.8 * 5 / 16)
    for z, want in ((p[0] > 0, e["energy_forecast"]), (t[0] > 0, e["energy_target"]), ((p[0] > 0).astype(int) - (t[0] > 0), e["mse"])):
        assert np.abs(R.haar_bands(z) - want).max() < 1e-15 and np.abs(R.nonstandard_bands(z) - want).max() < 1e-15
    h, lev = R.haar_matrix(4)
    assert lev.tolist() == [2, 1, 0, 0] and np.allclose(h[0], 0.5) and np.allclose(h[1], [0.5, 0.5, -0.5, -0.5]) and np.allclose(h[3] * math.sqrt(2), [0, 0, 1, -1])


def test_the_routes_of_the_yardstick_agree():
    """the block-sum form against the orthonormal 2-D Haar transform (H Z H^T with a band mask, and level by level).  The bar is derived, not
    measured: a component is a sum of at most 2^16 terms of magnitude <= 1 in double (relative error <= 2^16 * 2^-53 < 1e-11).  What was seen:
    profiles/iscale_error.txt (`python tests/iscale_ref.py` writes it)."""
    lines, worst = R.route_report()
    print("\n".join(lines), f"\nlargest deviation {worst:.3e}")
    assert len(lines) == len(R.ROUTE_CASES) and worst <= 1e-10
    t, p = R.radar_fields(3, 33, 20, 53, plant=True)
    s = R.ref_sums(t, p, R.THR, R.SCALE).sum(axis=0)
    assert (s[:, 0::3] > 0).all() and (s[:, 1::3] > 0).all() and (s[0, 0::3] + s[0, 1::3] > 2 * s[0, 2::3]).all(), "no event or no error: nothing was compared"
    for k, thr in enumerate(R.THR):      # every component >= 0 and the components sum to the whole
        e = R.entries(s, 3, (33, 20), R.THR)[thr]
        assert (e["mse"] >= 0).all() and abs(e["mse"].sum() - e["mse_total"]) < 1e-15 and abs(e["energy_target"].sum() - e["base_rate"]) < 1e-15


def test_the_patterns_are_what_their_names_say():
    c = R.checkerboard(2, 5, 7)
    assert c.shape == (2, 5, 7) and c[0, 0, 0] > 0 and c[0, 0, 1] == 0 and c[1, 1, 1] > 0
    full = R.checkerboard(1, 8, 8)     # the frame fills the domain: every 2 x 2 block holds 2 events, so every block mean from scale 2 up is 1/2
    s = R.ref_sums(full, np.zeros_like(full), [30], 90.0)[0]
    mse = R.components(s[:, 0] + s[:, 1] - 2 * s[:, 2], 1, 8)
    assert mse.tolist() == [0.25, 0.0, 0.0, 0.25], "a checkerboard against nothing: the error is its mean and a component of scale 1"
    h = R.half_plane(1, 4, 6)
    assert h[0, :, :3].all() and not h[0, :, 3:].any()
    f = np.arange(12, dtype=np.float32).reshape(1, 2, 6)
    assert R.shifted(f, 2)[0, 0].tolist() == [0, 0, 0, 1, 2, 3] and not R.shifted(f, 6).any()
    a, b = R.noise(2, 33, 65, 0.5, 1)
    assert 0.45 < (a > 0).mean() < 0.55 and 0.2 < ((a > 0) & (b > 0)).mean() < 0.3
    t, p = R.radar_fields(2, 24, 28, 3, plant=True)
    assert all(np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any() and (x < 0).any() and (x[np.isfinite(x)] > 1).any() for x in (t, p))


def test_a_shift_moves_the_error_to_coarser_scales():
    """the target against itself moved by 1, 2, 4, 8 and 16 px: the component with the largest MSE never moves to a finer scale and ends coarser"""
    t = R.radar_fields(4, 64, 64, 0)[0]
    peak = []
    for px in (1, 2, 4, 8, 16):
        s = R.ref_sums(t, R.shifted(t, px), [20], R.SCALE).sum(axis=0)
        peak.append(int(R.components(s[:, 0] + s[:, 1] - 2 * s[:, 2], 4, 64).argmax()))
    print("the scale index of the largest component per shift", peak)
    assert all(b >= a for a, b in zip(peak, peak[1:])) and peak[-1] > peak[0]


# ------------------------------------------------------------------------------------------------ intensity_scale_levels
def test_intensity_scale_levels():
    lv = ops.intensity_scale_levels
    assert [lv(*s) for s in ((1, 1), (1, 2), (1, 7), (5, 7), (32, 32), (33, 32), (96, 40), (128, 128), (3, 1024), (1024, 1024))] == \
        [(1, 0), (2, 1), (8, 3), (8, 3), (32, 5), (64, 6), (128, 7), (128, 7), (1024, 10), (1024, 10)]
    assert lv(np.int64(65), 63) == (128, 7) and all(isinstance(v, int) for v in lv(np.int64(65), 63))
    for H in range(1, 70):
        assert lv(H, 3) == R.levels(H, 3) == lv(3, H)
    for bad in ((0, 8), (8, 0), (1025, 1), (1, 1025), (-4, 4), (8.0, 8), (True, 8), (None, 8), ("8", 8)):
        with pytest.raises(ValueError, match="intensity_scale"):
            lv(*bad)


# ------------------------------------------------------------------------------------------------ the parts table
def test_the_rows_are_absent_by_default_and_stand_in_front_of_the_tracks():
    from adnm_hip.validate import Part, block_layout, block_parts, block_tables, iscale_doubles
    params = list(inspect.signature(block_tables).parameters)
    assert params[:8] == ["T", "nthr", "pools", "persistence", "fss", "advection", "spectrum", "joint"] and inspect.signature(block_tables).parameters["iscale"].default is None
    assert set(params[8:]) == {"sal", "nprob", "tracks", "objects", "iscale"}
    assert list(inspect.signature(block_layout).parameters) == [p for p in params if p != "iscale"], "block_layout keeps the parameter list it had"
    assert list(inspect.signature(block_parts).parameters) == [p for p in params if p not in ("iscale", "tracks")], "block_parts keeps the parameter list it had"
    T, n = 5, 3
    sal = ops.sal_spec(True)
    full = dict(pools=((4, 4),), persistence=True, fss=(1, 5), advection=True, spectrum=(16, 32), joint=7, objects=2, sal=sal, nprob=(1, 5))
    for kw in (dict(), dict(persistence=True), dict(advection=True, pools=(2,)), full):
        base = block_layout(T, n, **kw)
        assert block_tables(T, n, **kw) == base and block_parts(T, n, **kw) == base, "without the keyword: the parts there were"
        for none in (None, False, ()):
            assert block_tables(T, n, iscale=none, **kw) == base
        with_tracks = block_layout(T, n, tracks=1, **kw)
        assert block_tables(T, n, tracks=1, **kw) == with_tracks
        names = ["iscale"] + (["persistence/iscale"] if kw.get("persistence") else []) + (["advection/iscale"] if kw.get("advection") else [])
        fields = dict(zip(("iscale", "persistence/iscale", "advection/iscale"), ("pred", "last", "adv")))
        for frame, levels in (((96, 40), 8), ((1, 1), 1), ((3, 1024), 11)):
            on, total = block_tables(T, n, iscale=frame, **kw)
            assert on[:len(base[0])] == base[0], "a part moved"
            at = base[1]
            for part, name in zip(on[len(base[0]):], names):
                assert part == Part(name, "iscale", fields[name], (), (T, levels, 3 * n), at)
                at += T * levels * 3 * n
            assert len(on) == len(base[0]) + len(names) and total == at
            both, total2 = block_tables(T, n, iscale=frame, tracks=1, **kw)
            assert both[:-1] == on and both[-1] == with_tracks[0][-1]._replace(offset=at) and total2 == at + with_tracks[0][-1].size, "directly in front of the tracks"
            assert iscale_doubles(T, n, frame, kw.get("persistence", False), kw.get("advection", False)) == \
                tuple(T * levels * 3 * n if name in names else 0 for name in fields)
    assert iscale_doubles(T, n) == iscale_doubles(T, n, None, True, True) == (0, 0, 0)
    with pytest.raises(ValueError, match="intensity_scale"):
        block_tables(T, n, iscale=(1025, 1))


# ------------------------------------------------------------------------------------------------ intensity_scale_entries
def _hand_table():
    """(3, 6) for frames of 4 x 4 (L = 2), thresholds 20 and 30.5, two frames: at 20 the hand pair's sums and, as a second frame, a target of
    (0, 0) and (1, 1) against a forecast of the whole top row; at 30.5 the target's events of both frames and no forecast"""
    a = np.array([[5, 4, 0], [17, 16, 0], [25, 16, 20]]) + np.array([[2, 4, 1], [4, 8, 4], [4, 16, 8]])
    b = np.array([[7, 0, 0], [21, 0, 0], [29, 0, 0]])
    return np.concatenate([a, b], axis=1).astype(np.int64)


def test_intensity_scale_entries_on_a_hand_made_table():
    from adnm_hip.validate import intensity_scale_entries
    r = _hand_table()
    e = intensity_scale_entries(r, 2, (4, 4), [20, 30.5])
    assert list(e) == ["scale_px", "domain_px", "levels", 20, 30.5]
    assert e["scale_px"].tolist() == [1, 2, 4] and e["scale_px"].dtype == np.int64 and (e["domain_px"], e["levels"]) == (4, 2)
    a = e[20]
    assert list(a) == KEYS
    # D = (7 + 8 - 2, 21 + 24 - 8, 29 + 32 - 56) = (13, 37, 5), N = 32
    assert a["mse"].tolist() == [(52 - 37) / 128, (148 - 5) / 512, 20 / 2048] and a["mse_total"] == 13 / 32 and a["mse"].sum() == 13 / 32
    assert a["base_rate"] == 7 / 32 and a["bias"] == 8 / 7 and isinstance(a["mse_total"], float) and isinstance(a["bias"], float)
    rand = (8 / 7) * (7 / 32) * (25 / 32) + (7 / 32) * (1 - (8 / 7) * (7 / 32))
    assert a["mse_random"] == rand and np.array_equal(a["skill"], 1.0 - a["mse"] * 3 / rand) and np.array_equal(a["mse_share"], a["mse"] / (13 / 32))
    assert abs(a["skill"].mean() - (1 - a["mse_total"] / rand)) < 1e-15, "the mean skill over the scales is the skill of the whole"
    assert a["energy_target"].tolist() == [(28 - 21) / 128, (84 - 29) / 512, 116 / 2048] and a["energy_target"].sum() == 7 / 32
    assert a["energy_forecast"].tolist() == [(32 - 24) / 128, (96 - 32) / 512, 128 / 2048] and a["energy_forecast"].sum() == 8 / 32
    assert np.array_equal(a["energy_rel_diff"], (a["energy_forecast"] - a["energy_target"]) / (a["energy_forecast"] + a["energy_target"]))
    mine = R.entries(r, 2, (4, 4), [20, 30.5])
    for thr in (20, 30.5):
        for key in KEYS:
            assert np.allclose(e[thr][key], mine[thr][key], rtol=1e-15, atol=0), (thr, key)
    # a zero forecast: the error is the target, the forecast has no energy
    b = e[30.5]
    assert np.array_equal(b["mse"], b["energy_target"]) and (b["energy_forecast"] == 0).all() and (b["energy_rel_diff"] == -1).all()
    assert b["bias"] == 0.0 and b["mse_random"] == b["base_rate"] == 7 / 32 and b["mse_total"] == 7 / 32
    # pred == target: C = A = F
    same = intensity_scale_entries(np.array([[5, 5, 5], [17, 17, 17], [25, 25, 25]]), 1, (4, 4), [30])[30]
    assert (same["mse"] == 0).all() and (same["skill"] == 1).all() and same["mse_total"] == 0 and np.isnan(same["mse_share"]).all()
    assert (same["energy_rel_diff"] == 0).all() and same["bias"] == 1.0 and same["mse_random"] == 2 * (5 / 16) * (11 / 16)
    # nothing anywhere: every division is 0 / 0
    empty = intensity_scale_entries(np.zeros((3, 3)), 4, (4, 4), [30])[30]
    assert (empty["mse"] == 0).all() and empty["base_rate"] == 0 and all(np.isnan(empty[k]).all() for k in ("skill", "mse_share", "bias", "mse_random", "energy_rel_diff"))
    assert np.isnan(intensity_scale_entries(np.zeros((3, 3)), 0, (4, 4), [30])[30]["mse"]).all(), "no frame: NaN"
    # a leading axis: every row by itself, with its own number of frames
    lead = intensity_scale_entries(np.stack([r, 3 * r]), np.array([2, 6]), (4, 4), [20, 30.5])
    assert lead[20]["mse"].shape == (2, 3) and lead[20]["mse_total"].shape == (2,)
    for i in (0, 1):
        for key in KEYS:
            assert np.array_equal(np.asarray(lead[20][key])[i], np.asarray(a[key]), equal_nan=True), key
    # components are never negative, whatever the sums (4 D_j >= D_(j+1) for counts; the numerator is formed in integers)
    t, p = R.radar_fields(3, 13, 32, 2, plant=True)
    s = R.ref_sums(t, p, R.THR, R.SCALE)
    got = intensity_scale_entries(s, 1, (13, 32), R.THR)
    for k, thr in enumerate(R.THR):
        assert all((got[thr][key] >= 0).all() for key in ("mse", "energy_target", "energy_forecast")) and got[thr]["mse"].shape == (3, 6)
        fp_fn = s[:, 0, 3 * k] + s[:, 0, 3 * k + 1] - 2 * s[:, 0, 3 * k + 2]
        assert np.allclose(got[thr]["mse"].sum(axis=-1), fp_fn / 1024.0, rtol=1e-14, atol=0) and np.array_equal(got[thr]["mse_total"], fp_fn / 1024.0)


def test_intensity_scale_entries_checks_its_rows():
    import torch
    from adnm_hip.validate import intensity_scale_entries
    r = _hand_table()
    assert _same_tree(intensity_scale_entries(torch.from_numpy(r), 2, (4, 4), [20, 30.5]), intensity_scale_entries(r.astype(np.float64), 2, (4, 4), [20, 30.5]))
    for bad in (np.zeros((3, 3)), np.zeros((2, 6)), np.zeros((6,)), np.full((3, 6), 0.5), np.full((3, 6), np.nan), np.zeros((3, 6), dtype=bool), -np.ones((3, 6))):
        with pytest.raises(ValueError, match="intensity_scale"):
            intensity_scale_entries(bad, 2, (4, 4), [20, 30.5])
    with pytest.raises(ValueError, match="intensity_scale"):
        intensity_scale_entries(r, 2, (5, 4), [20, 30.5])           # L = 3: another table
    with pytest.raises(ValueError, match="intensity_scale"):
        intensity_scale_entries(r, 2, (1025, 4), [20, 30.5])


# ------------------------------------------------------------------------------------------------ aggregate
T, THR, FRAME = 3, [20, 30.5], (16, 32)
HW, AREA = FRAME[0] * FRAME[1], (FRAME[0] - 10) * (FRAME[1] - 10)
ALL = dict(pools=((4, 4), (16, 8)), persistence=True, fss=(1, 5), advection=True, spectrum=FRAME, joint=7, objects=2, nprob=(1, 3), sal=True)


def _counts_table(rng, frames):
    """(T, 6, 6) sums a field of FRAME could leave: per row the sums of `frames` random frame pairs"""
    out = np.zeros((T, 6, 3 * len(THR)), dtype=np.int64)
    for t in range(T):
        a, b = (rng.random((frames,) + FRAME) < 0.3).astype(np.float32) * 0.5, (rng.random((frames,) + FRAME) < 0.4).astype(np.float32) * 0.5
        out[t] = R.ref_sums(a, b, THR, 90.0).sum(axis=0)
    return out


def test_aggregate_reads_the_tables_at_their_own_offsets():
    from adnm_hip.validate import HEADER, aggregate, block_tables, intensity_scale_entries
    sig = inspect.signature(aggregate).parameters
    assert list(sig)[-2:] == ["objects", "joint"] and sig["intensity_scale"].default is None
    parts, total = block_tables(T, len(THR), tracks=2, iscale=FRAME, **dict(ALL, sal=ops.sal_spec(True)))
    assert [p.name for p in parts[-4:]] == ["iscale", "persistence/iscale", "advection/iscale", "tracks"] and parts[-1].offset + parts[-1].size == total
    rng = np.random.default_rng(31)
    blk = rng.integers(1, 1000, total).astype(np.float64)
    blk[:HEADER] = (12.5, 6, 12, 1)
    tabs = [_counts_table(rng, 12) for _ in range(3)]
    for part, tab in zip(parts[-4:-1], tabs):
        assert part.shape == tab.shape
        blk[part.offset:part.offset + part.size] = tab.ravel()
    from test_tracks_host import _hand_table as track_table
    blk[parts[-1].offset:] = track_table().ravel()
    res = aggregate(blk, THR, T, HW, AREA, per_lead=True, tracks=2, intensity_scale=FRAME, **ALL)
    for name, tab in zip(("forecast", "persistence", "advection"), tabs):
        got, lead = (res["intensity_scale"], res["per_lead"]["intensity_scale"]) if name == "forecast" else (res[name]["intensity_scale"], res["per_lead"][name]["intensity_scale"])
        assert _same_tree(got, intensity_scale_entries(tab.sum(axis=0), 36, FRAME, THR)), name
        assert _same_tree(lead, intensity_scale_entries(tab, 12, FRAME, THR)) and lead[20]["mse"].shape == (T, 6), name
    # every former entry is what it is without the tables, and the new ones stand in front of the tracks
    cut = np.concatenate([blk[:parts[-4].offset], blk[parts[-1].offset:]])
    former = aggregate(cut, THR, T, HW, AREA, per_lead=True, tracks=2, **ALL)
    assert list(res) == list(former)[:-2] + ["intensity_scale", "tracks", "per_lead"] and list(res["per_lead"]) == list(former["per_lead"]) + ["intensity_scale"]
    for name in ("persistence", "advection"):
        assert list(res[name]) == list(former[name]) + ["intensity_scale"] and list(res["per_lead"][name]) == list(former["per_lead"][name]) + ["intensity_scale"]
        res[name].pop("intensity_scale"), res["per_lead"][name].pop("intensity_scale")
    res["per_lead"].pop("intensity_scale")
    assert repr({k: res[k] for k in former}) == repr(former)
    # without a baseline only the forecast's table is there
    alone_parts, alone_total = block_tables(T, len(THR), iscale=FRAME)
    alone = np.zeros(alone_total)
    alone[:HEADER] = (12.5, 6, 12, 1)
    alone[alone_parts[-1].offset:] = tabs[0].ravel()
    only = aggregate(alone, THR, T, HW, AREA, intensity_scale=FRAME)
    assert list(only)[-1] == "intensity_scale" and _same_tree(only["intensity_scale"], intensity_scale_entries(tabs[0].sum(axis=0), 36, FRAME, THR))
    assert "per_lead" not in only and "intensity_scale" not in aggregate(alone[:alone_parts[-1].offset], THR, T, HW, AREA)
    with pytest.raises(ValueError, match="intensity_scale"):
        aggregate(blk[:-1], THR, T, HW, AREA, tracks=2, intensity_scale=FRAME, **ALL)
    with pytest.raises(ValueError):
        aggregate(blk, THR, T, HW, AREA, tracks=2, **ALL)            # the block has the tables, the options do not
    with pytest.raises(ValueError, match="intensity_scale"):
        aggregate(blk, THR, T, HW, AREA, intensity_scale=(2048, 16), **ALL)


def test_validator_arguments_and_nothing_new_when_unset():
    import torch
    from adnm_hip.validate import Validator, block_doubles
    from models.loss import enRainfallLoss
    sig = inspect.signature(Validator.__init__).parameters
    assert list(sig)[-1] == "joint" and sig["intensity_scale"].default is False
    model, crit = torch.nn.Identity(), enRainfallLoss()
    plain = Validator(model, crit, 20, 90.0)
    assert plain.intensity_scale is False and [p.name for p in plain._parts] == ["main"]
    assert plain._table((64, 64)) == plain._table(None) and plain._table((64, 64))[1] == block_doubles(20, 4)[0], "unset: nothing new in the block"
    val = Validator(model, crit, 20, 90.0, intensity_scale=True, persistence=True, advection=True, tracks=True)
    assert val.intensity_scale is True and [p.name for p in val._parts] == ["main", "persistence/pooled", "advection/pooled", "tracks"], "the tables come with the frames"
    parts, _ = val._table((96, 40))
    assert [p.name for p in parts] == ["main", "persistence/pooled", "advection/pooled", "iscale", "persistence/iscale", "advection/iscale", "tracks"]
    assert all(p.shape == (20, 8, 12) for p in parts[3:6]) and [p.field for p in parts[3:6]] == ["pred", "last", "adv"]
    with pytest.raises(ValueError, match="intensity_scale"):
        val._table((1025, 40))


def test_the_one_shot_wrapper_refuses_what_is_not_a_gpu_tensor():
    import torch
    a = torch.zeros(2, 3, 8, 8)
    with pytest.raises(RuntimeError):
        ops.intensity_scale_sums(a, a, (20,), 90.0)
    with pytest.raises(RuntimeError):
        ops.intensity_scale_sums(a.numpy(), a.numpy(), (20,), 90.0)


# ------------------------------------------------------------------------------------------------ the C boundary
def test_new_prototypes_are_declared_and_exported_and_the_abi_version_stays():
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/adnm_hip.h"
        assert hasattr(so, name), f"{name} declared but not exported"
    assert protos["adnm_valid_iscale_block_bytes"] == ("int64_t", ["int64_t"] * 4)
    assert protos["adnm_valid_iscale_accum_ws_bytes"] == ("int64_t", ["int64_t"] * 5) == protos["adnm_valid_objects_accum_ws_bytes"]
    fss = protos["adnm_valid_fss_accum"]
    assert protos["adnm_valid_iscale_accum"] == (fss[0], fss[1][:8] + fss[1][10:]), "adnm_valid_fss_accum's arguments without the scales"
    assert lib.load().adnm_abi_version() == 11
    text = open(lib.HEADER.replace("include/adnm_hip.h", "adnm-unet_amd/csrc/scored_pair.h")).read()
    assert "adnm_valid_iscale_accum" in text.split("#pragma once")[0], "the contract's comment lists its entry points"
    assert "2^13 frames" in open(lib.HEADER).read() and "2^25" in open(lib.HEADER).read(), "the header states how long the sums stay exact"


def test_the_queries_are_pure_host_functions_with_the_limits():
    q = lib.query
    blk, ws = "adnm_valid_iscale_block_bytes", "adnm_valid_iscale_accum_ws_bytes"
    assert q(blk, 20, 4, 128, 128) == 8 * 20 * 8 * 12 and q(blk, 1, 1, 1, 1) == 8 * 3 and q(blk, 3, 8, 3, 1024) == 8 * 3 * 11 * 24 and q(blk, 5, 2, 96, 40) == 8 * 5 * 8 * 6
    assert [q(blk, *bad) for bad in ((0, 4, 8, 8), (65536, 4, 8, 8), (20, 0, 8, 8), (20, 9, 8, 8), (20, 4, 0, 8), (20, 4, 8, 0), (20, 4, 1025, 8), (20, 4, 8, 1025))] == [-1] * 8
    # uint32 per (frame, tile): three sums per threshold for each of the levels 0 .. min(L, 5), and the tile's two counts per threshold
    assert q(ws, 80, 20, 128, 128, 4) == 80 * 16 * (3 * 6 + 2) * 4 * 4 and q(ws, 1, 1, 1, 1, 1) == (3 * 1 + 2) * 4 and q(ws, 6, 3, 5, 7, 4) == 6 * (3 * 4 + 2) * 4 * 4
    assert q(ws, 2, 1, 32, 32, 8) == 2 * 20 * 8 * 4 and q(ws, 2, 1, 33, 32, 8) == 2 * 2 * 20 * 8 * 4 and q(ws, 1, 1, 3, 1024, 2) == 32 * 20 * 2 * 4
    assert q(ws, 65535, 1, 1024, 1024, 8) == 65535 * 1024 * 20 * 8 * 4, "the largest call there is: 64-bit arithmetic"
    for H, W in ((0, 8), (8, 0), (1025, 1), (1, 1025), (-1, -1), (1 << 40, 1 << 40)):
        assert q(ws, 1, 1, H, W, 4) == -1, (H, W)
    for bad in ((0, 1), (3, 2), (65536, 1), (4, 0), (4, -2)):          # frames, T
        assert q(ws, *bad, 16, 16, 4) == -1, bad
    assert q(ws, 4, 2, 16, 16, 0) == -1 and q(ws, 4, 2, 16, 16, 9) == -1


def test_every_limit_is_refused_on_the_host_with_its_message():
    """every check comes before the first launch, so the refusals can be seen without a GPU (the pointers are never followed)"""
    so = lib.load()
    thr = (ctypes.c_float * 9)(*range(10, 19))
    ok = dict(pred=64, ss=512, fs=256, tgt=128, table=192, thr=thr, nthr=2, scale=90.0, ws=256, ws_bytes=1 << 40, frames=4, T=2, H=16, W=16)

    def accum(**kw):
        a = dict(ok, **kw)
        return so.adnm_valid_iscale_accum(a["pred"], a["ss"], a["fs"], a["tgt"], a["table"], a["thr"], a["nthr"], a["scale"], a["ws"], a["ws_bytes"], a["frames"],
                                          a["T"], a["H"], a["W"], None)
    need = lib.query("adnm_valid_iscale_accum_ws_bytes", 4, 2, 16, 16, 2)
    assert need == 4 * (3 * 5 + 2) * 2 * 4
    named = ((dict(H=0), -1, ("H and W must be in [1, 1024]", "0 x 16")),
             (dict(W=0), -1, ("H and W must be in [1, 1024]", "16 x 0")),
             (dict(H=1025, W=1, fs=1025, ss=2050), -1, ("H and W must be in [1, 1024]", "1025 x 1")),
             (dict(H=1, W=1025, fs=1025, ss=2050), -1, ("H and W must be in [1, 1024]", "1 x 1025")),
             (dict(nthr=0), -1, ("1..8 thresholds", "nthr 0")),
             (dict(nthr=9), -1, ("1..8 thresholds", "nthr 9")),
             (dict(frames=5), -1, ("T >= 1 must divide frames", "frames 5 T 2")),
             (dict(T=3), -1, ("T >= 1 must divide frames", "frames 4 T 3")),
             (dict(ws_bytes=need - 4), -3, (f"workspace {need - 4} < {need} bytes",)),
             (dict(ws=None), -3, ("workspace",)),
             (dict(ws=260), -1, ("the workspace must be 8-byte aligned",)),
             (dict(fs=255), -1, ("pred_frame_stride must be 0 or >= H*W", "255")),
             (dict(fs=-256), -1, ("pred_frame_stride must be 0 or >= H*W",)),
             (dict(ss=-1), -1, ("pred_sample_stride must be >= 0",)))
    for kw, rc, words in named:
        assert accum(**kw) == rc, (kw, lib.last_error())
        assert lib.last_error().startswith("valid_iscale_accum: ") and all(w in lib.last_error() for w in words), (kw, lib.last_error())
    for kw in (dict(pred=None), dict(tgt=None), dict(table=None), dict(thr=None), dict(pred=66), dict(tgt=130), dict(table=196), dict(T=0), dict(frames=65536, T=1),
               dict(ws_bytes=0), dict(ws_bytes=-1)):
        assert accum(**kw) != 0, kw
        assert "valid_iscale_accum" in lib.last_error(), kw
