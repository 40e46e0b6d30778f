"""The SAL scores without a GPU: the yardstick (sal_ref) on fields with strict expectations and on two hand-computed cases, ops.sal_spec and
ops.sal_weights, validate.sal_entries on a hand-made table, validate.block_parts with the new row for every on/off combination of the other
options, validate.aggregate reading the SAL table at its own offset, and the entry points at the C boundary (declared, exported, the queries
pure host functions that refuse every limit, bad arguments refused before any launch; pair_check's cases repeated for the new entry point)."""
import ctypes
import inspect
import itertools
import math

import numpy as np
import pytest
from scipy import ndimage

import sal_ref as S
from adnm_hip import lib, ops
from test_joint_host import _same_tree   # bitwise, NaN equal to NaN, the keys in order

NEW = ("adnm_valid_sal_block_bytes", "adnm_valid_sal_accum_ws_bytes", "adnm_valid_sal_accum", "adnm_object_moments_ws_bytes", "adnm_object_moments")
SCALE = 90.0


def _levels(q):
    """integer levels -> a float32 field that quantises to them at SCALE (the middle of each level's interval)"""
    return ((np.asarray(q, dtype=np.float64) + 0.5) / SCALE * (np.asarray(q) > 0)).astype(np.float32)


def _shift(a, dy, dx):
    out = np.zeros_like(a)
    H, W = a.shape
    out[dy:, dx:] = a[:H - dy, :W - dx]
    return out


# ------------------------------------------------------------------------------------------------ the yardstick, strict conditions
@pytest.fixture(scope="module")
def blobs():
    t = S.blobs(64, 64, 6, seed=0, margin=20)
    assert len(S.objects(t, 20, SCALE)) >= 2 and t.max() < 1.0
    return t


def test_a_forecast_equal_to_the_target_scores_exact_zeros(blobs):
    s = S.scores(blobs, blobs.copy(), 20, SCALE)
    assert (s["A"], s["S"], s["L1"], s["L2"], s["L"]) == (0.0, 0.0, 0.0, 0.0, 0.0) and not s["only_target"] and not s["only_forecast"]
    assert S.row(blobs, blobs, 20, SCALE).tolist() == [1, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0]


def test_a_shifted_forecast_moves_l1_only(blobs):
    moved = _shift(blobs, 3, 5)
    assert S.mass(S.weights(moved, SCALE))[0] == S.mass(S.weights(blobs, SCALE))[0] > 0, "no mass leaves the frame"
    s = S.scores(blobs, moved, 20, SCALE)
    assert s["A"] == 0.0 and s["S"] == 0.0 and abs(s["L2"]) <= 1e-12
    assert abs(s["L1"] - math.hypot(3, 5) / math.hypot(64, 64)) <= 1e-12 and abs(s["L1"] - 0.0644235254) < 1e-9


def test_a_zero_forecast_has_amplitude_minus_two_and_nothing_else(blobs):
    s = S.scores(blobs, np.zeros_like(blobs), 20, SCALE)
    assert s["A"] == -2.0 and s["S"] is None and s["L1"] is None and s["L2"] is None and s["L"] is None and s["only_target"] and not s["only_forecast"]
    assert S.row(blobs, np.zeros_like(blobs), 20, SCALE).tolist() == [1, -2, 2, 0, 0, 0, 0, 0, 0, 0, 1, 0]
    assert S.row(np.zeros_like(blobs), blobs, 20, SCALE).tolist() == [1, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    assert S.row(np.zeros_like(blobs), np.zeros_like(blobs), 20, SCALE).tolist() == [0] * 12


def test_a_smoothed_forecast_has_positive_structure_and_a_scaled_one_positive_amplitude(blobs):
    smooth = ndimage.gaussian_filter(blobs.astype(np.float64), 3).astype(np.float32)
    s = S.scores(blobs, smooth, 20, SCALE)
    assert s["S"] > 0 and abs(s["A"]) < 0.05, s
    assert S.scores(blobs, np.clip(blobs * 1.3, 0, 1), 20, SCALE)["A"] > 0


def test_a_hand_computed_row_of_four_pixels():
    """target levels 0 30 60 0: one object R 90, Q 60, X 150; forecast 45 0 0 45: two objects R 45, Q 45 at x = 0 and 3"""
    t, p = _levels([[0, 30, 60, 0]]), _levels([[45, 0, 0, 45]])
    assert S.objects(t, 20, SCALE) == [(1, 2, 90, 60, 150, 0)] and S.objects(p, 20, SCALE) == [(0, 1, 45, 45, 0, 0), (3, 1, 45, 45, 135, 0)]
    assert S.mass(S.weights(t, SCALE)) == (90, 150, 0) and S.mass(S.weights(p, SCALE)) == (90, 135, 0)
    assert S.moments(t, 20, SCALE).tolist() == [[[0, 90, 0, 0]], [[0, 60, 0, 0]], [[0, 150, 0, 0]], [[0, 0, 0, 0]]]
    d = math.sqrt(17)
    s = S.scores(t, p, 20, SCALE)
    # V_o = 90 * (90 / 60) / 90 = 1.5, V_f = 1; r_o = 0, r_f = 1.5 (both objects 1.5 from the centre 1.5); c_o = 5 / 3
    assert s["A"] == 0.0 and s["S"] == pytest.approx(-0.4, abs=1e-15) and s["L1"] == pytest.approx((5 / 3 - 1.5) / d, abs=1e-15)
    assert s["L2"] == pytest.approx(3 / d, abs=1e-15) and s["L"] == s["L1"] + s["L2"]
    ones = S.scores(t, p, 20, SCALE, intensity=[0] * 20 + [1] * 71)          # every event weighs 1: R is the area, Q is 1
    assert S.objects(t, 20, SCALE, intensity=[0] * 20 + [1] * 71) == [(1, 2, 2, 1, 3, 0)]
    assert ones["A"] == 0.0 and ones["S"] == pytest.approx((1 - 2) / 1.5, abs=1e-15) and ones["L1"] == 0.0


def test_a_hand_computed_three_by_three():
    """target: a diagonal pair of 50s (one object under 8-connectivity) and a 10 below the threshold that still has mass; forecast: one 40"""
    t, p = _levels([[50, 0, 0], [0, 50, 0], [0, 0, 10]]), _levels([[0, 0, 0], [0, 0, 0], [0, 0, 40]])
    assert S.objects(t, 20, SCALE) == [(0, 2, 100, 50, 50, 50)] and S.objects(p, 20, SCALE) == [(8, 1, 40, 40, 80, 80)]
    assert S.mass(S.weights(t, SCALE)) == (110, 70, 70)
    s = S.scores(t, p, 20, SCALE)
    assert s["A"] == pytest.approx(-14 / 15, abs=1e-15) and s["L1"] == pytest.approx(5 / 11, abs=1e-15)
    assert s["S"] == pytest.approx(-2 / 3, abs=1e-15) and s["L2"] == pytest.approx(1 / 11, abs=1e-15)
    two = S.row(t, p, 20, SCALE, min_area=2)          # the forecast's one pixel is ignored: only the target has an object
    assert two[[0, 3, 5, 10, 11]].tolist() == [1, 1, 0, 1, 0] and two[1] == pytest.approx(-14 / 15) and (two[6:10] == 0).all()
    zero_weight = S.row(t, p, 20, SCALE, intensity=[0] * 45 + list(range(45, 91)))          # the 40 weighs nothing: no mass, no object
    assert zero_weight[[0, 3, 5, 10, 11]].tolist() == [1, 0, 0, 1, 0] and zero_weight[1] == -2.0


def test_fold_adds_the_batch_sum_once():
    rows = np.random.default_rng(3).random((6, 2, 12))
    onto = np.random.default_rng(4).random((3, 2, 12))
    got = S.fold(rows, 3, onto)
    assert (got == onto + ((0.0 + rows[:3]) + rows[3:])).all() and (S.fold(rows, 3) == rows[:3] + rows[3:]).all()


# ------------------------------------------------------------------------------------------------ sal_spec, sal_weights
def test_sal_spec():
    assert ops.sal_spec(None) is None and ops.sal_spec(False) is None
    assert ops.sal_spec(True) == (1, None) and ops.sal_spec(1) == (1, None) and ops.sal_spec(9) == (9, None) and ops.sal_spec(np.int64(4)) == (4, None)
    assert ops.sal_spec(dict(min_area=3)) == (3, None) and ops.sal_spec(dict()) == (1, None) and ops.sal_spec(dict(intensity=None)) == (1, None)
    assert ops.sal_spec(dict(min_area=2, intensity=[0, 5, 7])) == (2, (0, 5, 7)) and ops.sal_spec(dict(intensity=np.arange(3))) == (1, (0, 1, 2))
    assert ops.sal_spec(dict(intensity=[1] * 7)) == (1, (1,) * 7), "the table's length is checked against a value_scale later"
    for bad in (0, -1, 2.0, "3", (1,), [2], 1.5, float("nan"), dict(min_area=0), dict(min_area=True), dict(min_area=1.0), dict(area=2),
                dict(intensity="abc"), dict(min_area=2, weights=[1])):
        with pytest.raises(ValueError, match="sal"):
            ops.sal_spec(bad)
    assert ops.SAL_COLS == 12 == S.COLS


def test_sal_weights_checks_the_table_against_the_value_scale():
    assert ops.sal_weights(None, 90.0) is None and ops.sal_levels(90.0) == 91 and ops.sal_levels(1.0) == 2 and ops.sal_levels(255.9) == 256
    tab = ops.sal_weights(list(range(90)) + [65535], 90.0)
    assert len(tab) == 91 and tab[90] == 65535 and tab[7] == 7 and ctypes.sizeof(tab) == 182
    assert list(ops.sal_weights(np.arange(3), 2.5)) == [0, 1, 2]
    for bad_table in (list(range(90)), list(range(92)), [0.5] * 91, [65536] + [0] * 90, [-1] + [0] * 90, [True] * 91):
        with pytest.raises(ValueError, match="intensity"):
            ops.sal_weights(bad_table, 90.0)
    for bad_scale in (0.5, 0.0, -3.0, 256.0, 256.5, 1e9, float("nan"), float("inf"), None, "x"):
        with pytest.raises(ValueError, match="value_scale"):
            ops.sal_weights(None, bad_scale)


# ------------------------------------------------------------------------------------------------ sal_entries
def _hand_table():
    """(2, 12): threshold 20 over 4 frames, threshold 30.5 where no frame has objects in both fields"""
    r = np.zeros((2, 12))
    r[0] = (4, 0.5, 1.5, 3, 0.75, 2, -0.5, 1.0, 0.25, 0.5, 1, 1)
    r[1] = (4, 0.5, 1.5, 3, 0.75, 0, 0, 0, 0, 0, 3, 0)
    return r


def test_sal_entries_on_a_hand_made_table():
    from adnm_hip.validate import sal_entries
    e = sal_entries(_hand_table(), [20, 30.5], (2, (0, 1, 2)))
    assert list(e) == ["min_area", "intensity", 20, 30.5] and e["min_area"] == 2 and e["intensity"] == (0, 1, 2)
    a = e[20]
    assert list(a) == ["A", "abs_A", "S", "abs_S", "L1", "L2", "L", "frames_A", "frames_L1", "frames_S", "missed_frames", "false_frames"]
    assert (a["A"], a["abs_A"], a["S"], a["abs_S"], a["L1"], a["L2"], a["L"]) == (0.125, 0.375, -0.25, 0.5, 0.25, 0.125, 0.25)
    assert (a["frames_A"], a["frames_L1"], a["frames_S"], a["missed_frames"], a["false_frames"]) == (4, 3, 2, 1, 1)
    assert isinstance(a["frames_A"], int) and isinstance(a["A"], float)
    b = e[30.5]
    assert b["A"] == 0.125 and b["L1"] == 0.25 and all(math.isnan(b[k]) for k in ("S", "abs_S", "L2", "L")), "a mean over no frame is NaN"
    assert (b["frames_S"], b["missed_frames"], b["false_frames"]) == (0, 3, 0)
    empty = sal_entries(np.zeros((1, 12)), [20])
    assert empty["min_area"] == 1 and empty["intensity"] is None
    assert all(math.isnan(empty[20][k]) for k in ("A", "abs_A", "S", "abs_S", "L1", "L2", "L")) and empty[20]["frames_A"] == 0


def test_sal_entries_keeps_a_leading_axis_and_checks_its_rows():
    import torch
    from adnm_hip.validate import sal_entries
    one = _hand_table()
    lead = sal_entries(np.stack([one, 2 * one, 0 * one]), [20, 30.5])
    for i, mult in enumerate((1, 2, 0)):
        want = sal_entries(mult * one, [20, 30.5])
        for thr in (20, 30.5):
            assert _same_tree({k: np.asarray(v[i]).item() for k, v in lead[thr].items()}, want[thr]), (i, thr)
    assert lead[20]["frames_A"].dtype == np.int64 and lead[20]["S"].shape == (3,) and math.isnan(lead[20]["S"][2])
    assert _same_tree(sal_entries(torch.from_numpy(one), [20, 30.5]), sal_entries(one, [20, 30.5]))
    half = one.copy()
    half[0, 5] = 1.5
    for bad in (np.zeros((3, 12)), np.zeros((2, 11)), np.zeros((12,)), half, np.full((2, 12), np.nan), -one):
        with pytest.raises(ValueError, match="sal"):
            sal_entries(bad, [20, 30.5])


# ------------------------------------------------------------------------------------------------ block_parts
T, THR, POOLS, FSS, FRAME, L = 3, [20, 30.5], ((4, 4), (16, 8)), (1, 5), (16, 32), 7
HW, AREA = FRAME[0] * FRAME[1], (FRAME[0] - 10) * (FRAME[1] - 10)
ALL = dict(pools=POOLS, persistence=True, fss=FSS, advection=True, spectrum=FRAME, joint=L, objects=2)


def _options(pools, persistence, fss, advection, spectrum, joint, objects):
    return dict(pools=POOLS if pools else (), persistence=persistence, fss=FSS if fss else (), advection=advection,
                spectrum=FRAME if spectrum else None, joint=L if joint else None, objects=2 if objects else None)


@pytest.mark.parametrize("combo", list(itertools.product((False, True), repeat=7)), ids=lambda c: "".join("01"[v] for v in c))
def test_the_new_part_is_last_and_moves_no_other(combo):
    from adnm_hip.validate import block_parts, sal_doubles
    kw, n = _options(*combo), len(THR)
    off, off_n = block_parts(T, n, **kw)
    for none in (None, False):
        assert block_parts(T, n, sal=ops.sal_spec(none), **kw) == (off, off_n), "the same parts as without the keyword"
    on, on_n = block_parts(T, n, sal=ops.sal_spec(True), **kw)
    assert on[:-1] == off and on_n == off_n + T * n * 12
    assert tuple(on[-1]) == ("sal", "sal", "pred", (), (T, n, 12), off_n) and on[-1].size == T * n * 12, "last, and contiguous behind the others"
    assert block_parts(T, n, sal=ops.sal_spec(dict(min_area=9, intensity=[1] * 91)), **kw) == (on, on_n), "the options do not change the table"
    assert sal_doubles(T, n) == sal_doubles(T, n, None) == sal_doubles(T, n, False) == 0 and sal_doubles(T, n, True) == sal_doubles(T, n, 5) == T * n * 12


def test_the_signatures_default_to_off():
    from adnm_hip.validate import Validator, aggregate, block_parts, sal_doubles
    for fn in (block_parts, aggregate, Validator.__init__, sal_doubles):
        assert inspect.signature(fn).parameters["sal"].default is None, fn
    assert sal_doubles(20, 4, True) == 20 * 4 * 12
    with pytest.raises(ValueError, match="sal"):
        sal_doubles(T, 2, 0)


# ------------------------------------------------------------------------------------------------ aggregate
def _fill_sal(tab, rng):
    """a consistent SAL table in place: counts with S <= L1 <= A frames, sums of plausible size"""
    n_a = rng.integers(6, 12, tab.shape[:-1])
    n_l1 = n_a - rng.integers(0, 3, n_a.shape)
    n_s = n_l1 - rng.integers(0, 3, n_a.shape)
    tab[..., 0], tab[..., 3], tab[..., 5] = n_a, n_l1, n_s
    tab[..., 10], tab[..., 11] = rng.integers(0, 3, n_a.shape), rng.integers(0, 3, n_a.shape)
    for c in (1, 2, 4, 6, 7, 8, 9):
        tab[..., c] = rng.standard_normal(n_a.shape)


@pytest.fixture(scope="module")
def full():
    """the block with every option on, integers in the former tables, a consistent SAL table, and what aggregate makes of it"""
    from adnm_hip.validate import HEADER, aggregate, block_parts
    parts, total = block_parts(T, len(THR), sal=(3, None), **ALL)
    rng = np.random.default_rng(29)
    blk = rng.integers(1, 1000, total).astype(np.float64)
    blk[:HEADER] = (12.5, 6, 12, 1)
    me = parts[-1]
    _fill_sal(blk[me.offset:].reshape(me.shape), rng)
    blk.setflags(write=False)
    return blk, {p.name: p for p in parts}, aggregate(blk, THR, T, HW, AREA, per_lead=True, sal=3, **ALL)


def test_aggregate_reads_the_sal_table_at_its_own_offset(full):
    from adnm_hip.validate import aggregate, block_parts, sal_entries
    blk, whole, res = full
    me = whole["sal"]
    assert me.offset + me.size == blk.size, "the last part of the one allocation"
    tab = blk[me.offset:].reshape(T, len(THR), 12)
    assert _same_tree(res["sal"], sal_entries(tab.sum(axis=0), THR, (3, None))) and res["sal"]["min_area"] == 3 and res["sal"]["intensity"] is None
    assert _same_tree(res["per_lead"]["sal"], sal_entries(tab, THR, (3, None)))
    assert res["sal"][20]["frames_A"] == int(tab[:, 0, 0].sum()) and res["sal"][30.5]["S"] == tab[:, 1, 6].sum() / tab[:, 1, 5].sum()
    assert (res["per_lead"]["sal"][20]["L1"] == tab[:, 0, 4] / tab[:, 0, 3]).all()
    # cut down to main plus the SAL table: the same entries, so nothing of them is read from another table
    parts, total = block_parts(T, len(THR), sal=(3, None))
    cut = np.zeros(total)
    for p in parts:
        cut[p.offset:p.offset + p.size] = blk[whole[p.name].offset:whole[p.name].offset + p.size]
    alone = aggregate(cut, THR, T, HW, AREA, per_lead=True, sal=3)
    assert _same_tree(alone["sal"], res["sal"]) and _same_tree(alone["per_lead"]["sal"], res["per_lead"]["sal"])
    # and every former entry is what it is without the SAL table
    former = aggregate(blk[:me.offset], THR, T, HW, AREA, per_lead=True, **ALL)
    assert list(res) == list(former)[:-1] + ["sal", "per_lead"] and list(res["per_lead"]) == list(former["per_lead"]) + ["sal"]
    assert list(res)[-4:] == ["joint", "objects", "sal", "per_lead"]
    assert _same_tree({k: res[k] for k in former if k != "per_lead"}, {k: former[k] for k in former if k != "per_lead"})
    assert _same_tree({k: res["per_lead"][k] for k in former["per_lead"]}, former["per_lead"])
    short = aggregate(blk, THR, T, HW, AREA, sal=3, **ALL)
    assert "per_lead" not in short and _same_tree(short["sal"], res["sal"])
    table = aggregate(blk, THR, T, HW, AREA, sal=dict(min_area=3, intensity=range(91)), **ALL)["sal"]
    assert table["intensity"] == tuple(range(91)) and _same_tree({k: v for k, v in table.items() if k != "intensity"}, {k: v for k, v in res["sal"].items() if k != "intensity"})


def test_aggregate_refuses_a_block_of_another_length(full):
    from adnm_hip.validate import aggregate
    blk = full[0]
    with pytest.raises(ValueError, match="sal"):
        aggregate(blk[:-1], THR, T, HW, AREA, sal=3, **ALL)
    with pytest.raises(ValueError):
        aggregate(blk, THR, T, HW, AREA, **ALL)            # the block has a SAL table, the options do not
    with pytest.raises(ValueError, match="sal"):
        aggregate(blk, THR, T, HW, AREA, sal=0.5, **ALL)


def test_validator_arguments():
    import torch
    from adnm_hip.validate import Validator
    from models.loss import enRainfallLoss
    model, crit = torch.nn.Identity(), enRainfallLoss()
    plain = Validator(model, crit, 20, 90.0)
    assert plain.sal is None and plain._weights is None and [p.name for p in plain._parts] == ["main"]
    assert Validator(model, crit, 20, 90.0, sal=False).sal is None
    val = Validator(model, crit, 20, 90.0, sal=True)
    assert val.sal == (1, None) and val.objects is None and [p.name for p in val._parts] == ["main", "sal"] and val._parts[-1].shape == (20, 4, 12)
    both = Validator(model, crit, 20, 90.0, objects=2, sal=dict(min_area=4, intensity=list(range(91))))
    assert both.sal == (4, tuple(range(91))) and both.objects == 2 and [p.name for p in both._parts] == ["main", "objects", "sal"]
    assert list(both._weights) == list(range(91))
    for bad in (0, -3, 1.5, "yes", dict(min_area=0)):
        with pytest.raises(ValueError, match="sal"):
            Validator(model, crit, 20, 90.0, sal=bad)
    with pytest.raises(ValueError, match="intensity"):
        Validator(model, crit, 20, 90.0, sal=dict(intensity=[1, 2, 3]))          # 3 entries for 91 levels
    with pytest.raises(ValueError, match="intensity"):
        Validator(model, crit, 20, 90.0, sal=dict(intensity=[65536] * 91))
    for scale in (0.5, 256.5):
        with pytest.raises(ValueError, match="value_scale"):
            Validator(model, crit, 20, scale, sal=True)
        assert Validator(model, crit, 20, scale).sal is None          # without sal= the scale is no concern of it


def test_the_one_shot_wrappers_refuse_what_is_not_a_gpu_tensor():
    import torch
    a = torch.zeros(2, 8, 8)
    with pytest.raises(RuntimeError):
        ops.sal_table(a, a, (20,), 90.0)
    with pytest.raises(RuntimeError):
        ops.object_moments(a, 20, 90.0)
    with pytest.raises(RuntimeError):
        ops.object_moments(a.numpy(), 20, 90.0)


# ------------------------------------------------------------------------------------------------ the C boundary
def test_new_prototypes_are_declared_and_exported_and_the_abi_version_stays():
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/adnm_hip.h"
        assert hasattr(so, name), f"{name} declared but not exported"
    assert protos["adnm_valid_sal_block_bytes"] == ("int64_t", ["int64_t", "int64_t"])
    assert protos["adnm_valid_sal_accum_ws_bytes"] == ("int64_t", ["int64_t"] * 5)
    assert protos["adnm_object_moments_ws_bytes"] == ("int64_t", ["int64_t"] * 4)
    assert protos["adnm_valid_sal_accum"] == ("int", ["const float*", "int64_t", "int64_t", "const float*", "void*", "const float*", "int64_t", "float", "int64_t",
                                                      "const uint16_t*", "void*", "int64_t", "int64_t", "int64_t", "int64_t", "int64_t", "adnm_stream_t"])
    assert protos["adnm_object_moments"] == ("int", ["const float*", "int64_t", "int64_t", "void*", "float", "float", "int64_t", "const uint16_t*", "void*",
                                                     "int64_t", "int64_t", "int64_t", "int64_t", "int64_t", "adnm_stream_t"])
    assert lib.load().adnm_abi_version() == 11


def test_the_queries_are_pure_host_functions_with_the_limits():
    """no GPU here: they answer all the same.  A frame of 65 536 pixels is inside, one of 65 537 outside."""
    q = lib.query
    blk, ws, mws = "adnm_valid_sal_block_bytes", "adnm_valid_sal_accum_ws_bytes", "adnm_object_moments_ws_bytes"
    assert q(blk, 20, 4) == 8 * 20 * 4 * 12 and q(blk, 1, 1) == 96 and q(blk, 3, 8) == 8 * 3 * 8 * 12
    assert [q(blk, *bad) for bad in ((0, 4), (-1, 4), (20, 0), (20, 9), (65536, 1))] == [-1] * 5
    for H, W in ((1, 1), (1, 7), (5, 3), (16, 16), (33, 65), (64, 64), (114, 116)):
        assert q(ws, 80, 20, H, W, 4) == 8 * 80 * 4 * 12 and q(mws, 80, 20, H, W) == 0, "records and words of such a frame live in LDS: the item rows alone"
    for H, W in ((115, 115), (128, 128), (130, 129), (161, 161)):
        cells = ((H + 1) // 2) * ((W + 1) // 2)
        assert q(mws, 2, 1, H, W) == 2 * 24 * cells and q(ws, 2, 1, H, W, 4) == 8 * 8 * 12 + 8 * 24 * cells, "the records live in the workspace"
    for H, W in ((162, 162), (200, 200), (256, 256), (1, 65536), (65536, 1), (1, 65535)):
        cells, words = ((H + 1) // 2) * ((W + 1) // 2), (4 * H * W + 7) // 8 * 8
        assert q(mws, 2, 1, H, W) == 2 * (24 * cells + words) and q(ws, 2, 1, H, W, 4) == 8 * 8 * 12 + 8 * (24 * cells + words), "records and words do"
        assert 24 * cells + words <= 16 * H * W + 16, "at most 16 bytes per pixel per workgroup"
    assert q(ws, 80, 20, 256, 256, 4) == 8 * 320 * 12 + 256 * 10 * 65536 and q(ws, 80, 20, 256, 256, 8) == 8 * 640 * 12 + 256 * 10 * 65536, "at most 256 slices"
    for H, W in ((65537, 1), (1, 65537), (257, 256), (256, 257), (0, 8), (8, 0), (-1, -1), (1 << 40, 1 << 40)):
        assert q(ws, 1, 1, H, W, 4) == -1 and q(mws, 1, 1, H, W) == -1, (H, W)
    for bad in ((0, 1), (3, 2), (65536, 1), (4, 0), (4, -2)):          # frames, T
        assert q(ws, *bad, 16, 16, 4) == -1 and q(mws, *bad, 16, 16) == -1, bad
    assert q(ws, 65535, 1, 16, 16, 8) == 8 * 65535 * 8 * 12 and q(ws, 4, 2, 16, 16, 0) == -1 and q(ws, 4, 2, 16, 16, 9) == -1


def test_bad_arguments_are_refused_before_any_launch():
    """every check comes before the first launch, so the refusals can be seen without a GPU (the pointers are never followed)"""
    so = lib.load()
    thr = (ctypes.c_float * 2)(20.0, 30.0)
    tab = (ctypes.c_uint16 * 91)(*range(91))
    rows = 8 * 2 * 2 * 12
    ok = dict(pred=64, ss=256, fs=256, tgt=128, table=192, thr=thr, nthr=2, scale=90.0, min_area=1, tab=tab, ws=512, ws_bytes=rows, frames=2, T=2, H=16, W=16)
    big = 8 * 2 * 2 * 12 + 4 * 10 * 65536          # two frames of 256 x 256 at two thresholds

    def accum(**kw):
        a = dict(ok, **kw)
        return so.adnm_valid_sal_accum(a["pred"], a["ss"], a["fs"], a["tgt"], a["table"], a["thr"], a["nthr"], a["scale"], a["min_area"], a["tab"], a["ws"],
                                       a["ws_bytes"], a["frames"], a["T"], a["H"], a["W"], None)
    for kw in (dict(pred=None), dict(tgt=None), dict(table=None), dict(thr=None), dict(ws=None), dict(pred=66), dict(tgt=130), dict(table=196), dict(ws=516),
               dict(ws_bytes=rows - 1), dict(ws_bytes=0), dict(nthr=0), dict(nthr=9), dict(min_area=0), dict(min_area=-5), dict(scale=0.5), dict(scale=256.5),
               dict(scale=0.0), dict(scale=float("nan")), dict(scale=float("inf")), dict(frames=3), dict(T=0), dict(frames=65536, T=1), dict(H=0), dict(W=0),
               dict(H=257, W=256), dict(H=1, W=65537), dict(fs=255), dict(fs=-256), dict(ss=-1), dict(H=256, W=256, fs=65536, ss=131072),
               dict(H=256, W=256, fs=65536, ss=131072, ws_bytes=big - 1), dict(H=256, W=256, fs=65535, ss=131072, ws_bytes=big)):
        assert accum(**kw) != 0, kw
        assert "valid_sal_accum" in lib.last_error(), kw

    def moments(**kw):
        a = dict(ok, ws=None, ws_bytes=0)
        a.update(kw)
        return so.adnm_object_moments(a["pred"], a["ss"], a["fs"], a["table"], 20.0, a["scale"], a["min_area"], a["tab"], a["ws"], a["ws_bytes"], a["frames"],
                                      a["T"], a["H"], a["W"], None)
    for kw in (dict(pred=None), dict(table=None), dict(pred=66), dict(table=196), dict(ws=4), dict(min_area=0), dict(scale=0.5), dict(scale=256.5),
               dict(scale=float("nan")), dict(frames=3), dict(T=0), dict(frames=65536, T=1), dict(H=0), dict(H=257, W=256), dict(fs=255), dict(ss=-1),
               dict(H=256, W=256, fs=65536, ss=131072), dict(H=256, W=256, fs=65536, ss=131072, ws=512, ws_bytes=2 * 10 * 65536 - 1),
               dict(H=128, W=128, fs=16384, ss=32768), dict(H=128, W=128, fs=16384, ss=32768, ws=512, ws_bytes=2 * 24 * 4096 - 1)):
        assert moments(**kw) != 0, kw
        assert "object_moments" in lib.last_error(), kw


def test_the_scored_pair_contract_of_the_new_entry_point():
    """pair_check's own cases (tests/test_scored_pair_host.py states them for the five former entry points), in its order: null pointers, the
    alignment of the fields, of the table, of the workspace, the shape, the frame stride, the sample stride, the workspace's size"""
    so = lib.load()
    thr = (ctypes.c_float * 1)(20.0)
    need = lib.query("adnm_valid_sal_accum_ws_bytes", 4, 2, 8, 8, 1)
    assert need == 8 * 4 * 12

    def call(pred=64, ss=128, fs=64, tgt=1024, table=4096, thr=thr, ws=8192, ws_bytes=need, frames=4, T=2, H=8, W=8):
        rc = so.adnm_valid_sal_accum(pred, ss, fs, tgt, table, thr, 1, 90.0, 1, None, ws, ws_bytes, frames, T, H, W, None)
        return rc, lib.last_error()
    for kw, text in ((dict(pred=None), "null pointer"), (dict(tgt=None), "null pointer"), (dict(table=None), "null pointer"), (dict(thr=None), "null pointer"),
                     (dict(pred=66), "pred and target must be 4-byte aligned"), (dict(tgt=1026), "pred and target must be 4-byte aligned"),
                     (dict(table=4100), "the table must be 8-byte aligned"), (dict(ws=8196), "the workspace must be 8-byte aligned"),
                     (dict(frames=5), "T >= 1 must divide frames"), (dict(frames=65536, T=1), "frames <= 65535"), (dict(H=257, W=256), "1 <= H * W <= 65536"),
                     (dict(fs=63), "pred_frame_stride must be 0 or >= H*W, got 63"), (dict(ss=-1), "pred_sample_stride must be >= 0, got -1"),
                     (dict(ws_bytes=need - 1), f"workspace {need - 1} < {need} bytes"), (dict(ws=None), "workspace")):
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("valid_sal_accum: ") and text in msg, (kw, msg)
    # the order: a null pointer is named before a misaligned one, the alignment before the shape, the shape before the strides, those before the workspace
    assert "null pointer" in call(pred=None, tgt=1026, H=0)[1] and "aligned" in call(tgt=1026, H=0, fs=1)[1]
    assert "1 <= H * W" in call(H=0, fs=-5, ws_bytes=0)[1] and "pred_frame_stride" in call(fs=63, ss=-1, ws_bytes=0)[1] and "pred_sample_stride" in call(ss=-1, ws_bytes=0)[1]
    # a held source (frame stride 0) and a strided one pass the check as far as the workspace
    assert "workspace" in call(fs=0, ws_bytes=0)[1] and "workspace" in call(fs=100, ss=1000, ws_bytes=0)[1]
