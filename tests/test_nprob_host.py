"""The neighbourhood exceedance probability without a GPU: the table's layout and its place in the Validator's block, the entry points at
the C boundary (declared, exported, refusing every limit before any launch), validate.nprob_entries against the yardstick's pixel-wise
scores (nprob_ref) on the yardstick's own tables, the decomposition identity, the degenerate forecasts, and the arguments."""
import ctypes
import inspect

import numpy as np
import pytest

import nprob_ref as N
from adnm_hip import lib, ops
from adnm_hip import validate as V

NEW = ("adnm_valid_nprob_block_bytes", "adnm_valid_nprob_accum_ws_bytes", "adnm_valid_nprob_accum", "adnm_neighbour_prob")
THR, SCALE = [20.0, 30.0, 35.0, 40.0], 90.0


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= tol)).all())


# ------------------------------------------------------------------------------------------------ layout and parts
def test_layout_offsets_and_size():
    assert ops.nprob_layout((1,)) == (((0, 2),), 4)
    assert ops.nprob_layout((1, 5, 17, 33)) == (((0, 2), (4, 30), (56, 346), (636, 1726)), 2816)
    assert ops.nprob_layout((33, 3)) == (((0, 1090), (2180, 2190)), 2200)
    for scales in ((1,), (3, 1), (1, 5, 17, 33)):
        offs, S = ops.nprob_layout(scales)
        assert (list(offs), S) == N.layout(scales) and S == sum(2 * (n * n + 1) for n in scales)
    assert ops.nprob_layout(()) == ((), 0) and ops.nprob_layout(None) == ((), 0)
    assert 20 * 4 * ops.nprob_layout((1, 5, 17, 33))[1] == 225280
    for bad in ((2,), (35,), (5, 5), (1, 3, 5, 7, 9)):
        with pytest.raises(ValueError):
            ops.nprob_layout(bad)


def test_block_parts_gains_one_last_row_and_nothing_else_moves():
    T, n = 5, 4
    sal = ops.sal_spec(True)
    configs = [dict(), dict(pools=((4, 4),), persistence=True), dict(fss=(1, 5), advection=True, pools=((2, 2),)), dict(spectrum=(48, 64), joint=91),
               dict(objects=2, sal=sal), dict(pools=((4, 4), (16, 8)), persistence=True, fss=(1, 33), advection=True, spectrum=(32, 32), joint=91, sal=sal, objects=1)]
    for kw in configs:
        base = V.block_parts(T, n, **kw)
        assert V.block_parts(T, n, nprob=None, **kw) == base and V.block_parts(T, n, nprob=(), **kw) == base, "the default changed a configuration"
        parts, total = V.block_parts(T, n, nprob=(3, 1), **kw)
        assert parts[:-1] == base[0], "a part moved"
        assert parts[-1] == V.Part("nprob", "nprob", "pred", (), (T, n, 24), base[1]) and total == base[1] + T * n * 24
    params = list(inspect.signature(V.block_parts).parameters)
    assert params[:8] == ["T", "nthr", "pools", "persistence", "fss", "advection", "spectrum", "joint"] and params[-1] == "objects", "the positional parameters stay"
    assert set(params[8:]) == {"sal", "nprob", "objects"}, "the tables that are passed by name"
    assert inspect.signature(V.block_parts).parameters["nprob"].default is None
    assert V.nprob_doubles(20, 4) == 0 and V.nprob_doubles(20, 4, ()) == 0 and V.nprob_doubles(20, 4, (1, 5, 17, 33)) == 225280
    assert V.nprob_doubles(3, 8, 33) == 3 * 8 * 2180


# ------------------------------------------------------------------------------------------------ the C boundary
def _scales(*ns):
    return lib.i64_table(list(ns))


def test_new_prototypes_are_declared_and_exported_and_the_abi_version_stays():
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/adnm_hip.h"
        assert hasattr(so, name), f"{name} declared but not exported"
    assert protos["adnm_valid_nprob_accum"] == protos["adnm_valid_fss_accum"], "the argument list is adnm_valid_fss_accum's"
    assert protos["adnm_valid_nprob_accum_ws_bytes"] == protos["adnm_valid_fss_accum_ws_bytes"]
    assert protos["adnm_neighbour_prob"] == ("int", ["const float*", "float*", "const float*", "int64_t", "float", "int64_t", "int64_t", "int64_t", "int64_t",
                                                     "adnm_stream_t"])
    assert lib.load().adnm_abi_version() == 11


def test_byte_queries():
    q = lib.query
    assert q("adnm_valid_nprob_block_bytes", 20, 4, _scales(1, 5, 17, 33), 4) == 8 * 225280
    assert q("adnm_valid_nprob_block_bytes", 1, 8, _scales(33), 1) == 8 * 8 * 2180
    for bad in ((0, 4, _scales(1), 1), (65536, 4, _scales(1), 1), (20, 0, _scales(1), 1), (20, 9, _scales(1), 1), (20, 4, _scales(1), 0), (20, 4, None, 1),
                (20, 4, _scales(2), 1), (20, 4, _scales(35), 1), (20, 4, _scales(3, 3), 2), (20, 4, _scales(1, 3, 5, 7, 9), 5)):
        assert q("adnm_valid_nprob_block_bytes", *bad) == -1, bad
    ok, ws = _scales(1, 33), "adnm_valid_nprob_accum_ws_bytes"
    assert q(ws, 80, 20, 128, 128, 4, ok, 2) == 0 and q(ws, 2, 1, 5, 40, 8, ok, 2) == 0 and q(ws, 1, 1, 1, 1, 1, _scales(33), 1) == 0, "no workspace"
    for bad in ((80, 7, 128, 128, 4, ok, 2), (80, 0, 128, 128, 4, ok, 2), (65540, 20, 128, 128, 4, ok, 2), (80, 20, 128, 128, 0, ok, 2),
                (80, 20, 128, 128, 9, ok, 2), (80, 20, 128, 128, 4, ok, 0), (80, 20, 128, 128, 4, None, 2), (80, 20, 4096, 4096, 4, ok, 2),
                (80, 20, 4, 40000, 4, ok, 1), (80, 20, 0, 16, 4, ok, 1), (80, 20, 128, 128, 4, _scales(5, 9, 5), 3)):
        assert q(ws, *bad) == -1, bad
    for bad in (0, 2, 32, 34, 35, -1):
        assert q(ws, 80, 20, 128, 128, 4, _scales(bad), 1) == -1, bad


def test_every_limit_is_refused_on_the_host_with_its_own_message():
    """fake addresses: anything that reached a launch would fault, and the stream is never touched"""
    so = lib.load()
    thr, ok = (ctypes.c_float * 4)(20, 30, 35, 40), _scales(1, 33)

    def call(pred=16, ss=20 * 64 * 64, fs=64 * 64, tgt=32, table=64, thr_=thr, nthr=4, scales=ok, nscale=2, ws=None, ws_bytes=0, frames=40, T=20, H=64, W=64):
        rc = so.adnm_valid_nprob_accum(pred, ss, fs, tgt, table, thr_, nthr, 90.0, scales, nscale, ws, ws_bytes, frames, T, H, W, None)
        return rc, lib.last_error()

    cases = [(dict(pred=None), "null pointer"), (dict(tgt=None), "null pointer"), (dict(table=None), "null pointer"), (dict(thr_=None), "null pointer"),
             (dict(scales=None), "null pointer"),
             (dict(pred=18), "4-byte aligned"), (dict(tgt=34), "4-byte aligned"), (dict(table=68), "8-byte aligned"),
             (dict(nscale=0), "1..4 scales"), (dict(scales=_scales(1, 3, 5, 7, 9), nscale=5), "1..4 scales"),
             (dict(scales=_scales(4), nscale=1), "odd and in 1..33"), (dict(scales=_scales(35), nscale=1), "odd and in 1..33"),
             (dict(scales=_scales(0), nscale=1), "odd and in 1..33"), (dict(scales=_scales(3, -1), nscale=2), "odd and in 1..33"),
             (dict(scales=_scales(5, 9, 5), nscale=3), "given twice"),
             (dict(nthr=0), "1..8 thresholds"), (dict(nthr=9), "1..8 thresholds"),
             (dict(T=0), "must divide frames"), (dict(T=7), "must divide frames"),
             (dict(frames=65540, T=20), "frames <= 65535"),
             (dict(W=32768, H=16), "[1, 32768)"), (dict(H=32768, W=16), "[1, 32768)"), (dict(H=0), "[1, 32768)"),
             (dict(H=4096, W=4096), "2^24"),
             (dict(fs=64 * 64 - 1), "pred_frame_stride"), (dict(fs=-4096), "pred_frame_stride"),
             (dict(ss=-1), "pred_sample_stride")]
    for kw, text in cases:
        rc, err = call(**kw)
        assert rc == -1 and text in err and "valid_nprob_accum" in err, (kw, rc, err)
    assert len({text for _, text in cases}) == 13, "one message per limit"

    def prob(field=16, out=32, thr_=thr, nthr=4, scale=9, frames=4, H=64, W=64):
        rc = so.adnm_neighbour_prob(field, out, thr_, nthr, 90.0, scale, frames, H, W, None)
        return rc, lib.last_error()
    for kw, text in [(dict(field=None), "null pointer"), (dict(out=None), "null pointer"), (dict(thr_=None), "null pointer"), (dict(field=18), "4-byte aligned"),
                     (dict(out=34), "4-byte aligned"), (dict(nthr=0), "1..8 thresholds"), (dict(nthr=9), "1..8 thresholds"), (dict(scale=4), "odd and in 1..33"),
                     (dict(scale=35), "odd and in 1..33"), (dict(scale=-1), "odd and in 1..33"), (dict(frames=0), "frames <= 65535"),
                     (dict(frames=65536), "frames <= 65535"), (dict(H=0), "[1, 32768)"), (dict(W=32768, H=4), "[1, 32768)"), (dict(H=4096, W=4096), "2^24")]:
        rc, err = prob(**kw)
        assert rc == -1 and text in err and "neighbour_prob" in err, (kw, rc, err)


# ------------------------------------------------------------------------------------------------ the host function
CASES = [("sparse", lambda: N.sparse_fields(3, 37, 45, 2)), ("noise", lambda: N.noise_fields(2, 37, 45, 4, 0.41)), ("thin", lambda: N.noise_fields(2, 37, 45, 5, 0.1))]
SCALES = (1, 3, 9)


@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_entries_equal_the_pixel_wise_scores(name, make):
    t, p = make()
    rows = N.frame_hist(t, p, THR, SCALE, SCALES).sum(axis=0)
    res = V.nprob_entries(rows, SCALES, THR)
    assert list(res) == list(SCALES)
    seen = 0
    for i, n in enumerate(SCALES):
        assert list(res[n]) == [20, 30, 35, 40]
        (a0, a1), per = N.layout(SCALES)[0][i], n * n + 1
        for k, thr in enumerate(THR):
            e, want = res[n][int(thr)], N.pixel_scores(t, p, thr, SCALE, n)
            assert e["histogram"].dtype == np.int64 and e["histogram"].shape == (2, per)
            assert (e["histogram"][0] == rows[k, a0:a0 + per]).all() and (e["histogram"][1] == rows[k, a1:a1 + per]).all()
            assert e["histogram"].sum() == t.size
            for key in ("base_rate", "brier", "reliability", "resolution", "uncertainty", "brier_skill", "roc_area"):
                assert _close(e[key], want[key]), (name, n, thr, key, e[key], want[key])
            assert e["roc"]["pod"].shape == (per + 1,) and _close(e["roc"]["pod"], want["pod"]) and _close(e["roc"]["pofd"], want["pofd"])
            d = e["reliability_diagram"]
            assert _close(d["edges"], np.linspace(0, 1, 11)) and (d["count"] == want["count"]).all() and d["count"].sum() == t.size
            assert _close(d["forecast_mean"], want["forecast_mean"]) and _close(d["observed_frequency"], want["observed_frequency"])
            # the decomposition is exact for this discrete forecast
            assert abs(e["brier"] - (e["reliability"] - e["resolution"] + e["uncertainty"])) <= 1e-12, (name, n, thr)
            if 0.0 < want["base_rate"] < 1.0:
                seen += 1
                assert e["roc"]["pod"][0] == 1.0 and e["roc"]["pofd"][0] == 1.0 and e["roc"]["pod"][-1] == 0.0 and e["roc"]["pofd"][-1] == 0.0
                assert (np.diff(e["roc"]["pod"]) <= 0).all() and (np.diff(e["roc"]["pofd"]) <= 0).all() and 0.0 <= e["roc_area"] <= 1.0
    assert seen >= 6, "hardly a cell has both events and non-events: nothing is compared"


def test_other_bin_counts_and_the_leading_axis():
    t, p = N.sparse_fields(4, 20, 24, 7)
    rows = N.table(t, p, THR[:2], SCALE, (5,), 2)
    lead = V.nprob_entries(rows, (5,), THR[:2], bins=4)
    for tt in range(2):
        one = V.nprob_entries(rows[tt], (5,), THR[:2], bins=4)
        want = N.pixel_scores(t[tt::2], p[tt::2], 20.0, SCALE, 5, bins=4)
        assert (one[5][20]["reliability_diagram"]["count"] == want["count"]).all() and _close(one[5][20]["reliability_diagram"]["forecast_mean"], want["forecast_mean"])
        for key in ("base_rate", "brier", "reliability", "resolution", "uncertainty", "brier_skill", "roc_area"):
            assert lead[5][20][key].shape == (2,) and _close(lead[5][20][key][tt], one[5][20][key]), key
        assert (lead[5][20]["histogram"][tt] == one[5][20]["histogram"]).all() and lead[5][20]["histogram"].shape == (2, 2, 26)
        assert _close(lead[5][20]["roc"]["pod"][tt], one[5][20]["roc"]["pod"]) and lead[5][20]["roc"]["pofd"].shape == (2, 27)
        assert _close(lead[5][20]["reliability_diagram"]["observed_frequency"][tt], one[5][20]["reliability_diagram"]["observed_frequency"])
    # p = 15 / 25 = 0.6 belongs to the bin that starts at 0.6, whatever 6 * 0.1 is in binary
    rows = np.zeros((1, 52), dtype=np.int64)
    rows[0, 15] = 7
    d = V.nprob_entries(rows, (5,), [20.0])[5][20]["reliability_diagram"]
    assert d["count"][6] == 7 and d["count"].sum() == 7
    rows[0, 15], rows[0, 25] = 0, 3        # p = 1: the last bin is closed on the right
    assert V.nprob_entries(rows, (5,), [20.0])[5][20]["reliability_diagram"]["count"][9] == 3


def test_a_perfect_forecast_at_scale_one():
    t, _ = N.sparse_fields(2, 37, 45, 3)
    rows = N.frame_hist(t, t, THR, SCALE, (1,)).sum(axis=0)
    res = V.nprob_entries(rows, (1,), THR)
    for thr in (20, 30, 35, 40):
        e = res[1][thr]
        assert e["histogram"][0, 1] == 0 and e["histogram"][1, 0] == 0 and e["histogram"][1, 1] > 0
        assert e["brier"] == 0.0 and e["roc_area"] == 1.0 and e["reliability"] == 0.0 and e["brier_skill"] == 1.0
        assert e["resolution"] == e["uncertainty"] > 0.0


def test_no_events_gives_the_nans():
    z = np.zeros((2, 16, 16), dtype=np.float32)
    rows = N.frame_hist(z, z, THR[:1], SCALE, (3,)).sum(axis=0)
    assert rows[0, 0] == 512 and rows.sum() == 512
    e = V.nprob_entries(rows, (3,), THR[:1])[3][20]
    assert e["base_rate"] == 0.0 and e["brier"] == 0.0 and e["uncertainty"] == 0.0 and e["reliability"] == 0.0 and e["resolution"] == 0.0
    assert np.isnan(e["brier_skill"]) and np.isnan(e["roc"]["pod"][:-1]).all() and np.isnan(e["roc_area"])
    assert (e["roc"]["pofd"][:2] == [1.0, 0.0]).all() and e["roc"]["pod"][-1] == 0.0
    d = e["reliability_diagram"]
    assert d["count"][0] == 512 and np.isnan(d["forecast_mean"][1:]).all() and np.isnan(d["observed_frequency"][1:]).all() and d["observed_frequency"][0] == 0.0
    empty = V.nprob_entries(np.zeros((1, 20)), (3,), THR[:1])[3][20]     # no pixel at all
    assert np.isnan(empty["base_rate"]) and np.isnan(empty["brier"]) and np.isnan(empty["roc_area"])


def test_entries_refuse_what_is_not_a_table():
    with pytest.raises(ValueError, match="rows are"):
        V.nprob_entries(np.zeros((4, 19)), (3,), THR)
    with pytest.raises(ValueError, match="rows are"):
        V.nprob_entries(np.zeros((4, 20)), (), THR)
    with pytest.raises(ValueError, match="integer"):
        V.nprob_entries(np.full((4, 20), 0.5), (3,), THR)
    with pytest.raises(ValueError, match="bins"):
        V.nprob_entries(np.zeros((4, 20)), (3,), THR, bins=0)
    for bad in ((2,), (35,), (5, 5)):
        with pytest.raises(ValueError):
            V.nprob_entries(np.zeros((4, 20)), bad, THR)


# ------------------------------------------------------------------------------------------------ aggregate and the arguments
def test_aggregate_reads_the_last_table_and_the_former_result_stays():
    T, n, scales = 3, 2, (1, 3)
    t, p = N.sparse_fields(2 * T, 24, 24, 9)
    tab = N.table(t, p, THR[:n], SCALE, scales, T).astype(np.float64)
    rng = np.random.default_rng(1)
    main = rng.integers(1, 1 << 20, (T, 4 * n + 3)).astype(np.float64)
    head = np.concatenate([[1.25, 2, 2, 0], main.ravel()])
    plain = V.aggregate(head, THR[:n], T, 576, None, per_lead=True)
    res = V.aggregate(np.concatenate([head, tab.ravel()]), THR[:n], T, 576, None, per_lead=True, nprob=scales)
    assert list(res) == [k for k in plain if k != "per_lead"] + ["nprob", "per_lead"] and list(res["per_lead"]) == list(plain["per_lead"]) + ["nprob"]
    assert repr({k: res[k] for k in plain if k != "per_lead"}) == repr({k: plain[k] for k in plain if k != "per_lead"})
    assert repr({k: res["per_lead"][k] for k in plain["per_lead"]}) == repr(plain["per_lead"])
    assert repr(res["nprob"]) == repr(V.nprob_entries(tab.sum(axis=0), scales, THR[:n])) and repr(res["per_lead"]["nprob"]) == repr(V.nprob_entries(tab, scales, THR[:n]))
    assert res["nprob"][3][20]["histogram"].sum() == 2 * T * 576
    with pytest.raises(ValueError, match="doubles"):
        V.aggregate(np.concatenate([head, tab.ravel()]), THR[:n], T, 576, None)
    with pytest.raises(ValueError, match="nprob"):
        V.aggregate(np.concatenate([head, tab.ravel()]), THR[:n], T, 576, None, nprob=(1,))


def test_validator_and_forecaster_arguments():
    import torch
    from adnm_hip.forecast import Forecast, Forecaster, Palette
    from adnm_hip.validate import Validator
    from models.loss import enRainfallLoss
    assert inspect.signature(Validator.__init__).parameters["nprob"].default is None
    model, crit = torch.nn.Identity(), enRainfallLoss()
    kinds = lambda v: [p.kind for p in v._parts]
    val = Validator(model, crit, 20, 255.0)
    assert val.nprob == () and kinds(val) == ["main"]
    val = Validator(model, crit, 20, 255.0, nprob=(1, 5, 17, 33))
    assert val.nprob == (1, 5, 17, 33) and kinds(val) == ["main", "nprob"] and val._parts[-1].shape == (20, 4, 2816)
    val = Validator(model, crit, 20, 255.0, fss=(9, 3), nprob=True, sal=True)
    assert val.nprob == (9, 3) and kinds(val) == ["main", "fss", "sal", "nprob"], "behind the SAL pass"
    assert Validator(model, crit, 20, 255.0, fss=(9, 3), nprob=5).nprob == (5,) and Validator(model, crit, 20, 255.0, fss=(9,), nprob=False).nprob == ()
    with pytest.raises(ValueError, match="fss"):
        Validator(model, crit, 20, 255.0, nprob=True)
    for bad in ((2,), (35,), (5, 5), (1, 3, 5, 7, 9), (4.0,), "5"):
        with pytest.raises(ValueError):
            Validator(model, crit, 20, 255.0, nprob=bad)
    pal = Palette([0.0, 0.5, 1.0], np.array([[0, 0, 0, 255], [255, 0, 0, 255]], dtype=np.uint8))
    assert Forecaster(model, pal).probability is None and inspect.signature(Forecaster.__init__).parameters["probability"].default is None
    fc = Forecaster(model, pal, pixel_scale=90.0, probability=dict(thresholds=(35, 40), scale=9))
    assert list(fc.probability[0]) == [35.0, 40.0] and fc.probability[1:] == (2, 9)
    for scale in (None, 0):
        with pytest.raises(ValueError, match="pixel_scale"):
            Forecaster(model, pal, pixel_scale=scale, probability=dict(thresholds=(35,), scale=9))
    for bad in (dict(thresholds=(35,), scale=4), dict(thresholds=(35,), scale=(3, 5)), dict(thresholds=(), scale=3), dict(thresholds=range(9), scale=3),
                dict(thresholds=(35,)), (35, 9)):
        with pytest.raises(ValueError):
            Forecaster(model, pal, probability=bad)
    assert Forecast(1, 2, 3).prob is None and Forecast(1, 2, 3, 4).prob == 4
