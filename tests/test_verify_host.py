"""Pooled scores, per-lead-time scores and the persistence baseline without a GPU: the CPU yardstick checks itself, the three entry points
at the C boundary (declared, exported, additive, refusing every limit before any launch), validate.aggregate on a hand-made block,
and the Validator's new arguments."""
import ctypes

import numpy as np
import pytest

import verify_ref as R
from adnm_hip import lib
from adnm_hip.evaluator import contingency_metrics

NEW = ("adnm_valid_pool_block_bytes", "adnm_valid_pool_accum_ws_bytes", "adnm_valid_pool_accum")


# ------------------------------------------------------------------------------------------------ the helper
def test_max_pool_reference_equals_a_plain_window_loop():
    t, p = R.radar_fields(2, 9, 11, 0)
    t[0, 0, 0], p[0, 8, 10], p[1, 4, 4] = 1.5, 0.9, float("nan")
    pools = [(1, 1), (3, 2), (4, 4), (9, 1), (2, 1)]
    a, b = R.ref_counts(t, p, R.THR, R.SCALE, pools), R.loop_counts(t, p, R.THR, R.SCALE, pools)
    assert (a == b).all()
    for i, pool in enumerate(pools):
        assert (a[:, i].reshape(2, 4, 4).sum(-1) == R.windows(9, 11, pool)).all()
    assert a[:, :, 0].sum() > 0 and a[:, :, 2].sum() > 0, "no event at all: nothing is compared"


def test_quant_is_the_device_statement():
    v = np.array([-1.0, 0.0, 0.5, 1.0, 2.0, np.nan, np.inf, -np.inf, 0.2222222], dtype=np.float32)
    assert R.quant(v, 90.0).tolist() == [0, 0, 45, 90, 90, 0, 90, 0, float(np.floor(np.float32(0.2222222) * np.float32(90.0)))]
    assert R.quant(v, 90.0).dtype == np.float32


# ------------------------------------------------------------------------------------------------ the C boundary
def test_new_prototypes_are_declared_and_exported_and_the_abi_version_stays():
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/adnm_hip.h"
        assert hasattr(so, name), f"{name} declared but not exported"
    assert protos["adnm_valid_pool_accum"][0] == "int" and protos["adnm_valid_pool_accum"][1][-1] == "adnm_stream_t"
    assert protos["adnm_valid_pool_block_bytes"][0] == protos["adnm_valid_pool_accum_ws_bytes"][0] == "int64_t"
    assert lib.load().adnm_abi_version() == 11


def _pools(*pairs):
    return lib.i64_table([v for p in pairs for v in p])


def test_byte_queries():
    q = lib.query
    assert q("adnm_valid_pool_block_bytes", 20, 4, 3) == 8 * 20 * 3 * 16
    for bad in ((0, 4, 3), (20, 0, 3), (20, 9, 3), (20, 4, 0), (20, 4, 5)):
        assert q("adnm_valid_pool_block_bytes", *bad) == -1, bad
    ok = _pools((4, 4), (16, 8))
    # 16 tiles of 32 x 32 window origins per 128 x 128 frame, per pool and threshold three uint32 (target, forecast, both)
    assert q("adnm_valid_pool_accum_ws_bytes", 80, 20, 128, 128, 4, ok, 2) == 80 * 16 * 2 * 12 * 4
    assert q("adnm_valid_pool_accum_ws_bytes", 6, 6, 37, 53, 4, ok, 2) == 6 * 4 * 2 * 12 * 4
    assert q("adnm_valid_pool_accum_ws_bytes", 80, 7, 128, 128, 4, ok, 2) == -1, "T does not divide frames"
    assert q("adnm_valid_pool_accum_ws_bytes", 80, 0, 128, 128, 4, ok, 2) == -1, "T = 0"
    assert q("adnm_valid_pool_accum_ws_bytes", 65540, 20, 128, 128, 4, ok, 2) == -1, "frames > 65535"
    assert q("adnm_valid_pool_accum_ws_bytes", 80, 20, 128, 128, 0, ok, 2) == -1 and q("adnm_valid_pool_accum_ws_bytes", 80, 20, 128, 128, 9, ok, 2) == -1
    assert q("adnm_valid_pool_accum_ws_bytes", 80, 20, 128, 128, 4, ok, 0) == -1 and q("adnm_valid_pool_accum_ws_bytes", 80, 20, 128, 128, 4, ok, 5) == -1
    assert q("adnm_valid_pool_accum_ws_bytes", 80, 20, 128, 128, 4, None, 2) == -1, "no pools"
    assert q("adnm_valid_pool_accum_ws_bytes", 80, 20, 4096, 4096, 4, ok, 2) == -1, "H*W >= 2^24"
    assert q("adnm_valid_pool_accum_ws_bytes", 80, 20, 4, 40000, 4, ok, 1) == -1, "W >= 32768"
    assert q("adnm_valid_pool_accum_ws_bytes", 80, 20, 128, 15, 4, ok, 2) == -1, "a 16-pixel window on a 15-pixel frame"
    for bad in ((0, 0), (4, 5), (33, 1), (4, 0)):
        assert q("adnm_valid_pool_accum_ws_bytes", 80, 20, 128, 128, 4, _pools(bad), 1) == -1, bad


def test_every_limit_is_refused_on_the_host_with_its_own_message():
    """fake addresses: anything that reached a launch would fault, and the stream is never touched"""
    so = lib.load()
    thr, ok = (ctypes.c_float * 4)(20, 30, 35, 40), _pools((4, 4), (16, 8))

    def call(pred=16, ss=20 * 64 * 64, fs=64 * 64, tgt=32, table=64, thr_=thr, nthr=4, pools=ok, npool=2, ws=128, ws_bytes=1 << 30, frames=40, T=20, H=64, W=64):
        rc = so.adnm_valid_pool_accum(pred, ss, fs, tgt, table, thr_, nthr, 90.0, pools, npool, ws, ws_bytes, frames, T, H, W, None)
        return rc, lib.last_error()

    cases = [(dict(pred=None), "null pointer"), (dict(tgt=None), "null pointer"), (dict(table=None), "null pointer"), (dict(thr_=None), "null pointer"),
             (dict(pools=None), "null pointer"),
             (dict(pred=18), "4-byte aligned"), (dict(tgt=34), "4-byte aligned"), (dict(table=68), "8-byte aligned"),
             (dict(npool=0), "1..4 pools"), (dict(npool=5), "1..4 pools"),
             (dict(pools=_pools((4, 0)), npool=1), "1 <= stride <= size <= 32"), (dict(pools=_pools((4, 5)), npool=1), "1 <= stride <= size <= 32"),
             (dict(pools=_pools((33, 1)), npool=1), "1 <= stride <= size <= 32"), (dict(pools=_pools((0, 0)), npool=1), "1 <= stride <= size <= 32"),
             (dict(H=15), "larger than the frame"), (dict(W=15), "larger than the frame"),
             (dict(nthr=0), "1..8 thresholds"), (dict(nthr=9), "1..8 thresholds"),
             (dict(T=0), "must divide frames"), (dict(T=7), "must divide frames"),
             (dict(frames=65540, T=20), "frames <= 65535"),
             (dict(W=32768, H=16), "[1, 32768)"), (dict(H=32768, W=16), "[1, 32768)"),
             (dict(H=4096, W=4096), "2^24"),
             (dict(fs=64 * 64 - 1), "pred_frame_stride"), (dict(fs=-4096), "pred_frame_stride"),
             (dict(ss=-1), "pred_sample_stride")]
    for kw, text in cases:
        rc, err = call(**kw)
        assert rc == -1 and text in err, (kw, rc, err)
    assert len({text for _, text in cases}) == 13, "one message per limit"
    rc, err = call(ws_bytes=8)
    assert rc == -3 and "workspace" in err
    rc, err = call(ws=None)
    assert rc == -3 and "workspace" in err


# ------------------------------------------------------------------------------------------------ aggregate
T, THR, POOLS = 5, [20, 30, 35, 40], ((4, 4), (16, 8), (1, 1))


def _hand_block(seed, pools=POOLS, persistence=True):
    """an integer block: header, main table, forecast pooled table, baseline pooled table"""
    from adnm_hip.validate import baseline_pools, block_doubles
    rng = np.random.default_rng(seed)
    n = len(THR)
    n0, n1, n2 = block_doubles(T, n, pools, persistence)
    main = rng.integers(1, 1 << 20, (T, 4 * n + 3)).astype(np.float64)
    main[:, 4 * n:] += rng.random((T, 3))
    blk = np.concatenate([[1.25, 2, 6, 0], main.ravel(), rng.integers(0, 1 << 20, n1 + n2).astype(np.float64)])
    assert blk.shape == (n0 + n1 + n2,)
    ftab = blk[n0:n0 + n1].reshape(T, len(pools), 4 * n)
    btab = blk[n0 + n1:].reshape(T, len(baseline_pools(pools)) if persistence else 0, 4 * n)
    return blk, main, ftab, btab


def _same(a, b):
    return repr(a) == repr(b)


def _check_lead(lead, rows):
    """lead: {thr: {name: length-T array}} against contingency_metrics on each row"""
    for t in range(T):
        m, far = contingency_metrics(rows[t], THR)
        for k, thr in enumerate(THR):
            for name in ("TP", "FN", "FP", "TN", "CSI", "POD", "HSS"):
                assert _same(float(lead[thr][name][t]), float(m[thr][name])), (t, thr, name)
            assert _same(float(lead[thr]["FAR"][t]), float(far[k]))
    for thr in THR:
        assert set(lead[thr]) == {"TP", "FN", "FP", "TN", "CSI", "POD", "FAR", "HSS"} and all(v.shape == (T,) for v in lead[thr].values())


def test_aggregate_on_a_hand_made_block():
    from adnm_hip.validate import aggregate, baseline_pools
    hw, area, n = 48 * 48, 38 * 38, len(THR)
    blk, main, ftab, btab = _hand_block(3)
    base = baseline_pools(POOLS)
    assert base == ((1, 1), (4, 4), (16, 8))
    res = aggregate(blk, THR, T, hw, area, pools=POOLS, persistence=True, per_lead=True)
    plain = aggregate(blk[:4 + T * (4 * n + 3)], THR, T, hw, area)
    assert list(plain) == ["threshold_metrics", "FAR", "RMSE", "MAE", "MSE", "SSIM", "LPIPS", "loss_sum", "loss_mean", "batches", "samples", "nonfinite"]
    assert _same({k: res[k] for k in plain}, plain) and set(res) == set(plain) | {"pooled", "persistence", "per_lead"}
    # the default call is what the parent's aggregate returned: its statement, restated
    m, far = contingency_metrics(main[:, :4 * n].sum(0), THR)
    mse_t = main[:, 4 * n + 1] / (hw * 6)
    want = {"threshold_metrics": m, "FAR": float(np.mean(far)), "RMSE": float(np.mean(np.sqrt(mse_t))), "MAE": float(main[:, 4 * n].sum() / (hw * 6 * T)),
            "MSE": float(mse_t.mean()), "SSIM": float(main[:, 4 * n + 2].sum() / (area * 6 * T)), "LPIPS": None, "loss_sum": 1.25, "loss_mean": 0.625,
            "batches": 2, "samples": 6, "nonfinite": 0}
    assert _same(plain, want)

    def scores(counts):
        mm, ff = contingency_metrics(counts, THR)
        return {"threshold_metrics": mm, "FAR": float(np.mean(ff))}
    assert list(res["pooled"]) == list(POOLS)
    for i, p in enumerate(POOLS):
        assert _same(res["pooled"][p], scores(ftab[:, i].sum(0)))
        assert _same(res["persistence"]["pooled"][p], scores(btab[:, base.index(p)].sum(0)))
    assert _same({k: res["persistence"][k] for k in ("threshold_metrics", "FAR")}, scores(btab[:, 0].sum(0)))
    assert set(res["persistence"]) == {"threshold_metrics", "FAR", "pooled"}
    lead = res["per_lead"]
    assert set(lead) == {"RMSE", "MAE", "SSIM", "threshold_metrics", "pooled", "persistence"}
    assert (lead["RMSE"] == np.sqrt(mse_t)).all() and (lead["MAE"] == main[:, 4 * n] / (hw * 6)).all() and (lead["SSIM"] == main[:, 4 * n + 2] / (area * 6)).all()
    assert abs(float(np.mean(lead["RMSE"])) - res["RMSE"]) <= 1e-12 and abs(float(np.mean(lead["MAE"])) - res["MAE"]) <= 1e-9
    _check_lead(lead["threshold_metrics"], main[:, :4 * n])
    _check_lead(lead["persistence"]["threshold_metrics"], btab[:, 0])
    for i, p in enumerate(POOLS):
        _check_lead(lead["pooled"][p]["threshold_metrics"], ftab[:, i])
        _check_lead(lead["persistence"]["pooled"][p]["threshold_metrics"], btab[:, base.index(p)])
        # the per-lead counts summed over t are the counts pooled over the horizon
        for thr in THR:
            for name in ("TP", "FN", "FP", "TN"):
                assert lead["pooled"][p]["threshold_metrics"][thr][name].sum() == res["pooled"][p]["threshold_metrics"][thr][name]
                assert lead["persistence"]["pooled"][p]["threshold_metrics"][thr][name].sum() == res["persistence"]["pooled"][p]["threshold_metrics"][thr][name]
    for thr in THR:
        for name in ("TP", "FN", "FP", "TN"):
            assert lead["threshold_metrics"][thr][name].sum() == res["threshold_metrics"][thr][name]


def test_aggregate_variants_and_refusals():
    from adnm_hip.validate import aggregate
    hw, n = 48 * 48, len(THR)
    blk, main, ftab, btab = _hand_block(4, pools=(), persistence=True)     # persistence alone: the baseline at (1, 1)
    res = aggregate(blk, THR, T, hw, None, persistence=True, per_lead=True)
    assert "pooled" not in res and res["persistence"]["pooled"] == {} and res["SSIM"] is None and res["per_lead"]["SSIM"] is None
    assert "pooled" not in res["per_lead"] and res["per_lead"]["persistence"]["pooled"] == {}
    assert res["persistence"]["threshold_metrics"][20]["TP"] == btab[:, 0, 0].sum()
    blk, main, ftab, btab = _hand_block(5, pools=((4, 2),), persistence=False)
    res = aggregate(blk, THR, T, hw, None, pools=((4, 2),))
    assert "persistence" not in res and "per_lead" not in res and res["pooled"][(4, 2)]["threshold_metrics"][40]["TN"] == ftab[:, 0, 15].sum()
    lead = aggregate(blk[:4 + T * (4 * n + 3)], THR, T, hw, None, per_lead=True)["per_lead"]      # per-lead with no new table at all
    assert set(lead) == {"RMSE", "MAE", "SSIM", "threshold_metrics"}
    with pytest.raises(ValueError, match="doubles"):
        aggregate(blk, THR, T, hw, None)
    with pytest.raises(ValueError, match="doubles"):
        aggregate(blk[:4 + T * (4 * n + 3)], THR, T, hw, None, persistence=True)


# ------------------------------------------------------------------------------------------------ the Validator's arguments
def test_validator_arguments():
    import inspect

    import torch
    from adnm_hip.validate import Validator
    from models.loss import enRainfallLoss
    sig = inspect.signature(Validator.__init__).parameters
    assert sig["pools"].default is None and sig["persistence"].default is False
    assert inspect.signature(Validator.done).parameters["per_lead"].default is False
    assert list(inspect.signature(Validator.done).parameters)[:2] == ["self", "reset"]
    model, crit = torch.nn.Identity(), enRainfallLoss()
    val = Validator(model, crit, 20, 255.0)
    passes = lambda v: [(p.field, p.pools) for p in v._parts if p.kind == "pool"]   # the pooled passes, in the order of their tables and launches
    assert val.pools == () and val.persistence is False and passes(val) == [] and [p.name for p in val._parts] == ["main"]
    val = Validator(model, crit, 20, 255.0, pools=(4, 16, (16, 8)), persistence=True)
    assert val.pools == ((4, 4), (16, 16), (16, 8)) and passes(val) == [("pred", val.pools), ("last", ((1, 1),) + val.pools)]
    assert passes(Validator(model, crit, 20, 255.0, persistence=True)) == [("last", ((1, 1),))]
    assert passes(Validator(model, crit, 20, 255.0, pools=(4, 1), persistence=True)) == [("pred", ((4, 4), (1, 1))), ("last", ((1, 1), (4, 4)))]
    for bad in ((0,), ((4, 5),), ((33, 1),), (2, 3, 4, 5, 6), (4.0,), ("4",), ((4, 2, 1),), (4, (4, 4))):
        with pytest.raises(ValueError):
            Validator(model, crit, 20, 255.0, pools=bad)
    with pytest.raises(ValueError, match="persistence"):
        Validator(model, crit, 20, 255.0, pools=(2, 3, 4, 5), persistence=True)     # (1, 1) would be a fifth pool of the baseline's pass
