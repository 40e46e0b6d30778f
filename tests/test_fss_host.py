"""The Fractions Skill Score without a GPU: the CPU yardstick checks itself (a plain window loop, scipy's uniform_filter), the three
entry points at the C boundary (declared, exported, additive, refusing every limit before any launch), validate.aggregate on a
hand-made block, and the Validator's and ops.fss_scales' arguments."""
import ctypes

import numpy as np
import pytest

import fss_ref as F
import verify_ref as R
from adnm_hip import lib

NEW = ("adnm_valid_fss_block_bytes", "adnm_valid_fss_accum_ws_bytes", "adnm_valid_fss_accum")


# ------------------------------------------------------------------------------------------------ the helper
def _planted(n, H, W, seed):
    t, p = (a.copy() for a in R.radar_fields(n, H, W, seed))
    t[0, 0, 0], p[0, H - 1, W - 1], p[1, 4, 4], t[1, 2, 3] = 1.5, 0.9, float("nan"), float("-inf")
    return t, p


def test_conv_reference_equals_a_plain_window_loop():
    t, p = _planted(2, 9, 11, 0)
    scales = (1, 3, 5, 9, 33)        # 33: every window is larger than the frame
    a, b = F.ref_sums(t, p, R.THR, R.SCALE, scales), F.loop_sums(t, p, R.THR, R.SCALE, scales)
    assert a.shape == (2, 5, 12) and (a == b).all()
    assert (a[:, :, 0::3] > 0).any() and (a[:, :, 2::3] > 0).any(), "no event at all: nothing is compared"
    # a window that covers the whole frame counts every event at every pixel: A = (events)^2 * H * W
    ev = (R.quant(t, R.SCALE) >= 20).sum(axis=(1, 2)).astype(np.float64)
    assert (a[:, 4, 0] == ev * ev * 99).all()


def test_conv_reference_equals_scipy_uniform_filter():
    from scipy import ndimage
    t, p = _planted(3, 37, 53, 1)
    qt, qp = R.quant(t, R.SCALE), R.quant(p, R.SCALE)
    scales = (1, 3, 9, 17, 33)
    ref = F.ref_sums(t, p, R.THR, R.SCALE, scales)
    for i, n in enumerate(scales):
        for k, thr in enumerate(R.THR):
            co, cf = (np.rint(np.stack([ndimage.uniform_filter((q[f] >= thr).astype(np.float64), size=n, mode="constant", cval=0.0) for f in range(3)])
                              * n * n) for q in (qt, qp))
            got = np.stack([(co * co).sum((1, 2)), (cf * cf).sum((1, 2)), (co * cf).sum((1, 2))], axis=1)
            assert (got == ref[:, i, 3 * k:3 * k + 3]).all(), (n, thr)
    # pysteps' statement of the score, 1 - sum (f - o)^2 / (sum o^2 + sum f^2) on the fractions, is 2C / (A + F)
    n, thr = 9, 30
    fo, ff = (ndimage.uniform_filter((q[0] >= thr).astype(np.float64), size=n, mode="constant", cval=0.0) for q in (qt, qp))
    want = 1.0 - ((ff - fo) ** 2).sum() / ((fo ** 2).sum() + (ff ** 2).sum())
    assert abs(F.fss(ref[0, 2])[1] - want) <= 1e-12


def test_the_listed_cases_are_dense_and_the_eight_thresholds_are_not():
    for case in F.CASES:
        t, p = F.radar_fields(*case)
        for name in ("one", "default"):
            F.assert_dense(F.ref_sums(t, p, F.THR_SETS[name], F.SCALE, (1, 33)), f"{case} {name}")
    t, p = F.radar_fields(*F.CASES[0])
    cells = F.ref_sums(t, p, F.THR_SETS["eight"], F.SCALE, (1, 5)).sum(axis=0)
    assert (cells[:, 3 * 7 + 1:] == 0).all() and cells[0, 3 * 7] > 0, "threshold 70: the forecast has no event, the target has"
    with pytest.raises(AssertionError, match="do not weaken"):
        F.assert_dense(F.ref_sums(t, p, F.THR_SETS["eight"], F.SCALE, (1, 5)))
    only_obs = np.zeros((1, 1, 3))
    assert np.isnan(F.fss(only_obs)).all() and F.fss(np.array([4.0, 0.0, 0.0]))[0] == 0.0


# ------------------------------------------------------------------------------------------------ the C boundary
def test_new_prototypes_are_declared_and_exported_and_the_abi_version_stays():
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/adnm_hip.h"
        assert hasattr(so, name), f"{name} declared but not exported"
    assert protos["adnm_valid_fss_accum"][0] == "int" and protos["adnm_valid_fss_accum"][1][-1] == "adnm_stream_t"
    assert len(protos["adnm_valid_fss_accum"][1]) == len(protos["adnm_valid_pool_accum"][1]) == 17
    assert protos["adnm_valid_fss_block_bytes"][0] == protos["adnm_valid_fss_accum_ws_bytes"][0] == "int64_t"
    assert lib.load().adnm_abi_version() == 11


def _scales(*ns):
    return lib.i64_table(list(ns))


def test_byte_queries():
    q = lib.query
    assert q("adnm_valid_fss_block_bytes", 20, 4, 3) == 8 * 20 * 3 * 12
    assert q("adnm_valid_fss_block_bytes", 1, 8, 4) == 8 * 4 * 24
    for bad in ((0, 4, 3), (65536, 4, 3), (20, 0, 3), (20, 9, 3), (20, 4, 0), (20, 4, 5)):
        assert q("adnm_valid_fss_block_bytes", *bad) == -1, bad
    ok = _scales(1, 33)
    ws = "adnm_valid_fss_accum_ws_bytes"
    # 16 tiles of 32 x 32 window centres per 128 x 128 frame, per scale and threshold three uint32 (A, F, C)
    assert q(ws, 80, 20, 128, 128, 4, ok, 2) == 80 * 16 * 2 * 12 * 4
    assert q(ws, 6, 6, 37, 53, 4, ok, 2) == 6 * 4 * 2 * 12 * 4
    assert q(ws, 2, 1, 5, 40, 8, ok, 2) == 2 * 2 * 2 * 24 * 4, "a window larger than the frame is allowed"
    assert q(ws, 1, 1, 1, 1, 1, _scales(33), 1) == 12
    assert q(ws, 80, 7, 128, 128, 4, ok, 2) == -1, "T does not divide frames"
    assert q(ws, 80, 0, 128, 128, 4, ok, 2) == -1, "T = 0"
    assert q(ws, 65540, 20, 128, 128, 4, ok, 2) == -1, "frames > 65535"
    assert q(ws, 80, 20, 128, 128, 0, ok, 2) == -1 and q(ws, 80, 20, 128, 128, 9, ok, 2) == -1
    assert q(ws, 80, 20, 128, 128, 4, ok, 0) == -1 and q(ws, 80, 20, 128, 128, 4, _scales(1, 3, 5, 7, 9), 5) == -1
    assert q(ws, 80, 20, 128, 128, 4, None, 2) == -1, "no scales"
    assert q(ws, 80, 20, 4096, 4096, 4, ok, 2) == -1, "H*W >= 2^24"
    assert q(ws, 80, 20, 4, 40000, 4, ok, 1) == -1 and q(ws, 80, 20, 40000, 4, 4, ok, 1) == -1, "H or W >= 32768"
    assert q(ws, 80, 20, 0, 16, 4, ok, 1) == -1 and q(ws, 80, 20, 16, 0, 4, ok, 1) == -1
    for bad in (0, 2, 32, 34, 35, -1):
        assert q(ws, 80, 20, 128, 128, 4, _scales(bad), 1) == -1, bad
    assert q(ws, 80, 20, 128, 128, 4, _scales(5, 9, 5), 3) == -1, "a scale twice"


def test_every_limit_is_refused_on_the_host_with_its_own_message():
    """fake addresses: anything that reached a launch would fault, and the stream is never touched"""
    so = lib.load()
    thr, ok = (ctypes.c_float * 4)(20, 30, 35, 40), _scales(1, 33)

    def call(pred=16, ss=20 * 64 * 64, fs=64 * 64, tgt=32, table=64, thr_=thr, nthr=4, scales=ok, nscale=2, ws=128, ws_bytes=1 << 30, frames=40, T=20, H=64, W=64):
        rc = so.adnm_valid_fss_accum(pred, ss, fs, tgt, table, thr_, nthr, 90.0, scales, nscale, ws, ws_bytes, frames, T, H, W, None)
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
        assert rc == -1 and text in err and "valid_fss_accum" in err, (kw, rc, err)
    assert len({text for _, text in cases}) == 13, "one message per limit"
    rc, err = call(ws_bytes=8)
    assert rc == -3 and "workspace" in err
    rc, err = call(ws=None)
    assert rc == -3 and "workspace" in err


# ------------------------------------------------------------------------------------------------ aggregate
T, THR, POOLS, FSS = 5, [20, 30, 35, 40], ((4, 4), (16, 8)), (1, 5, 33)


def _hand_block(seed, pools=POOLS, persistence=True, fss=FSS):
    """an integer block: header, main table, the two pooled tables, the two FSS tables (C <= sqrt(A F), as Cauchy-Schwarz has it)"""
    from adnm_hip.validate import block_doubles, fss_doubles
    rng = np.random.default_rng(seed)
    n = len(THR)
    n0, n1, n2 = block_doubles(T, n, pools, persistence)
    n3, n4 = fss_doubles(T, n, fss, persistence)
    main = rng.integers(1, 1 << 20, (T, 4 * n + 3)).astype(np.float64)
    main[:, 4 * n:] += rng.random((T, 3))
    tabs = rng.integers(1, 1 << 20, (n3 + n4) // 3 * 3).astype(np.float64).reshape(-1, 3)
    tabs[:, 2] = np.floor(np.sqrt(tabs[:, 0] * tabs[:, 1]) * rng.random(len(tabs)))
    blk = np.concatenate([[1.25, 2, 6, 0], main.ravel(), rng.integers(0, 1 << 20, n1 + n2).astype(np.float64), tabs.ravel()])
    assert blk.shape == (n0 + n1 + n2 + n3 + n4,)
    at = n0 + n1 + n2
    return blk, main, blk[at:at + n3].reshape(T, len(fss), 3 * n), blk[at + n3:].reshape(T, len(fss) if persistence else 0, 3 * n)


def _same(a, b):
    return repr(a) == repr(b)


def _score(a, f, c):
    return float(np.float64(2.0 * c) / np.float64(a + f)) if a + f > 0 else float("nan")


def _check(res_fss, lead_fss, tab):
    assert list(res_fss) == list(FSS)
    for i, n in enumerate(FSS):
        assert list(res_fss[n]) == THR
        for k, thr in enumerate(THR):
            a, f, c = (tab[:, i, 3 * k + j].sum() for j in range(3))
            assert _same(res_fss[n][thr], _score(a, f, c)), (n, thr)
            assert 0.0 <= res_fss[n][thr] <= 1.0
            rows = lead_fss[n][thr]
            assert rows.shape == (T,) and rows.dtype == np.float64
            for t in range(T):
                assert _same(float(rows[t]), _score(*tab[t, i, 3 * k:3 * k + 3])), (n, thr, t)


def test_aggregate_with_fss_alone():
    from adnm_hip.validate import aggregate
    hw, area, n = 48 * 48, 38 * 38, len(THR)
    blk, main, ftab, btab = _hand_block(3, pools=(), persistence=False)
    assert btab.size == 0
    res = aggregate(blk, THR, T, hw, area, fss=FSS, per_lead=True)
    plain = aggregate(blk[:4 + T * (4 * n + 3)], THR, T, hw, area, per_lead=True)
    assert set(res) == set(plain) | {"fss", "fss_useful"} and set(res["per_lead"]) == set(plain["per_lead"]) | {"fss"}
    assert _same({k: res[k] for k in plain if k != "per_lead"}, {k: plain[k] for k in plain if k != "per_lead"})
    assert _same({k: res["per_lead"][k] for k in plain["per_lead"]}, plain["per_lead"])
    _check(res["fss"], res["per_lead"]["fss"], ftab)
    cells = main[:, :4 * n].sum(0)
    for k, thr in enumerate(THR):
        f_o = (cells[4 * k] + cells[4 * k + 1]) / cells[4 * k:4 * k + 4].sum()
        assert abs(res["fss_useful"][thr] - (0.5 + f_o / 2)) <= 1e-15 and 0.5 < res["fss_useful"][thr] < 1.0
    short = aggregate(blk, THR, T, hw, area, fss=FSS)
    assert "per_lead" not in short and _same(short["fss"], res["fss"])


def test_aggregate_with_pools_persistence_and_fss_together():
    from adnm_hip.validate import aggregate, block_doubles
    hw, area, n = 48 * 48, 38 * 38, len(THR)
    blk, main, ftab, btab = _hand_block(4)
    res = aggregate(blk, THR, T, hw, area, pools=POOLS, persistence=True, per_lead=True, fss=FSS)
    # the former result for the former arguments, key for key: the block without the FSS tables
    former = aggregate(blk[:sum(block_doubles(T, n, POOLS, True))], THR, T, hw, area, pools=POOLS, persistence=True, per_lead=True)
    assert list(former) == ["threshold_metrics", "FAR", "RMSE", "MAE", "MSE", "SSIM", "LPIPS", "loss_sum", "loss_mean", "batches", "samples", "nonfinite",
                            "pooled", "persistence", "per_lead"]
    assert set(res) == set(former) | {"fss", "fss_useful"}
    for k in former:
        if k not in ("persistence", "per_lead"):
            assert _same(res[k], former[k]), k
    assert set(res["persistence"]) == set(former["persistence"]) | {"fss"} == {"threshold_metrics", "FAR", "pooled", "fss"}
    assert _same({k: res["persistence"][k] for k in former["persistence"]}, former["persistence"])
    lead, old = res["per_lead"], former["per_lead"]
    assert set(lead) == set(old) | {"fss"} and set(lead["persistence"]) == set(old["persistence"]) | {"fss"}
    assert _same({k: lead[k] for k in old if k != "persistence"}, {k: old[k] for k in old if k != "persistence"})
    assert _same({k: lead["persistence"][k] for k in old["persistence"]}, old["persistence"])
    _check(res["fss"], lead["fss"], ftab)
    _check(res["persistence"]["fss"], lead["persistence"]["fss"], btab)
    assert not _same(res["fss"], res["persistence"]["fss"])


def test_aggregate_scale_one_identity_and_the_empty_cell():
    """n = 1: A = TP + FN, F = TP + FP, C = TP, so FSS = 2 TP / (2 TP + FN + FP); A + F = 0 gives NaN"""
    from adnm_hip.validate import aggregate
    hw, n = 48 * 48, len(THR)
    blk, main, ftab, btab = _hand_block(5, pools=(), persistence=False, fss=(1,))
    for k in range(n):
        tp, fn, fp = main[:, 4 * k], main[:, 4 * k + 1], main[:, 4 * k + 2]
        ftab[:, 0, 3 * k], ftab[:, 0, 3 * k + 1], ftab[:, 0, 3 * k + 2] = tp + fn, tp + fp, tp
    ftab[:, 0, 9:12] = 0.0          # threshold 40: no event in either field over the whole epoch
    ftab[2, 0, 3:6] = 0.0           # threshold 30: none at frame index 2 only
    res = aggregate(blk, THR, T, hw, None, per_lead=True, fss=(1,))
    for k, thr in enumerate(THR[:3]):
        m = res["threshold_metrics"][thr]
        if k != 1:
            assert abs(res["fss"][1][thr] - 2 * m["TP"] / (2 * m["TP"] + m["FN"] + m["FP"])) <= 1e-15
    assert np.isnan(res["fss"][1][40]) and np.isnan(res["per_lead"]["fss"][1][40]).all()
    rows = res["per_lead"]["fss"][1][30]
    assert np.isnan(rows[2]) and np.isfinite(np.delete(rows, 2)).all() and np.isfinite(res["fss"][1][30])


def test_aggregate_former_result_and_refusals():
    from adnm_hip.validate import aggregate, block_doubles, fss_doubles
    hw, n = 48 * 48, len(THR)
    assert block_doubles(T, n) == (4 + T * (4 * n + 3), 0, 0) and block_doubles(T, n, POOLS, True) == (4 + T * 19, T * 2 * 16, T * 3 * 16)
    assert fss_doubles(T, n) == (0, 0) and fss_doubles(T, n, FSS) == (T * 3 * 12, 0) and fss_doubles(T, n, FSS, True) == (T * 3 * 12, T * 3 * 12)
    blk, main, ftab, btab = _hand_block(6)
    with pytest.raises(ValueError, match="doubles"):
        aggregate(blk, THR, T, hw, None, pools=POOLS, persistence=True)                       # the FSS tables are there, the argument is not
    with pytest.raises(ValueError, match="fss"):
        aggregate(blk, THR, T, hw, None, pools=POOLS, persistence=True, fss=(1, 5))
    with pytest.raises(ValueError, match="doubles"):
        aggregate(blk[:4 + T * (4 * n + 3)], THR, T, hw, None, fss=FSS)
    res = aggregate(blk[:4 + T * (4 * n + 3)], THR, T, hw, None)
    assert list(res) == ["threshold_metrics", "FAR", "RMSE", "MAE", "MSE", "SSIM", "LPIPS", "loss_sum", "loss_mean", "batches", "samples", "nonfinite"]


# ------------------------------------------------------------------------------------------------ the arguments
def test_fss_scales():
    from adnm_hip import ops
    assert ops.fss_scales(None) == () and ops.fss_scales(()) == ()
    assert ops.fss_scales(5) == (5,) and ops.fss_scales(np.int64(33)) == (33,)
    assert ops.fss_scales([1, 5, 17, 33]) == (1, 5, 17, 33) and ops.fss_scales(iter((9, 3))) == (9, 3)
    assert all(type(n) is int for n in ops.fss_scales(np.array([1, 3])))
    for bad in (0, 2, 35, -3, (4,), (1, 1), (3, 5, 3), (1, 3, 5, 7, 9), (5.0,), 5.0, ("5",), "5", True, (True,), ((3, 1),)):
        with pytest.raises(ValueError):
            ops.fss_scales(bad)
    assert list(ops.fss_table((1, 33))) == [1, 33]


def test_validator_arguments():
    import inspect

    import torch
    from adnm_hip.validate import Validator
    from models.loss import enRainfallLoss
    assert inspect.signature(Validator.__init__).parameters["fss"].default is None
    model, crit = torch.nn.Identity(), enRainfallLoss()
    val = Validator(model, crit, 20, 255.0)
    pool = lambda v: [(p.field, p.pools) for p in v._parts if p.kind == "pool"]   # the pooled and the FSS passes, in the order of their tables and launches
    fss = lambda v: [p.field for p in v._parts if p.kind == "fss"]
    assert val.fss == () and fss(val) == [] and pool(val) == []
    val = Validator(model, crit, 20, 255.0, fss=(1, 5, 17, 33))
    assert val.fss == (1, 5, 17, 33) and fss(val) == ["pred"] and pool(val) == []
    val = Validator(model, crit, 20, 255.0, fss=9, persistence=True, pools=(4,))
    assert val.fss == (9,) and fss(val) == ["pred", "last"] and pool(val) == [("pred", ((4, 4),)), ("last", ((1, 1), (4, 4)))]
    for bad in ((2,), (35,), (5, 5), (1, 3, 5, 7, 9), (4.0,), "5"):
        with pytest.raises(ValueError):
            Validator(model, crit, 20, 255.0, fss=bad)
