"""The joint intensity histogram without a GPU: validate.joint_entries and joint_counts_at on known histograms and against the mask-based
yardstick (joint_ref), ops.joint_levels, validate.aggregate with and without the joint tail, the arguments, and the four entry points at
the C boundary (declared, exported, refusing every limit before any launch)."""
import ctypes

import numpy as np
import pytest

import joint_ref as J
from adnm_hip import lib, ops

NEW = ("adnm_valid_joint_levels", "adnm_valid_joint_block_bytes", "adnm_valid_joint_accum_ws_bytes", "adnm_valid_joint_accum")


def _eq(a, b):
    """equal values, NaN equal to NaN, arrays of equal shape and integer arrays of equal kind"""
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


# ------------------------------------------------------------------------------------------------ joint_entries
def test_joint_entries_on_a_hand_written_histogram():
    from adnm_hip.validate import joint_entries
    h = [[5, 1, 0],      # target 0: forecast 0 five times, 1 once
         [2, 3, 1],      # target 1
         [0, 2, 6]]      # target 2
    e = joint_entries(h)
    assert list(e) == ["levels", "histogram", "marginal_target", "marginal_forecast", "curves", "conditional_mean", "qq", "correlation", "mean_error"]
    assert e["levels"] == 3 and e["histogram"].dtype == np.int64 and (e["histogram"] == np.array(h)).all()
    assert e["marginal_target"].dtype == np.int64 and e["marginal_target"].tolist() == [6, 6, 8] and e["marginal_forecast"].tolist() == [7, 6, 7]
    c = e["curves"]
    assert list(c) == ["TP", "FN", "FP", "TN", "CSI", "POD", "FAR", "HSS", "bias"]
    assert c["TP"].tolist() == [20, 12, 6] and c["FN"].tolist() == [0, 2, 2] and c["FP"].tolist() == [0, 1, 1] and c["TN"].tolist() == [0, 5, 11]
    assert all(c[k].dtype == np.int64 for k in ("TP", "FN", "FP", "TN"))
    assert np.allclose(c["CSI"], [1.0, 12 / 15, 6 / 9], rtol=1e-15) and np.allclose(c["POD"], [1.0, 12 / 14, 6 / 8], rtol=1e-15)
    assert np.allclose(c["FAR"], [0.0, 1 / 13, 1 / 7], rtol=1e-15) and np.allclose(c["bias"], [1.0, 13 / 14, 7 / 8], rtol=1e-15)
    hss1 = 2 * (12 * 5 - 1 * 2) / (1 + 4 + 2 * 12 * 5 + 3 * 17)
    hss2 = 2 * (6 * 11 - 1 * 2) / (1 + 4 + 2 * 6 * 11 + 3 * 17)
    assert np.isnan(c["HSS"][0]) and np.allclose(c["HSS"][1:], [hss1, hss2], rtol=1e-15)      # threshold 0: every pixel an event, 0 / 0
    assert np.allclose(e["conditional_mean"], [1 / 6, 5 / 6, 14 / 8], rtol=1e-15)
    # CDF_f = 7, 13, 20 of 20 and CDF_o = 6, 12, 20: the forecast's level 0 maps to 1 (6 < 7), 1 to 2 (12 < 13), 2 to 2
    assert e["qq"].dtype == np.int64 and e["qq"].tolist() == [1, 2, 2]
    so, sf = np.repeat([0, 0, 1, 1, 1, 2, 2], [5, 1, 2, 3, 1, 2, 6]), np.repeat([0, 1, 0, 1, 2, 1, 2], [5, 1, 2, 3, 1, 2, 6])
    assert isinstance(e["correlation"], float) and abs(e["correlation"] - np.corrcoef(so, sf)[0, 1]) < 1e-14
    assert isinstance(e["mean_error"], float) and abs(e["mean_error"] - (20 - 22) / 20) < 1e-15


def test_joint_entries_agrees_with_the_mask_based_yardstick_integer_for_integer():
    from adnm_hip.evaluator import contingency_metrics
    from adnm_hip.validate import joint_entries
    rng = np.random.default_rng(7)
    L, T = 17, 3
    h = rng.integers(0, 50, (T, L, L)) * (rng.random((T, L, L)) < 0.4)
    h[1, 5] = 0               # a level the target never takes
    h[2, :, 9] = 0            # a level the forecast never takes
    lead = joint_entries(h)
    assert lead["levels"] == L and lead["histogram"].shape == (T, L, L) and lead["qq"].shape == (T, L) and lead["correlation"].shape == (T,)
    rows = [(h[t], {k: ({c: a[t] for c, a in v.items()} if k == "curves" else v if k == "levels" else v[t]) for k, v in lead.items()}) for t in range(T)]
    for hist, e in rows + [(h.sum(0), joint_entries(h.sum(0)))]:      # every row of the leading axis, then the sum over it
        cur = e["curves"]
        want = J.curves(hist)
        for k in ("TP", "FN", "FP", "TN"):
            assert cur[k].dtype == np.int64 and (cur[k] == want[k]).all(), k
        assert (cur["TP"] + cur["FN"] + cur["FP"] + cur["TN"] == hist.sum()).all()
        for v in (0, 3, L - 1):
            m, far = contingency_metrics(np.array([want[k][v] for k in ("TP", "FN", "FP", "TN")], dtype=np.float64), [v])
            for k in ("CSI", "POD", "HSS"):
                assert _eq(cur[k][v], m[v][k]), (k, v)
            assert _eq(cur["FAR"][v], far[0])
            with np.errstate(divide="ignore", invalid="ignore"):
                assert _eq(cur["bias"][v], np.float64(want["TP"][v] + want["FP"][v]) / np.float64(want["TP"][v] + want["FN"][v]))
        assert (e["marginal_target"] == hist.sum(1)).all() and (e["marginal_forecast"] == hist.sum(0)).all()
        assert (e["qq"] == J.qq(hist)).all()
        cond, r, me = J.moments(hist)
        assert np.allclose(e["conditional_mean"], cond, rtol=1e-13, atol=0, equal_nan=True) and np.isnan(e["conditional_mean"]).sum() == np.isnan(cond).sum()
        assert abs(e["correlation"] - r) < 1e-12 and abs(e["mean_error"] - me) < 1e-12
    assert np.isnan(lead["conditional_mean"][1, 5]) and np.isfinite(lead["conditional_mean"][0]).all()


def test_qq_of_equal_marginals_is_the_identity_and_a_constant_field_has_no_correlation():
    from adnm_hip.validate import joint_entries
    rng = np.random.default_rng(9)
    a = rng.integers(1, 9, (6, 6))
    sym = a + a.T                                   # equal marginals, every level taken
    e = joint_entries(sym)
    assert (e["marginal_target"] == e["marginal_forecast"]).all() and e["qq"].tolist() == list(range(6)) and e["mean_error"] == 0.0
    diag = np.diag([4, 0, 3, 9])                    # forecast == target: r = 1, bias 1 wherever there is an event
    e = joint_entries(diag)
    assert abs(e["correlation"] - 1.0) < 1e-15 and (e["curves"]["bias"] == 1.0).all() and (e["curves"]["CSI"] == 1.0).all()
    assert e["qq"].tolist() == [0, 0, 2, 3], "level 1 is never taken: CDF_f(1) = CDF_f(0), which CDF_o reaches at 0 already"
    const = np.zeros((4, 4), dtype=np.int64)
    const[2, :] = [1, 2, 3, 4]                      # the target is always 2
    e = joint_entries(const)
    assert np.isnan(e["correlation"]) and np.isnan(e["conditional_mean"][[0, 1, 3]]).all() and e["conditional_mean"][2] == 2.0
    empty = joint_entries(np.zeros((3, 3)))
    assert np.isnan(empty["correlation"]) and np.isnan(empty["mean_error"]) and (empty["curves"]["TP"] == 0).all()
    for bad in (np.zeros((3, 4)), np.zeros(3), [[0.5, 0], [0, 1]], [[-1, 0], [0, 1]], [[np.nan, 0], [0, 1]]):
        with pytest.raises(ValueError, match="joint"):
            joint_entries(bad)


def test_joint_counts_at_any_threshold():
    from adnm_hip.validate import joint_counts_at, joint_entries
    rng = np.random.default_rng(11)
    L = 91
    h = rng.integers(0, 9, (2, L, L))
    for thr, v in ((19.5, 20), (20, 20), (20.0001, 21), (0.25, 1), (90, 90)):
        got = joint_counts_at(h, thr)
        for t in range(2):
            assert tuple(int(g[t]) for g in got) == J.counts_at(h[t], v), (thr, t)
        assert all(g.dtype == np.int64 and g.shape == (2,) for g in got)
    one = joint_counts_at(h[0], 35)
    assert all(isinstance(g, int) for g in one) and one == J.counts_at(h[0], 35)
    cur = joint_entries(h[0])["curves"]
    assert one == tuple(int(cur[k][35]) for k in ("TP", "FN", "FP", "TN"))
    n = int(h[0].sum())
    assert joint_counts_at(h[0], 90.5) == (0, 0, 0, n) and joint_counts_at(h[0], 1e9) == (0, 0, 0, n) and joint_counts_at(h[0], float("inf")) == (0, 0, 0, n)
    assert joint_counts_at(h[0], 0) == (n, 0, 0, 0) and joint_counts_at(h[0], -3.5) == (n, 0, 0, 0)
    with pytest.raises(ValueError):
        joint_counts_at(h[0], float("nan"))
    import torch
    assert joint_counts_at(torch.from_numpy(h[0]), 19.5) == J.counts_at(h[0], 20)


# ------------------------------------------------------------------------------------------------ the levels
def test_joint_levels():
    for scale, L in ((1, 2), (89.5, 90), (90, 91), (127, 128), (127.99, 128), (1.5, 2), (255.0 / 3, 86)):
        assert ops.joint_levels(scale) == L == J.levels(scale) and isinstance(ops.joint_levels(scale), int), scale
    for bad in (128, 0.5, float("nan"), float("inf"), -float("inf"), 0, -90, 255.0, 0.999, "ninety", None):
        with pytest.raises(ValueError, match="2 <= floor"):
            ops.joint_levels(bad)


# ------------------------------------------------------------------------------------------------ aggregate
T, THR, HW = 3, [20, 30, 35, 40], 16 * 64


def _hand_block(seed, L, extra=0):
    """header, main table, `extra` doubles of other tables, then a joint table (T, L, L)"""
    from adnm_hip.validate import block_doubles
    rng = np.random.default_rng(seed)
    n = len(THR)
    main = rng.integers(1, 1 << 20, (T, 4 * n + 3)).astype(np.float64)
    main[:, 4 * n:] += rng.random((T, 3))
    tab = (rng.integers(0, 1 << 16, (T, L, L)) * (rng.random((T, L, L)) < 0.3)).astype(np.float64)
    blk = np.concatenate([[1.25, 2, 6, 0], main.ravel(), rng.integers(0, 1 << 20, extra).astype(np.float64), tab.ravel()])
    assert blk.shape == (block_doubles(T, n)[0] + extra + T * L * L,)
    return blk, tab


def test_aggregate_with_and_without_the_joint_tail():
    from adnm_hip.validate import aggregate, fss_doubles, joint_doubles, joint_entries, spectrum_doubles
    n, fss, frame, L = len(THR), (1, 5), (16, 64), 91
    assert joint_doubles(T) == joint_doubles(T, None) == joint_doubles(T, False) == 0 and joint_doubles(T, 90.0) == T * 91 * 91 == joint_doubles(T, 90.9)
    assert joint_doubles(20, 89.5) == 20 * 90 * 90
    with pytest.raises(ValueError):
        joint_doubles(T, 128.0)
    extra = sum(fss_doubles(T, n, fss)) + spectrum_doubles(T, frame)
    blk, tab = _hand_block(1, L, extra=extra)
    res = aggregate(blk, THR, T, HW, None, fss=fss, per_lead=True, spectrum=frame, joint=L)
    former = aggregate(blk[:-tab.size], THR, T, HW, None, fss=fss, per_lead=True, spectrum=frame)
    assert list(res) == list(former)[:-1] + ["joint", "per_lead"] and list(res["per_lead"]) == list(former["per_lead"]) + ["joint"]
    assert _same_tree({k: res[k] for k in former if k != "per_lead"}, {k: former[k] for k in former if k != "per_lead"})
    assert _same_tree({k: res["per_lead"][k] for k in former["per_lead"]}, former["per_lead"])
    assert _same_tree(res["joint"], joint_entries(tab.sum(axis=0))) and _same_tree(res["per_lead"]["joint"], joint_entries(tab))
    assert res["joint"]["histogram"].shape == (L, L) and res["joint"]["histogram"].dtype == np.int64 and res["per_lead"]["joint"]["histogram"].shape == (T, L, L)
    assert res["per_lead"]["joint"]["curves"]["bias"].shape == (T, L) and res["per_lead"]["joint"]["mean_error"].shape == (T,)
    short = aggregate(blk, THR, T, HW, None, fss=fss, spectrum=frame, joint=L)
    assert "per_lead" not in short and _same_tree(short["joint"], res["joint"])
    plain_n = 4 + T * (4 * n + 3)
    alone = aggregate(np.concatenate([blk[:plain_n], tab.ravel()]), THR, T, HW, None, per_lead=True, joint=L)
    assert _same_tree(alone["joint"], res["joint"]) and _same_tree(alone["per_lead"]["joint"], res["per_lead"]["joint"])
    plain = aggregate(blk[:plain_n], THR, T, HW, None)
    assert list(plain) == ["threshold_metrics", "FAR", "RMSE", "MAE", "MSE", "SSIM", "LPIPS", "loss_sum", "loss_mean", "batches", "samples", "nonfinite"]
    with pytest.raises(ValueError, match="doubles"):
        aggregate(blk, THR, T, HW, None, fss=fss, spectrum=frame)                    # the tail is there, the argument is not
    with pytest.raises(ValueError, match="joint histogram of 90 levels"):
        aggregate(blk, THR, T, HW, None, fss=fss, spectrum=frame, joint=90)          # another L, another table
    with pytest.raises(ValueError, match="doubles"):
        aggregate(blk[:-1], THR, T, HW, None, fss=fss, spectrum=frame, joint=L)
    with pytest.raises(ValueError, match="joint"):
        aggregate(blk, THR, T, HW, None, fss=fss, spectrum=frame, joint=129)
    with pytest.raises(ValueError, match="joint"):
        aggregate(blk, THR, T, HW, None, fss=fss, spectrum=frame, joint=1)


def test_the_curves_of_a_consistent_block_equal_its_threshold_metrics():
    """a main table built from the joint table's own counts: the two routes to TP / FN / FP / TN agree integer for integer"""
    from adnm_hip.validate import aggregate, joint_counts_at
    L, n = 91, len(THR)
    blk, tab = _hand_block(4, L)
    main = blk[4:4 + T * (4 * n + 3)].reshape(T, 4 * n + 3)
    for k, thr in enumerate(THR):
        main[:, 4 * k:4 * k + 4] = np.stack(joint_counts_at(tab, thr), axis=1)
    res = aggregate(blk, THR, T, HW, None, per_lead=True, joint=L)
    for thr in THR:
        for k in ("TP", "FN", "FP", "TN"):
            assert res["threshold_metrics"][thr][k] == res["joint"]["curves"][k][thr]
            assert (res["per_lead"]["threshold_metrics"][thr][k] == res["per_lead"]["joint"]["curves"][k][:, thr]).all()
        for k in ("CSI", "POD", "HSS"):
            assert res["threshold_metrics"][thr][k] == res["joint"]["curves"][k][thr], (thr, k)


# ------------------------------------------------------------------------------------------------ the arguments
def test_validator_arguments():
    import inspect

    import torch
    from adnm_hip.validate import Validator
    from models.loss import enRainfallLoss
    params = list(inspect.signature(Validator.__init__).parameters)
    assert params[-1] == "joint" and inspect.signature(Validator.__init__).parameters["joint"].default is False
    from adnm_hip.validate import aggregate
    assert list(inspect.signature(aggregate).parameters)[-1] == "joint" and inspect.signature(aggregate).parameters["joint"].default is None
    model, crit = torch.nn.Identity(), enRainfallLoss()
    assert Validator(model, crit, 20, 255.0).joint is False                      # without joint, value_scale = 255 stays fine
    val = Validator(model, crit, 20, 90.0, joint=True)
    assert val.joint is True and val._levels == 91
    for bad in (255.0, 128.0, 0.5):
        with pytest.raises(ValueError, match="2 <= floor"):
            Validator(model, crit, 20, bad, joint=True)


def test_joint_histogram_refuses_what_is_not_two_gpu_tensors():
    import torch
    a = torch.zeros(2, 8, 8)
    with pytest.raises(RuntimeError):
        ops.joint_histogram(a, a, 90.0)                    # CPU tensors
    with pytest.raises(RuntimeError):
        ops.joint_histogram(a.numpy(), a.numpy(), 90.0)


# ------------------------------------------------------------------------------------------------ the C boundary
def test_new_prototypes_are_declared_and_exported():
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/adnm_hip.h"
        assert hasattr(so, name), f"{name} declared but not exported"
    assert protos["adnm_valid_joint_levels"] == ("int64_t", ["float"])
    assert protos["adnm_valid_joint_block_bytes"] == ("int64_t", ["int64_t", "float"])
    assert protos["adnm_valid_joint_accum_ws_bytes"] == ("int64_t", ["int64_t", "int64_t", "int64_t", "float"])
    assert protos["adnm_valid_joint_accum"] == ("int", ["const float*", "int64_t", "int64_t", "const float*", "void*", "float", "void*", "int64_t", "int64_t",
                                                        "int64_t", "int64_t", "adnm_stream_t"])


def test_the_three_queries():
    q = lib.query
    lev, blk, ws = "adnm_valid_joint_levels", "adnm_valid_joint_block_bytes", "adnm_valid_joint_accum_ws_bytes"
    assert [q(lev, s) for s in (1.0, 89.5, 90.0, 127.0, 127.99)] == [2, 90, 91, 128, 128]
    for bad in (128.0, 0.5, float("nan"), float("inf"), -float("inf"), 0.0, -90.0, 255.0):
        assert q(lev, bad) == -1 and q(blk, 20, bad) == -1 and q(ws, 40, 20, 4096, bad) == -1, bad
    assert q(blk, 20, 90.0) == 8 * 20 * 91 * 91 and q(blk, 1, 1.0) == 8 * 4 and q(blk, 3, 127.99) == 8 * 3 * 128 * 128
    assert q(blk, 0, 90.0) == -1 and q(blk, -1, 90.0) == -1
    need = q(ws, 80, 20, 128 * 128, 90.0)
    assert need >= 0 and need % 8 == 0, "0 is a valid answer"
    assert q(ws, 1, 1, 1, 90.0) >= 0 and q(ws, 65535, 1, 1, 90.0) >= 0 and q(ws, 4, 2, (1 << 24) - 1, 90.0) >= 0
    assert q(ws, 80, 7, 4096, 90.0) == -1, "T does not divide frames"
    assert q(ws, 80, 0, 4096, 90.0) == -1 and q(ws, 80, -1, 4096, 90.0) == -1, "T < 1"
    assert q(ws, 0, 1, 4096, 90.0) == -1, "no frame"
    assert q(ws, 65536, 1, 64, 90.0) == -1, "frames > 65535"
    assert q(ws, 4, 2, 0, 90.0) == -1 and q(ws, 4, 2, -5, 90.0) == -1 and q(ws, 4, 2, 1 << 24, 90.0) == -1, "hw"


def test_every_limit_is_refused_on_the_host_with_its_own_message():
    """fake addresses: anything that reached a launch would fault, and the stream is never touched"""
    so = lib.load()
    need = lib.query("adnm_valid_joint_accum_ws_bytes", 40, 20, 4096, 90.0)

    def call(pred=16, ss=20 * 4096, fs=4096, tgt=32, table=64, scale=90.0, ws=128, ws_bytes=1 << 40, frames=40, T=20, hw=4096):
        rc = so.adnm_valid_joint_accum(pred, ss, fs, tgt, table, scale, ws, ws_bytes, frames, T, hw, None)
        return rc, lib.last_error()

    cases = [(dict(pred=None), "null pointer"), (dict(tgt=None), "null pointer"), (dict(table=None), "null pointer"),
             (dict(pred=18), "4-byte aligned"), (dict(tgt=34), "4-byte aligned"), (dict(table=68), "table must be 8-byte aligned"),
             (dict(ws=132), "workspace must be 8-byte aligned"),
             (dict(scale=128.0), "value_scale must be finite"), (dict(scale=0.5), "value_scale must be finite"), (dict(scale=float("nan")), "value_scale must be finite"),
             (dict(scale=float("inf")), "value_scale must be finite"), (dict(scale=255.0), "value_scale must be finite"),
             (dict(T=0), "must divide frames"), (dict(T=7), "must divide frames"), (dict(frames=0), "must divide frames"),
             (dict(frames=65540, T=20), "frames <= 65535"),
             (dict(hw=0, fs=0), "hw < 2^24"), (dict(hw=1 << 24, fs=1 << 24), "hw < 2^24"), (dict(hw=-4), "hw < 2^24"),
             (dict(fs=4095), "pred_frame_stride"), (dict(fs=-4096), "pred_frame_stride"),
             (dict(ss=-1), "pred_sample_stride"),
             (dict(ws_bytes=need - 1), "workspace")]
    if need:
        cases.append((dict(ws=None), "null pointer"))
    for kw, text in cases:
        rc, err = call(**kw)
        assert rc == -1 and text in err and "valid_joint_accum" in err, (kw, rc, err)
    assert len({text for _, text in cases}) == 11, "one message per limit"
