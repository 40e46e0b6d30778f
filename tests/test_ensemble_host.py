"""The ensemble without a GPU: the yardstick (ensemble_ref) against two independent forms of the CRPS, validate.ensemble_entries on the
yardstick's own tables, the table's place in the Validator's block, the member recipe, the entry points at the C boundary (declared,
exported, refusing every limit before any launch), the symmetries and their stated inverses, and the arguments."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import ensemble_ref as E
import nprob_ref as N
from adnm_hip import lib, ops
from adnm_hip import validate as V

NEW = ("adnm_d4_members", "adnm_valid_ens_block_bytes", "adnm_valid_ens_accum_ws_bytes", "adnm_valid_ens_accum", "adnm_ensemble_product")
THR, SCALE = [20.0, 30.0, 35.0, 40.0], 90.0


def _half_dry(M, seed, frames=3, H=13, W=17):
    """half the pixels dry in the target and every member, the rest noise over every level"""
    t, m = E.noise_stack(M, frames, H, W, seed)
    wet = np.random.default_rng(seed + 100).uniform(size=t.shape) < 0.5
    return np.where(wet, t, 0).astype(np.float32), np.where(wet[None], m, 0).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the yardstick on its own
@pytest.mark.parametrize("M", [2, 3, 8, 16])
def test_the_yardstick_equals_the_integral_of_the_squared_cdf_difference_and_the_sorted_form(M):
    for scale in (90.0, 255.0, 1.0):
        t, m = _half_dry(M, 3 * M)
        rows = E.frame_rows(t, m, THR, scale).sum(axis=0)
        n, z, s0, s1, s2 = (int(v) for v in rows[:5])
        assert n == t.size and 0.4 * n < z < (0.6 * n if scale > 1.0 else n), "half the pixels are dry (at a scale of 1 nearly all levels are 0)"
        assert M * s1 - s2 == E.crps_integral(t, m, scale), "M S1 - S2 is the integral of the squared CDF difference"
        assert s2 == E.s2_sorted(m, scale), "S2 from the sorted members"
        x = E.quantise(m, scale).astype(np.float64)
        assert rows[5] == round(float((M * M * x.var(axis=0)).sum())) and s0 == int(np.abs(E.quantise(m[0], scale) - E.quantise(t, scale)).sum())
        assert rows[6] == round(float(((x.sum(axis=0) - M * E.quantise(t, scale)) ** 2).sum()))
        at = 7 + (M + 1) ** 2
        assert rows[7:at].sum() == n - z and all(rows[at + 2 * k * (M + 1):at + 2 * (k + 1) * (M + 1)].sum() == n - z for k in range(4))


def test_the_yardstick_quantises_as_the_kernels_do():
    v = np.array([np.nan, -np.inf, -0.5, -0.0, 0.0, 0.5, 1.0, 1.5, np.inf, 0.999999], dtype=np.float32)
    assert E.quantise(v, 90.0).tolist() == [0, 0, 0, 0, 0, 45, 90, 90, 90, 89] and E.quantise(v, 255.0).tolist()[5:9] == [127, 255, 255, 255]
    assert E.quantise(v, 1.0).tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 1, 0] and E.quantise(v, 90.7).max() == 90


# ------------------------------------------------------------------------------------------------ the host function
def test_layout():
    assert ops.ensemble_cols(8, 4) == (7 + 81 + 72, {"rank": 7, "exceed": 88}) and ops.ensemble_cols(16, 8)[0] == 7 + 289 + 272 == E.cols(16, 8)
    assert ops.ensemble_cols(2, 1) == (22, {"rank": 7, "exceed": 16})
    for bad in ((1, 4), (17, 4), (8, 0), (8, 9)):
        with pytest.raises(ValueError):
            ops.ensemble_cols(*bad)


@pytest.mark.parametrize("M", [2, 5, 16])
def test_entries_equal_the_pixel_wise_scores(M):
    t, m = E.radar_stack(M, 4, 21, 19, 7 + M)
    rows = E.frame_rows(t, m, THR, SCALE).sum(axis=0)
    e = V.ensemble_entries(rows, M, THR)
    y, x = E.quantise(t, SCALE).ravel().astype(np.float64), E.quantise(m, SCALE).reshape(M, -1).astype(np.float64)
    n = y.size
    crps = np.abs(x - y).mean(axis=0) - np.abs(x[:, None] - x[None]).sum(axis=(0, 1)) / (2.0 * M * M)
    fair = np.abs(x - y).mean(axis=0) - np.abs(x[:, None] - x[None]).sum(axis=(0, 1)) / (2.0 * M * (M - 1))
    assert (e["members"], e["pixels"], e["dry"]) == (M, n, int(((y == 0) & (x == 0).all(axis=0)).sum()))
    assert abs(e["crps"] - crps.mean()) < 1e-11 and abs(e["crps_fair"] - fair.mean()) < 1e-11 and abs(e["mae_control"] - np.abs(x[0] - y).mean()) < 1e-11
    assert abs(e["crpss"] - (1.0 - crps.mean() / np.abs(x[0] - y).mean())) < 1e-11
    spread, rmse = np.sqrt(x.var(axis=0, ddof=1).mean()), np.sqrt(((x.mean(axis=0) - y) ** 2).mean())
    assert abs(e["spread"] - spread) < 1e-10 and abs(e["rmse_mean"] - rmse) < 1e-10 and abs(e["spread_skill"] - np.sqrt((M + 1) / M) * spread / rmse) < 1e-10
    # the rank histogram pixel by pixel: ties shared equally
    want = np.zeros(M + 1)
    for b, q in zip((x < y).sum(axis=0), (x == y).sum(axis=0)):
        want[b:b + q + 1] += 1.0 / (q + 1)
    assert np.abs(e["rank_histogram"] - want).max() < 1e-8 and abs(e["rank_histogram"].sum() - n) < 1e-8
    assert abs(e["rank_histogram_wet"].sum() - (n - e["dry"])) < 1e-8 and np.abs(e["rank_histogram"] - e["rank_histogram_wet"] - e["dry"] / (M + 1)).max() < 1e-9
    for k, thr in enumerate(THR):
        o, c = (y >= thr), (x >= thr).sum(axis=0)
        p = c / M
        h = e[int(thr)]
        assert h["histogram"].shape == (2, M + 1) and h["histogram"].sum() == n
        assert (h["histogram"][0] == np.bincount(c[~o], minlength=M + 1)).all() and (h["histogram"][1] == np.bincount(c[o], minlength=M + 1)).all()
        assert abs(h["brier"] - ((p - o) ** 2).mean()) < 1e-12 and abs(h["base_rate"] - o.mean()) < 1e-12
        assert abs(h["brier"] - (h["reliability"] - h["resolution"] + h["uncertainty"])) < 1e-12
        assert h["roc"]["pod"].shape == (M + 2,) and h["reliability_diagram"]["count"].sum() == n


def test_members_equal_to_the_target_and_copies_of_one_forecast():
    M = 8
    t, m = E.radar_stack(M, 3, 16, 16, 2, plant=False)
    same = np.broadcast_to(t, (M,) + t.shape)
    e = V.ensemble_entries(E.frame_rows(t, same, THR, SCALE).sum(axis=0), M, THR)
    assert e["crps"] == 0.0 and e["spread"] == 0.0 and e["mae_control"] == 0.0 and e["rmse_mean"] == 0.0 and np.isnan(e["crpss"]) and np.isnan(e["spread_skill"])
    wet = e["pixels"] - e["dry"]
    assert wet > 0 and np.abs(e["rank_histogram_wet"] - wet / (M + 1)).max() < 1e-9, "flat by tie-sharing"
    assert np.abs(e["rank_histogram"] - e["pixels"] / (M + 1)).max() < 1e-9
    for thr in (20, 30, 35, 40):
        assert e[thr]["brier"] == 0.0 and (e[thr]["histogram"][0, 1:] == 0).all() and (e[thr]["histogram"][1, :M] == 0).all()
    copies = np.broadcast_to(m[1], (M,) + t.shape)
    rows = E.frame_rows(t, copies, THR, SCALE).sum(axis=0)
    e = V.ensemble_entries(rows, M, THR)
    assert rows[4] == 0 and rows[5] == 0 and e["crps"] == e["mae_control"] > 0.0 and e["crpss"] == 0.0 and e["spread"] == 0.0
    assert abs(e["rank_histogram"].sum() - e["pixels"]) < 1e-8


def test_the_leading_axis_the_threshold_at_zero_and_the_refusals():
    M = 3
    t, m = E.radar_stack(M, 4, 12, 12, 5)
    thr = [0.0, 35.0]
    tab = E.table(t, m, thr, SCALE, 2)
    lead = V.ensemble_entries(tab, M, thr)
    for tt in range(2):
        one = V.ensemble_entries(tab[tt], M, thr)
        for key in ("crps", "crps_fair", "mae_control", "spread", "rmse_mean", "pixels", "dry"):
            assert lead[key].shape == (2,) and lead[key][tt] == one[key], key
        assert (lead["rank_histogram"][tt] == one["rank_histogram"]).all() and (lead[35]["histogram"][tt] == one[35]["histogram"]).all()
        # every pixel is an event at a threshold of 0: the dry pixels go back to (o = 1, c = M)
        assert one[0]["histogram"][0].sum() == 0 and one[0]["histogram"][1, M] >= one["dry"] and one[0]["histogram"].sum() == one["pixels"]
    empty = V.ensemble_entries(np.zeros(E.cols(M, 2)), M, thr)
    assert np.isnan(empty["crps"]) and np.isnan(empty["spread"]) and np.isnan(empty[35]["brier"])
    with pytest.raises(ValueError, match="rows are"):
        V.ensemble_entries(np.zeros(E.cols(M, 2) + 1), M, thr)
    with pytest.raises(ValueError, match="integer"):
        V.ensemble_entries(np.full(E.cols(M, 2), 0.5), M, thr)
    with pytest.raises(ValueError, match=">= 0"):
        V.ensemble_entries(np.full(E.cols(M, 2), -1), M, thr)
    with pytest.raises(ValueError):
        V.ensemble_entries(np.zeros(E.cols(M, 2)), 1, thr)


def _former_nprob_entry(n0, n1, n, bins=10):
    """validate.nprob_entries' inner function as it stood before the helper was lifted, kept here word for word"""
    from adnm_hip.validate import _scalar, _tail_sums

    def ratio(a, b):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return _scalar(np.where(b == 0, np.nan, a / b))
    c = np.arange(n * n + 1)
    p = c / float(n * n)
    both = (n0 + n1).astype(np.float64)
    total, events, quiet = both.sum(axis=-1), n1.sum(axis=-1), n0.sum(axis=-1)
    base = np.asarray(ratio(events, total))
    freq = np.asarray(ratio(n1, both))
    rel = np.where(both == 0, 0.0, both * (p - freq) ** 2).sum(axis=-1)
    res = np.where(both == 0, 0.0, both * (freq - base[..., None]) ** 2).sum(axis=-1)
    brier, unc = np.asarray(ratio((n0 * p ** 2 + n1 * (p - 1.0) ** 2).sum(axis=-1), total)), base * (1.0 - base)
    zero = np.zeros(n0.shape[:-1] + (1,))
    pod = np.concatenate([np.asarray(ratio(_tail_sums(n1, -1), events[..., None])), zero], axis=-1)
    pofd = np.concatenate([np.asarray(ratio(_tail_sums(n0, -1), quiet[..., None])), zero], axis=-1)
    area = ((pofd[..., :-1] - pofd[..., 1:]) * (pod[..., :-1] + pod[..., 1:]) / 2.0).sum(axis=-1)
    member = (np.minimum(c * bins // (n * n), bins - 1)[:, None] == np.arange(bins)).astype(np.float64)
    count = both @ member
    return {"histogram": np.stack([n0, n1], axis=-2), "base_rate": _scalar(base), "brier": _scalar(brier),
            "reliability": ratio(rel, total), "resolution": ratio(res, total), "uncertainty": _scalar(unc),
            "brier_skill": _scalar(1.0 - np.asarray(ratio(brier, unc))), "roc": {"pofd": pofd, "pod": pod}, "roc_area": _scalar(area),
            "reliability_diagram": {"edges": np.linspace(0.0, 1.0, bins + 1), "count": count.astype(np.int64),
                                    "forecast_mean": ratio((both * p) @ member, count), "observed_frequency": ratio(n1.astype(np.float64) @ member, count)}}


def _bits(tree):
    """a result tree with every float as its bit pattern"""
    if isinstance(tree, dict):
        return {k: _bits(v) for k, v in tree.items()}
    a = np.asarray(tree)
    return (a.dtype.str, a.shape, a.astype(np.float64).view(np.int64).tolist() if a.dtype.kind == "f" else a.tolist())


def test_the_shared_helper_leaves_nprob_entries_bit_for_bit():
    scales = (1, 3, 9)
    cases = [N.sparse_fields(3, 37, 45, 2), N.noise_fields(2, 37, 45, 4, 0.41), N.noise_fields(2, 37, 45, 5, 0.1)]
    tables = [N.frame_hist(t, p, THR, SCALE, scales).sum(axis=0) for t, p in cases]
    t, p = N.sparse_fields(4, 20, 24, 7)
    tables += [N.table(t, p, THR, SCALE, scales, 2), np.zeros_like(tables[0])]
    for rows in tables:
        got = V.nprob_entries(rows, scales, THR)
        for n, (a0, a1) in zip(scales, ops.nprob_layout(scales)[0]):
            for k, thr in enumerate(THR):
                want = _former_nprob_entry(rows[..., k, a0:a0 + n * n + 1], rows[..., k, a1:a1 + n * n + 1], n)
                assert _bits(got[n][int(thr)]) == _bits(want), (n, thr)


# ------------------------------------------------------------------------------------------------ the parts table
def test_the_row_stands_directly_in_front_of_the_tracks_and_nothing_else_moves():
    T, n = 5, 3
    params = list(inspect.signature(V.block_rows).parameters)
    assert params[:8] == ["T", "nthr", "pools", "persistence", "fss", "advection", "spectrum", "joint"] and inspect.signature(V.block_rows).parameters["ensemble"].default is None
    assert list(inspect.signature(V.block_tables).parameters) == [p for p in params if p != "ensemble"], "block_tables keeps the parameter list it had"
    sal = ops.sal_spec(True)
    full = dict(pools=((4, 4),), persistence=True, fss=(1, 5), advection=True, spectrum=(16, 32), joint=7, objects=2, sal=sal, nprob=(1, 5), iscale=(16, 32))
    for kw in (dict(), dict(persistence=True, iscale=(8, 8)), dict(tracks=2), dict(tracks=1, **full)):
        base, size = V.block_tables(T, n, **kw)
        assert V.block_rows(T, n, **kw) == (base, size) == V.block_rows(T, n, ensemble=None, **kw), "the default changed a configuration"
        parts, total = V.block_rows(T, n, ensemble=8, **kw)
        C = ops.ensemble_cols(8, n)[0]
        assert total == size + T * C
        at = len(parts) - 2 if kw.get("tracks") else len(parts) - 1
        assert parts[at].name == "ensemble" and parts[at].kind == "ensemble" and parts[at].field == "pred" and parts[at].shape == (T, C)
        assert parts[:at] == base[:at], "a part in front of it moved"
        if kw.get("tracks"):
            assert parts[-1].name == "tracks" and parts[-1].offset == base[-1].offset + T * C and parts[-1].shape == base[-1].shape
    assert V.ensemble_doubles(20, 4) == 0 and V.ensemble_doubles(20, 4, 8) == 20 * 160 and V.ensemble_doubles(3, 8, 16) == 3 * 568


def test_aggregate_reads_the_table_and_the_former_result_stays():
    T, n, M = 3, 2, 4
    t, m = E.radar_stack(M, 2 * T, 24, 24, 9)
    tab = E.table(t, m, THR[:n], SCALE, T).astype(np.float64)
    rng = np.random.default_rng(1)
    main = rng.integers(1, 1 << 20, (T, 4 * n + 3)).astype(np.float64)
    head = np.concatenate([[1.25, 2, 2, 0], main.ravel()])
    plain = V.aggregate(head, THR[:n], T, 576, None, per_lead=True)
    res = V.aggregate(np.concatenate([head, tab.ravel()]), THR[:n], T, 576, None, per_lead=True, ensemble=M)
    assert list(res) == [k for k in plain if k != "per_lead"] + ["ensemble", "per_lead"] and list(res["per_lead"]) == list(plain["per_lead"]) + ["ensemble"]
    assert repr({k: res[k] for k in plain if k != "per_lead"}) == repr({k: plain[k] for k in plain if k != "per_lead"})
    assert repr(res["ensemble"]) == repr(V.ensemble_entries(tab.sum(axis=0), M, THR[:n])) and repr(res["per_lead"]["ensemble"]) == repr(V.ensemble_entries(tab, M, THR[:n]))
    assert res["ensemble"]["pixels"] == 2 * T * 576
    with pytest.raises(ValueError, match="doubles"):
        V.aggregate(np.concatenate([head, tab.ravel()]), THR[:n], T, 576, None)
    with pytest.raises(ValueError, match="ensemble"):
        V.aggregate(np.concatenate([head, tab.ravel()]), THR[:n], T, 576, None, ensemble=8)


# ------------------------------------------------------------------------------------------------ the member recipe
def test_ensemble_spec():
    spec = ops.ensemble_spec
    assert spec(None, True) is None and spec(False, False) is None
    assert spec(True, True) == (0, 1, 2, 3, 4, 5, 6, 7) and spec(True, False) == (0, 1, 2, 3) and spec(True, None) is True
    assert spec((0, 3), False) == (0, 3) and spec([0, 5, 6], True) == (0, 5, 6) and spec(dict(members=(0, 1)), True) == (0, 1)
    assert spec(np.array([0, 7]), True) == (0, 7) and spec((0, 4), None) == (0, 4)
    for bad in ((0,), (1, 0), (0, 0), (0, 1, 1), (0, 8), (0, -1), (0, 1.0), (0, True), "01", 5, dict(codes=(0, 1)), dict(members=(0, 1), thresholds=(1,)),
                tuple(range(8)) + (0,)):
        with pytest.raises(ValueError):
            spec(bad, True)
    for bad in ((0, 4), (0, 1, 5), (0, 6), (0, 7)):
        with pytest.raises(ValueError, match="square"):
            spec(bad, False)


@pytest.mark.parametrize("shape", [(5, 5), (4, 7), (1, 1)])
def test_the_codes_compose_to_the_identity_with_their_stated_inverses(shape):
    """on a CPU restatement of the kernel's index map (csrc/ensemble.hip: d4_source) and on the torch yardstick"""
    H, W = shape

    def source(code, inverse, y, x):
        lr, ud, tr = code & 1, code & 2, code & 4
        if not inverse:
            a, b = (x, y) if tr else (y, x)
            return (H - 1 - a if ud else a), (W - 1 - b if lr else b)
        fy, fx = (H - 1 - y if ud else y), (W - 1 - x if lr else x)
        return (fx, fy) if tr else (fy, fx)

    def apply(w, code, inverse):
        out = np.empty_like(w)
        for y in range(H):
            for x in range(W):
                out[y, x] = w[source(code, inverse, y, x)]
        return out
    w = np.arange(H * W, dtype=np.float32).reshape(H, W)
    for code in range(8 if H == W else 4):
        fwd = apply(w, code, False)
        assert (fwd == E.g(torch.from_numpy(w), code).numpy()).all() and (apply(w, code, True) == E.g_inv(torch.from_numpy(w), code).numpy()).all(), code
        assert (apply(fwd, code, True) == w).all() and (apply(apply(w, code, True), code, False) == w).all(), code
        twin = {5: 6, 6: 5}.get(code, code)     # the two quarter turns are each other's inverse, every other element its own
        assert (apply(w, code, True) == apply(w, twin, False)).all(), code


# ------------------------------------------------------------------------------------------------ the C boundary
def test_new_prototypes_are_declared_and_exported_and_the_abi_version_stays():
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/adnm_hip.h"
        assert hasattr(so, name), f"{name} declared but not exported"
    assert protos["adnm_d4_members"] == ("int", ["const float*", "float*", "const int*", "int64_t", "int", "int64_t", "int64_t", "int64_t", "adnm_stream_t"])
    assert protos["adnm_valid_ens_accum"] == ("int", ["const float*", "int64_t", "int64_t", "int64_t", "const float*", "void*", "const float*", "int64_t", "float",
                                                       "int64_t", "void*", "int64_t", "int64_t", "int64_t", "int64_t", "adnm_stream_t"])
    assert protos["adnm_ensemble_product"] == ("int", ["const float*", "int64_t", "int64_t", "int64_t", "float*", "float*", "const float*", "int64_t", "float",
                                                        "int64_t", "int64_t", "int64_t", "int64_t", "adnm_stream_t"])
    assert lib.load().adnm_abi_version() == 11


def test_byte_queries():
    q = lib.query
    assert q("adnm_valid_ens_block_bytes", 20, 4, 8) == 8 * 20 * 160 and q("adnm_valid_ens_block_bytes", 1, 8, 16) == 8 * 568
    assert q("adnm_valid_ens_block_bytes", 65535, 1, 2) == 8 * 65535 * 22
    for bad in ((0, 4, 8), (65536, 4, 8), (20, 0, 8), (20, 9, 8), (20, 4, 1), (20, 4, 17), (20, 4, 0)):
        assert q("adnm_valid_ens_block_bytes", *bad) == -1, bad
    ws = "adnm_valid_ens_accum_ws_bytes"
    assert q(ws, 80, 20, 128 * 128, 4, 8, 90.0) == 0 and q(ws, 1, 1, 1, 1, 2, 1.0) == 0 and q(ws, 65535, 1, (1 << 24) - 1, 8, 16, 255.99) == 0, "no workspace"
    for bad in ((80, 7, 16384, 4, 8, 90.0), (80, 0, 16384, 4, 8, 90.0), (0, 1, 16384, 4, 8, 90.0), (65540, 20, 16384, 4, 8, 90.0), (80, 20, 0, 4, 8, 90.0),
                (80, 20, 1 << 24, 4, 8, 90.0), (80, 20, 16384, 0, 8, 90.0), (80, 20, 16384, 9, 8, 90.0), (80, 20, 16384, 4, 1, 90.0), (80, 20, 16384, 4, 17, 90.0),
                (80, 20, 16384, 4, 8, 0.99), (80, 20, 16384, 4, 8, 256.0), (80, 20, 16384, 4, 8, float("nan")), (80, 20, 16384, 4, 8, float("inf")),
                (80, 20, 16384, 4, 8, -3.0)):
        assert q(ws, *bad) == -1, bad


def test_every_limit_is_refused_on_the_host_with_its_own_message():
    """fake addresses: anything that reached a launch would fault, and the stream is never touched"""
    so = lib.load()
    thr, hw = (ctypes.c_float * 4)(20, 30, 35, 40), 64 * 64

    def accum(mem=16, ms=40 * hw, ss=20 * hw, fs=hw, tgt=32, table=64, thr_=thr, nthr=4, scale=90.0, M=8, frames=40, T=20, hw_=hw):
        rc = so.adnm_valid_ens_accum(mem, ms, ss, fs, tgt, table, thr_, nthr, scale, M, None, 0, frames, T, hw_, None)
        return rc, lib.last_error()
    cases = [(dict(mem=None), "null pointer"), (dict(tgt=None), "null pointer"), (dict(table=None), "null pointer"), (dict(thr_=None), "null pointer"),
             (dict(mem=18), "4-byte aligned"), (dict(tgt=34), "4-byte aligned"), (dict(table=68), "8-byte aligned"),
             (dict(nthr=0), "1..8 thresholds"), (dict(nthr=9), "1..8 thresholds"), (dict(M=1), "2 <= M <= 16"), (dict(M=17), "2 <= M <= 16"),
             (dict(T=0), "must divide frames"), (dict(T=7), "must divide frames"), (dict(frames=65540, T=20), "frames <= 65535"),
             (dict(hw_=0), "hw < 2^24"), (dict(hw_=1 << 24), "hw < 2^24"),
             (dict(scale=0.5), "value_scale"), (dict(scale=256.0), "value_scale"), (dict(scale=float("nan")), "value_scale"), (dict(scale=float("inf")), "value_scale"),
             (dict(fs=hw - 1), "frame_stride"), (dict(fs=-hw), "frame_stride"), (dict(ss=20 * hw - 1), "sample_stride"), (dict(ss=-1), "sample_stride"),
             (dict(ms=40 * hw - 1), "member_stride"), (dict(ms=-4), "member_stride")]
    for kw, text in cases:
        rc, err = accum(**kw)
        assert rc == -1 and text in err and "valid_ens_accum" in err, (kw, rc, err)
    assert len({text for _, text in cases}) == 12, "one message per limit"

    def d4(src=16, dst=32, codes=(0, 1, 4), M=3, inverse=0, planes=10, H=32, W=32):
        arr = None if codes is None else (ctypes.c_int * len(codes))(*codes)
        rc = so.adnm_d4_members(src, dst, arr, M, inverse, planes, H, W, None)
        return rc, lib.last_error()
    for kw, text in [(dict(src=None), "null pointer"), (dict(dst=None), "null pointer"), (dict(codes=None), "null pointer"), (dict(src=18), "4-byte aligned"),
                     (dict(dst=34), "4-byte aligned"), (dict(M=0), "1 <= M <= 16"), (dict(M=17, codes=(0,) * 17), "1 <= M <= 16"),
                     (dict(codes=(0, 8, 1)), "0..7"), (dict(codes=(0, -1, 1)), "0..7"), (dict(H=32, W=33), "square"), (dict(H=31, W=32, inverse=1), "square"),
                     (dict(planes=0), "planes"), (dict(planes=65536), "planes"), (dict(H=0), "[1, 32768)"), (dict(W=32768, H=1, codes=(0, 1, 2)), "[1, 32768)"),
                     (dict(H=4096, W=4096), "2^24")]:
        rc, err = d4(**kw)
        assert rc == -1 and text in err and "d4_members" in err, (kw, rc, err)

    def product(mem=16, ms=40 * hw, ss=20 * hw, fs=hw, mean=32, prob=64, thr_=thr, K=4, M=8, frames=40, T=20, hw_=hw):
        rc = so.adnm_ensemble_product(mem, ms, ss, fs, mean, prob, thr_, K, 90.0, M, frames, T, hw_, None)
        return rc, lib.last_error()
    for kw, text in [(dict(mem=None), "null pointer"), (dict(mean=None), "null pointer"), (dict(prob=None), "null pointer"), (dict(thr_=None), "null pointer"),
                     (dict(mem=18), "4-byte aligned"), (dict(mean=34), "4-byte aligned"), (dict(prob=66), "4-byte aligned"), (dict(K=-1), "0..8 thresholds"),
                     (dict(K=9), "0..8 thresholds"), (dict(M=1), "2 <= M <= 16"), (dict(M=17), "2 <= M <= 16"), (dict(T=7), "must divide frames"),
                     (dict(frames=65540, T=20), "frames <= 65535"), (dict(hw_=1 << 24), "hw < 2^24"), (dict(fs=hw - 1), "frame_stride"),
                     (dict(ss=3), "sample_stride"), (dict(ms=5), "member_stride")]:
        rc, err = product(**kw)
        assert rc == -1 and text in err and "ensemble_product" in err, (kw, rc, err)


# ------------------------------------------------------------------------------------------------ the arguments
def test_validator_and_forecaster_arguments():
    from adnm_hip.forecast import Forecast, Forecaster, Palette
    from adnm_hip.validate import Validator
    from models.loss import enRainfallLoss
    assert inspect.signature(Validator.__init__).parameters["ensemble"].default is None
    model, crit = torch.nn.Identity(), enRainfallLoss()
    kinds = lambda v: [p.kind for p in v._parts]
    val = Validator(model, crit, 20, 90.0)
    assert val.ensemble is None and kinds(val) == ["main"]
    val = Validator(model, crit, 20, 90.0, ensemble=(0, 1, 2, 3), tracks=True, nprob=(3,))
    assert val.ensemble == (0, 1, 2, 3) and kinds(val) == ["main", "nprob", "ensemble", "tracks"] and val._parts[-2].shape == (20, ops.ensemble_cols(4, 4)[0])
    assert Validator(model, crit, 20, 90.0, ensemble=dict(members=(0, 7))).ensemble == (0, 7)
    val = Validator(model, crit, 20, 90.0, ensemble=True)
    assert val.ensemble is True and kinds(val) == ["main"], "the table comes with the block: the frames say how many members there are"
    assert val._codes((32, 32)) == tuple(range(8)) and val._codes((32, 48)) == (0, 1, 2, 3) and val._codes(None) is None
    with pytest.raises(ValueError, match="square"):
        Validator(model, crit, 20, 90.0, ensemble=(0, 4))._codes((32, 48))
    for bad in ((1, 0), (0, 0), (0, 9), "01", dict(codes=(0, 1))):
        with pytest.raises(ValueError):
            Validator(model, crit, 20, 90.0, ensemble=bad)
    with pytest.raises(ValueError, match="value_scale"):
        Validator(model, crit, 20, 300.0, ensemble=True)
    pal = Palette([0.0, 0.5, 1.0], np.array([[0, 0, 0, 255], [255, 0, 0, 255]], dtype=np.uint8))
    assert Forecaster(model, pal).ensemble is None and inspect.signature(Forecaster.__init__).parameters["ensemble"].default is None
    fc = Forecaster(model, pal, pixel_scale=90.0, ensemble=dict(members=True, thresholds=(35, 40)))
    assert fc.ensemble[0] is True and list(fc.ensemble[1]) == [35.0, 40.0] and fc.ensemble[2] == 2
    assert Forecaster(model, pal, pixel_scale=None, ensemble=dict(members=(0, 1))).ensemble[2] == 0
    with pytest.raises(ValueError, match="pixel_scale"):
        Forecaster(model, pal, pixel_scale=None, ensemble=dict(members=True, thresholds=(35,)))
    for bad in (True, (0, 1), dict(thresholds=(35,)), dict(members=None), dict(members=(1, 0)), dict(members=True, thresholds=range(9)), dict(members=True, scale=3)):
        with pytest.raises(ValueError):
            Forecaster(model, pal, ensemble=bad)
    res = Forecast(1, 2, 3)
    assert res.members is None and res.ens_mean is None and res.ens_prob is None and Forecast(1, 2, 3, 4, 5, 6, 7).ens_prob == 7
