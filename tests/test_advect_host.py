"""The advection baseline without a GPU: the CPU yardstick checks itself (a plain quadruple loop, a planted shift, the density of the
listed cases), the three entry points at the C boundary (declared, exported, additive, refusing every limit before any launch),
ops.advection_spec, validate.aggregate on a hand-made block with the two appended tables, and the Validator's arguments."""
import ctypes

import numpy as np
import pytest

import advect_ref as A
from adnm_hip import lib

NEW = ("adnm_trec_ws_bytes", "adnm_trec_motion", "adnm_advect")


# ------------------------------------------------------------------------------------------------ the helper
@pytest.mark.parametrize("shape,block,radius", [((2, 9, 11), 8, 2), ((1, 5, 40), 16, 3), ((1, 5, 40), 32, 8)])
def test_sliced_costs_equal_a_plain_quadruple_loop(shape, block, radius):
    prev, last = A.two_motion_fields(*shape, 0)
    last[0, 0, 0], prev[0, -1, -1], last[0, 2, 3], prev[0, 1, 1] = 1.5, 0.9, float("nan"), float("-inf")
    a, b = A.costs(prev, last, A.SCALE, block, radius), A.loop_costs(prev, last, A.SCALE, block, radius)
    D = 2 * radius + 1
    assert a.shape == b.shape == (shape[0], -(-shape[1] // block), -(-shape[2] // block), D, D) and (a == b).all()
    assert (a > 0).any() and len(np.unique(a)) > 4, "nothing is compared"
    # the advection by a plain loop
    m = A.motion(prev, last, A.SCALE, block, radius, 1)
    adv = A.advect(last, m, block, 3).view(np.int32)
    bits = last.view(np.int32)
    n, H, W = last.shape
    for s in range(n):
        for t in range(3):
            for y in range(H):
                for x in range(W):
                    vy, vx = m[s, y // block, x // block]
                    sy, sx = y - (t + 1) * vy, x - (t + 1) * vx
                    want = bits[s, sy, sx] if 0 <= sy < H and 0 <= sx < W else 0
                    assert adv[s, t, y, x] == want, (s, t, y, x)


def test_pick_order():
    """(cost, dy^2 + dx^2, dy, dx) lexicographically: an all-zero table gives (0, 0); among equal costs the shorter vector, then the smaller dy, then dx"""
    assert tuple(A.pick(np.zeros((5, 5), dtype=np.int64), 2)) == (0, 0)
    t = np.full((5, 5), 9, dtype=np.int64)
    t[2 + 1, 2 + 0] = t[2 + 0, 2 - 1] = t[2 - 1, 2 + 0] = t[2 + 0, 2 + 1] = 3          # four vectors of length 1
    assert tuple(A.pick(t, 2)) == (-1, 0)
    t[2 - 1, 2 + 0] = 9
    assert tuple(A.pick(t, 2)) == (0, -1)
    t[2 + 2, 2 + 2] = 2                                                                # a smaller cost beats a shorter vector
    assert tuple(A.pick(t, 2)) == (2, 2)
    big = np.full((17, 17), 32 * 32 * 255, dtype=np.int64)
    big[0, 16] = big[16, 0] = 32 * 32 * 255 - 1
    assert tuple(A.pick(big, 8)) == (-8, 8)


def test_a_planted_shift_is_recovered():
    """prev rolled by (2, -3): last(y, x) = prev(y - 2, x + 3), so v = (2, -3) for the frame and for every valid block whose window holds
    the whole blob (the blob lies well inside the frame, so the roll wraps nothing but zeros)"""
    H = W = 64
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    prev = (0.6 * np.exp(-((yy - 30) ** 2 + (xx - 34) ** 2) / (2 * 5.0 ** 2)))[None]
    prev[prev < 0.02] = 0.0
    ys, xs = np.nonzero(prev[0])
    assert ys.min() >= 12 and ys.max() < H - 12 and xs.min() >= 12 and xs.max() < W - 12
    last = np.roll(prev, (2, -3), axis=(1, 2))
    prev, last = prev.astype(np.float32), last.astype(np.float32)
    for block, radius in ((8, 3), (16, 4), (32, 8)):
        m, c, valid, g = A.motion(prev, last, A.SCALE, block, radius, A.ECHO, with_parts=True)
        assert tuple(g[0]) == (2, -3), (block, radius, g)
        assert valid.sum() >= 1 and (m[0][valid[0]] == (2, -3)).all(), (block, radius)
        assert (m[0][~valid[0]] == (2, -3)).all(), "an invalid block takes the global vector"
        assert c[0, :, :, radius + 2, radius - 3].sum() == 0
    adv = A.advect(last, A.motion(prev, last, A.SCALE, 16, 4, A.ECHO), 16, 2)
    assert (adv[0, 0] == np.roll(last[0], (2, -3), axis=(0, 1))).all() and (adv[0, 1] == np.roll(last[0], (4, -6), axis=(0, 1))).all()


@pytest.mark.parametrize("block,radius", A.CONFIGS)
def test_the_listed_cases_are_dense(block, radius):
    tied, invalid = A.assert_dense(A.CASES, block, radius)
    print("tied blocks", tied, "invalid blocks", invalid)
    still = np.zeros((1, 16, 16), dtype=np.float32)
    with pytest.raises(AssertionError, match="do not weaken this$"):
        A.assert_dense(["two empty frames"], block, radius, fields=lambda case: (still, still))


# ------------------------------------------------------------------------------------------------ the C boundary
def test_new_prototypes_are_declared_and_exported_and_the_abi_version_stays():
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW:
        assert name in protos, f"{name} is not declared in include/adnm_hip.h"
        assert hasattr(so, name), f"{name} declared but not exported"
    assert protos["adnm_trec_ws_bytes"] == ("int64_t", ["int64_t"] * 5)
    assert protos["adnm_trec_motion"][0] == "int" and protos["adnm_trec_motion"][1][-1] == "adnm_stream_t" and len(protos["adnm_trec_motion"][1]) == 15
    assert protos["adnm_advect"][0] == "int" and protos["adnm_advect"][1][-1] == "adnm_stream_t" and len(protos["adnm_advect"][1]) == 10
    assert lib.load().adnm_abi_version() == 11


def test_byte_query():
    q = lambda *a: lib.query("adnm_trec_ws_bytes", *a)   # noqa: E731
    # per sample and block (2R+1)^2 costs and one echo count, uint32
    assert q(4, 128, 128, 32, 4) == 4 * 16 * 82 * 4
    assert q(3, 37, 53, 8, 2) == 3 * 5 * 7 * 26 * 4
    assert q(2, 5, 40, 32, 8) == 2 * 1 * 2 * 290 * 4
    assert q(1, 1, 1, 16, 1) == 10 * 4
    assert q(65535, 16, 16, 16, 1) == 65535 * 40
    for bad in ((0, 64, 64, 16, 4), (65536, 64, 64, 16, 4), (2, 0, 64, 16, 4), (2, 64, 0, 16, 4), (2, 32768, 16, 16, 4), (2, 16, 32768, 16, 4),
                (2, 4096, 4096, 16, 4), (2, 64, 64, 4, 4), (2, 64, 64, 12, 4), (2, 64, 64, 64, 4), (2, 64, 64, 0, 4), (2, 64, 64, 16, 0),
                (2, 64, 64, 16, 9), (2, 64, 64, 16, -1)):
        assert q(*bad) == -1, bad


def test_every_limit_is_refused_on_the_host_with_its_own_message():
    """fake addresses: anything that reached a launch would fault, and the stream is never touched"""
    so = lib.load()

    def motion(prev=16, last=32, ss=64 * 64, mot=64, cost=None, scale=90.0, block=16, radius=4, echo=20, ws=128, ws_bytes=1 << 30, samples=2, H=64, W=64):
        rc = so.adnm_trec_motion(prev, last, ss, mot, cost, scale, block, radius, echo, ws, ws_bytes, samples, H, W, None)
        return rc, lib.last_error()

    def advect(last=32, ss=64 * 64, mot=64, out=96, block=16, samples=2, T=5, H=64, W=64):
        rc = so.adnm_advect(last, ss, mot, out, block, samples, T, H, W, None)
        return rc, lib.last_error()

    cases = [(dict(prev=None), "null pointer"), (dict(last=None), "null pointer"), (dict(mot=None), "null pointer"),
             (dict(prev=18), "prev and last must be 4-byte aligned"), (dict(last=34), "prev and last must be 4-byte aligned"),
             (dict(mot=66), "motion and cost_out must be 4-byte aligned"), (dict(cost=130), "motion and cost_out must be 4-byte aligned"),
             (dict(block=4), "8, 16 or 32"), (dict(block=24), "8, 16 or 32"), (dict(block=64), "8, 16 or 32"),
             (dict(radius=0), "radius"), (dict(radius=9), "radius"),
             (dict(echo=0), "echo"), (dict(echo=256), "echo"),
             (dict(scale=0.0), "value_scale"), (dict(scale=-1.0), "value_scale"), (dict(scale=255.5), "value_scale"), (dict(scale=float("nan")), "value_scale"),
             (dict(samples=0), "1..65535"), (dict(samples=65536), "1..65535"),
             (dict(H=0), "[1, 32768)"), (dict(W=32768, H=16, ss=1 << 20), "[1, 32768)"), (dict(H=32768, W=16, ss=1 << 20), "[1, 32768)"),
             (dict(H=4096, W=4096, ss=1 << 24), "2^24"),
             (dict(ss=64 * 64 - 1), "sample_stride"), (dict(ss=0), "sample_stride")]
    for kw, text in cases:
        rc, err = motion(**kw)
        assert rc == -1 and text in err and "trec_motion" in err, (kw, rc, err)
    assert len({text for _, text in cases}) == 11, "one message per limit"
    assert motion(scale=255.0, ws_bytes=8)[0] == -3 and "workspace" in lib.last_error()
    assert motion(ws=None)[0] == -3 and "workspace" in lib.last_error()
    assert motion(ws_bytes=lib.query("adnm_trec_ws_bytes", 2, 64, 64, 16, 4) - 1)[0] == -3

    cases = [(dict(last=None), "null pointer"), (dict(mot=None), "null pointer"), (dict(out=None), "null pointer"),
             (dict(last=34), "last and out must be 4-byte aligned"), (dict(out=98), "last and out must be 4-byte aligned"), (dict(mot=66), "motion must be 4-byte aligned"),
             (dict(block=4), "8, 16 or 32"), (dict(block=33), "8, 16 or 32"),
             (dict(samples=0), "1..65535"), (dict(samples=65536), "1..65535"),
             (dict(T=0), "T must be >= 1"), (dict(T=-3), "T must be >= 1"),
             (dict(H=0), "[1, 32768)"), (dict(W=32768, H=16, ss=1 << 20), "[1, 32768)"), (dict(H=4096, W=4096, ss=1 << 24), "2^24"),
             (dict(ss=64 * 64 - 1), "sample_stride")]
    for kw, text in cases:
        rc, err = advect(**kw)
        assert rc == -1 and text in err and "advect" in err, (kw, rc, err)


# ------------------------------------------------------------------------------------------------ the arguments
def test_advection_spec():
    from adnm_hip import ops
    thr = [20.0, 30.0, 35.0, 40.0]
    assert ops.advection_spec(None, thr) is None and ops.advection_spec(False, thr) is None
    assert ops.advection_spec(True, thr) == (32, 4, 10)
    assert ops.advection_spec(True, [1.0]) == (32, 4, 1) and ops.advection_spec(True, [0.5, 7]) == (32, 4, 1) and ops.advection_spec(True, [35, 9]) == (32, 4, 4)
    assert ops.advection_spec((16, 4), thr) == (16, 4, 10) and ops.advection_spec([8, 1, 255], thr) == (8, 1, 255)
    assert ops.advection_spec((np.int64(32), np.int32(8), np.int64(3)), thr) == (32, 8, 3)
    assert all(type(v) is int for v in ops.advection_spec(np.array([16, 2]), thr))
    for bad in ((12, 4), (64, 4), (16, 0), (16, 9), (16, 4, 0), (16, 4, 256), (16,), (16, 4, 20, 1), (), (16.0, 4), (16, 4.0), ("16", 4), "16", 16, 4.0,
                (True, 4), (16, True), ((16, 4),)):
        with pytest.raises(ValueError, match="advection"):
            ops.advection_spec(bad, thr)


def test_validator_arguments():
    import inspect

    import torch
    from adnm_hip.validate import Validator
    from models.loss import enRainfallLoss
    assert inspect.signature(Validator.__init__).parameters["advection"].default is None
    model, crit = torch.nn.Identity(), enRainfallLoss()
    val = Validator(model, crit, 20, 255.0)
    pool = lambda v: [(p.field, p.pools) for p in v._parts if p.kind == "pool"]   # the pooled and the FSS passes, in the order of their tables and launches
    fss = lambda v: [p.field for p in v._parts if p.kind == "fss"]
    assert val.advection is None and pool(val) == [] and fss(val) == []
    val = Validator(model, crit, 20, 255.0, advection=True)
    assert val.advection == (32, 4, 10) and pool(val) == [("adv", ((1, 1),))] and fss(val) == []
    val = Validator(model, crit, 20, 90.0, [30, 40], advection=(16, 4), persistence=True, pools=(4,), fss=9)
    assert val.advection == (16, 4, 15) and fss(val) == ["pred", "last", "adv"] and pool(val) == [("pred", ((4, 4),)), ("last", ((1, 1), (4, 4))), ("adv", ((1, 1), (4, 4)))]
    for bad in ((12, 4), (16, 9), (16, 4, 0), "yes", 3):
        with pytest.raises(ValueError, match="advection"):
            Validator(model, crit, 20, 255.0, advection=bad)
    with pytest.raises(ValueError, match="value_scale <= 255"):
        Validator(model, crit, 20, 256.0, advection=True)
    Validator(model, crit, 20, 256.0)                                               # only the advection needs bytes
    with pytest.raises(ValueError, match="advection baseline"):
        Validator(model, crit, 20, 255.0, advection=True, pools=(2, 4, 8, 16))       # (1, 1) would be the fifth pool
    Validator(model, crit, 20, 255.0, advection=True, pools=(1, 2, 4, 8))
    with pytest.raises(RuntimeError, match="advected"):
        Validator(model, crit, 20, 255.0).advected(torch.zeros(1, 5, 1, 8, 8))


# ------------------------------------------------------------------------------------------------ aggregate
T, THR, POOLS, FSS = 5, [20, 30, 35, 40], ((4, 4), (16, 8)), (1, 5, 33)


def _hand_block(seed, pools=POOLS, persistence=True, fss=FSS):
    """an integer block: what there is without the advection, then the two appended tables.  -> (block, former doubles, pooled, fss table)"""
    from adnm_hip.validate import advection_doubles, block_doubles, fss_doubles
    rng = np.random.default_rng(seed)
    n = len(THR)
    former = sum(block_doubles(T, n, pools, persistence)) + sum(fss_doubles(T, n, fss, persistence))
    n5, n6 = advection_doubles(T, n, pools, fss, True)
    head = rng.integers(1, 1 << 20, former).astype(np.float64)
    head[:4] = [1.25, 2, 6, 0]
    head[4:4 + T * (4 * n + 3)].reshape(T, -1)[:, 4 * n:] += rng.random((T, 3))
    tabs = rng.integers(1, 1 << 20, (n6 // 3, 3)).astype(np.float64)
    tabs[:, 2] = np.floor(np.sqrt(tabs[:, 0] * tabs[:, 1]) * rng.random(len(tabs)))
    blk = np.concatenate([head, rng.integers(1, 1 << 20, n5).astype(np.float64), tabs.ravel()])
    return blk, former, blk[former:former + n5].reshape(T, -1, 4 * n), blk[former + n5:].reshape(T, len(fss), 3 * n)


def _same(a, b):
    return repr(a) == repr(b)


def _csi(tp, fn, fp):
    return float(tp / (tp + fn + fp))


def test_aggregate_with_the_two_appended_tables():
    from adnm_hip.evaluator import contingency_metrics
    from adnm_hip.validate import advection_doubles, aggregate, baseline_pools
    hw, area, n = 48 * 48, 38 * 38, len(THR)
    assert advection_doubles(T, n) == (0, 0) and advection_doubles(T, n, POOLS, FSS, False) == (0, 0)
    assert advection_doubles(T, n, POOLS, FSS, True) == (T * 3 * 16, T * 3 * 12) and advection_doubles(T, n, (), (), True) == (T * 16, 0)
    blk, former, atab, ftab = _hand_block(4)
    res = aggregate(blk, THR, T, hw, area, pools=POOLS, persistence=True, per_lead=True, fss=FSS, advection=True)
    old = aggregate(blk[:former], THR, T, hw, area, pools=POOLS, persistence=True, per_lead=True, fss=FSS)
    # everything in front of the new tables is unchanged, key for key
    assert set(res) == set(old) | {"advection"} and set(res["per_lead"]) == set(old["per_lead"]) | {"advection"}
    assert _same({k: res[k] for k in old if k != "per_lead"}, {k: old[k] for k in old if k != "per_lead"})
    assert _same({k: res["per_lead"][k] for k in old["per_lead"]}, old["per_lead"])
    adv, lead = res["advection"], res["per_lead"]["advection"]
    assert set(adv) == set(res["persistence"]) == {"threshold_metrics", "FAR", "pooled", "fss"}
    assert set(lead) == set(res["per_lead"]["persistence"]) == {"threshold_metrics", "pooled", "fss"}
    assert list(adv["pooled"]) == list(POOLS) == list(lead["pooled"]) and list(adv["fss"]) == list(FSS) == list(lead["fss"])
    base = baseline_pools(POOLS)
    for i, p in enumerate(base):
        got = adv if p == (1, 1) else adv["pooled"][p]
        got_lead = lead if p == (1, 1) else lead["pooled"][p]
        want, far = contingency_metrics(atab[:, i].sum(axis=0), THR)
        assert _same(got["threshold_metrics"], want) and _same(got["FAR"], float(np.mean(far)))
        for k, thr in enumerate(THR):
            tp, fn, fp, tn = atab[:, i, 4 * k:4 * k + 4].T
            assert got["threshold_metrics"][thr]["TP"] == tp.sum() and got["threshold_metrics"][thr]["CSI"] == _csi(tp.sum(), fn.sum(), fp.sum())
            rows = got_lead["threshold_metrics"][thr]
            assert rows["CSI"].shape == (T,) and (rows["TP"] == tp).all() and (rows["TN"] == tn).all()
            assert all(rows["CSI"][t] == _csi(tp[t], fn[t], fp[t]) for t in range(T))
    for i, s in enumerate(FSS):
        for k, thr in enumerate(THR):
            a, f, c = (ftab[:, i, 3 * k + j] for j in range(3))
            assert adv["fss"][s][thr] == 2.0 * c.sum() / (a.sum() + f.sum())
            assert all(lead["fss"][s][thr][t] == 2.0 * c[t] / (a[t] + f[t]) for t in range(T))
    assert not _same(adv["threshold_metrics"], res["persistence"]["threshold_metrics"])
    short = aggregate(blk, THR, T, hw, area, pools=POOLS, persistence=True, fss=FSS, advection=True)
    assert "per_lead" not in short and _same(short["advection"], adv)


def test_aggregate_with_advection_alone_and_refusals():
    from adnm_hip.validate import aggregate
    hw, n = 48 * 48, len(THR)
    blk, former, atab, ftab = _hand_block(5, pools=(), persistence=False, fss=())
    assert former == 4 + T * (4 * n + 3) and atab.shape == (T, 1, 4 * n) and ftab.size == 0
    res = aggregate(blk, THR, T, hw, None, advection=True, per_lead=True)
    old = aggregate(blk[:former], THR, T, hw, None, per_lead=True)
    assert set(res) == set(old) | {"advection"} and set(res["advection"]) == {"threshold_metrics", "FAR", "pooled"} and res["advection"]["pooled"] == {}
    assert "persistence" not in res and _same({k: res[k] for k in old if k != "per_lead"}, {k: old[k] for k in old if k != "per_lead"})
    assert res["advection"]["threshold_metrics"][30]["FN"] == atab[:, 0, 5].sum()
    with pytest.raises(ValueError, match="doubles"):
        aggregate(blk, THR, T, hw, None)                                  # the tables are there, the argument is not
    with pytest.raises(ValueError, match="advection"):
        aggregate(blk[:former], THR, T, hw, None, advection=True)
    blk, former, _, _ = _hand_block(6)
    with pytest.raises(ValueError, match="doubles"):
        aggregate(blk, THR, T, hw, None, pools=POOLS, persistence=True, fss=FSS)
