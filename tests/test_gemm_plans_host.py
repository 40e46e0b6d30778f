"""The short-GEMM planner without a GPU, through the read-only query adnm_skgemm_plan (the planner the launch itself calls): the entry
point at the C boundary, every row of the measured table honoured after the legal clamps, the invariants the kernels assume over a sweep
of the rule boundaries, and the census of gemm_plan_cases — the list test_gemm_plans_gpu.py multiplies out — against the plans it is
meant to reach."""
import ctypes
import itertools

import pytest

import gemm_plan_cases as C
from adnm_hip import lib

NT, NN, TN = C.NT, C.NN, C.TN


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the C boundary
def test_the_prototype_is_declared_and_exported_and_the_abi_version_stays():
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    assert "adnm_skgemm_plan" in protos, "adnm_skgemm_plan is not declared in include/adnm_hip.h"
    assert hasattr(so, "adnm_skgemm_plan"), "adnm_skgemm_plan declared but not exported"
    assert protos["adnm_skgemm_plan"] == ("int", ["int", "int64_t", "int64_t", "int64_t", "int", "int", "int*"])
    assert lib.load().adnm_abi_version() == 11


def test_the_query_refuses_what_the_launch_refuses():
    out = (ctypes.c_int * 10)()
    ptr = ctypes.cast(out, ctypes.c_void_p)
    for op, M, N, K in ((NT, 64, 64, 6), (NN, 64, 6, 64), (TN, 64, 64, 6), (3, 64, 64, 64), (NT, 0, 64, 64), (NT, 64, 16388, 64), (NT, 64, 64, 16388),
                        (NT, (1 << 20) + 1, 64, 64), (NT, 1 << 20, 2048, 64)):
        assert lib.query("adnm_skgemm_supported", op, M, N, K) == 0
        assert lib.load().adnm_skgemm_plan(op, M, N, K, 0, 0, ptr) != 0 and "skgemm_plan" in lib.last_error()
    assert lib.load().adnm_skgemm_plan(NT, 64, 64, 64, 0, 0, None) != 0
    with pytest.raises(RuntimeError, match="adnm_skgemm_plan"):
        C.plan(NT, 64, 64, 6, 0)


# ------------------------------------------------------------------------------------------------ what the kernels assume of a plan
INSTANCES = {NT: {(1, 1, 4), (2, 2, 2), (4, 4, 1)}, NN: {(1, 4, 2), (2, 4, 2), (4, 4, 1)}, TN: {(4, 4, 1)}}   # the streaming kernels that exist


def ticket_bytes(ntiles):
    return (ntiles * 4 + 255) // 256 * 256


def needs(op, I, J, p):
    """(workspace bytes, counter bytes) a launch of plan p touches: [arrival counters (in-launch combine) | nbs slabs]; the LDS-tiled
    kernel keeps whole 64 x 64 tiles per slice, the streaming one I x J (+ I bias sums) per slice"""
    if p["nbs"] <= 1:
        return 16, 0
    if p["kernel"] == C.LDS:
        ntiles = cdiv(I, 64) * cdiv(J, 64)
        return ticket_bytes(ntiles) + ntiles * p["nbs"] * 64 * 64 * 4, ticket_bytes(ntiles)
    ntiles = cdiv(I, 16 * p["tm"]) * cdiv(J, 16 * p["tn"])
    tick = ticket_bytes(ntiles) if p["combine"] else 0
    return tick + p["nbs"] * (I * J + I) * 4, tick


def check_plan(op, I, J, R, bf16, direct, p, what):
    """the invariants; `what` names the case in a failure"""
    msg = f"{what}: {C.OPS[op]} I={I} J={J} R={R} bf16={bf16} direct={direct}: {C.show(p)}"
    tile = (p["tm"], p["tn"], p["kc"])
    if p["kernel"] == C.LDS:
        assert op != TN and tile == (4, 4, 2) and p["wpt"] == 1, msg
    else:
        assert p["kernel"] == C.STREAM and tile in INSTANCES[op], msg
    assert p["nchunks"] == cdiv(R, 16 * p["kc"]), msg
    assert p["wpt"] in (1, 2, 4, 8) and p["wpt"] <= max(1, p["nchunks"]), msg
    assert 1 <= p["nbs"] <= (64 if op == TN else 32) and p["cpw"] >= 1, msg
    assert p["nbs"] * p["wpt"] * p["cpw"] >= p["nchunks"], "a chunk without an owner: " + msg
    assert (p["nbs"] - 1) * p["wpt"] * p["cpw"] < p["nchunks"], "an empty slice: " + msg
    if direct or J % 4:
        assert p["nbs"] == 1, "split where the output takes no partials: " + msg
    assert p["combine"] == int(p["nbs"] > 1 and op != TN), msg
    assert p["source"] in (0, 1), msg


# ------------------------------------------------------------------------------------------------ the measured table
def test_the_table_parses_whole():
    rows = C.table_rows()
    assert len(rows) == 164 and len({r[:5] for r in rows}) == 164, "164 rows, no (op, shape, precision) twice"
    assert {r[0] for r in rows} == {NT, NN} and all(lib.query("adnm_skgemm_supported", r[0], *C.mnk(*r[:4])) == 1 for r in rows)
    assert len(C.table_cases()) == 82, "every shape has its f32 and its bf16 row"


def expected_of_row(op, I, J, R, cfg):
    """what a row's {kernel, tm, tn, kc, wpt, nbs} launches as: the legal clamps are (1) no more waves per tile than chunks, (2) slices
    only with 8 waves per tile, at most 32, (3) no more slices than the chunks per wave leave non-empty; the LDS-tiled kernel: (3) over its
    32-step tiles"""
    kernel, tm, tn, kc, wpt, nbs = cfg
    if kernel == C.LDS:
        nkt = cdiv(R, 32)
        nbs = max(1, min(nbs, nkt, 32))
        return (C.LDS, 4, 4, 2, 1, cdiv(nkt, cdiv(nkt, nbs)))
    nchunks = cdiv(R, 16 * kc)
    while wpt > 1 and wpt > nchunks:
        wpt //= 2
    nbs = min(nbs, 32) if wpt == 8 else 1
    cpw = cdiv(nchunks, nbs * wpt)
    return (kernel, tm, tn, kc, wpt, cdiv(cdiv(nchunks, cpw), wpt))


def test_every_table_row_is_honoured():
    clamped = []
    for op, I, J, R, bf16, cfg in C.table_rows():
        p = C.plan(op, I, J, R, bf16)
        what = f"row {{{op}, {I}, {J}, {R}, {bf16}, {cfg}}}"
        assert p["source"] == 0, f"{what} is not what the planner takes: {C.show(p)}"
        check_plan(op, I, J, R, bf16, 0, p, what)
        want = expected_of_row(op, I, J, R, cfg)
        assert C.key(p) == want, f"{what}: launches as {C.show(p)}, the row clamps to {want}"
        if cfg[0] == C.STREAM and C.key(p) != cfg:
            clamped.append((what, C.show(p)))
        assert C.plan(op, I, J, R, bf16, 1)["nbs"] == 1
    # rows that name more waves or slices than the reduction has chunks for (the tuner measured them through the same clamps): reported
    print(f"{len(clamped)} streaming rows launch with fewer waves per tile or slices than they name")
    for what, got in clamped:
        print("  ", what, "->", got)


def test_a_shape_beside_a_row_takes_the_rules():
    for op, I, J, R, bf16, _ in C.table_rows()[::7]:
        assert C.plan(op, I + 4, J, R, bf16)["source"] == 1 and C.plan(op, I, J + 4, R, bf16)["source"] == 1 and C.plan(op, I, J, R + 4, bf16)["source"] == 1
    assert all(C.plan(TN, I, J, R, bf16)["source"] == 1 for _, I, J, R, bf16, _ in C.table_rows()[::7]), "the table has no weight-gradient rows"


# ------------------------------------------------------------------------------------------------ the sweep
# 64 x 64 tile counts at 7 / 8 (I 64 x J 448 / 512), 99 / 100 (I 576 x J 704, I 640 x J 640, I 256 x J 1600), 127 / 128 (I 64 x J 8128 /
# 8192), 255 / 256 (I 64 x J 16320 / 16384; I 1024 x J 1020 / 1024), each +- one vector of 4; I at 252 / 256 / 260; the extremes shape_ok
# allows (1 row, 4 columns, 2^20 rows, 16384 columns, a reduction of 4 and of 16384 — 2^20 for the weight gradient)
SWEEP_I = (1, 4, 60, 64, 68, 252, 256, 260, 572, 576, 580, 636, 640, 644, 1020, 1024, 1028, 16384, 1 << 20)
SWEEP_J = (4, 6, 8, 60, 64, 68, 444, 448, 452, 508, 512, 516, 518, 636, 640, 644, 700, 704, 708, 1020, 1024, 1028, 1596, 1600, 1604, 8124, 8128, 8132,
           8188, 8192, 8196, 16316, 16320, 16324, 16380, 16384)
SWEEP_R = (4, 16, 20, 64, 68, 124, 128, 132, 1020, 1024, 1028, 16380, 16384, 1 << 20)


def _sweep(op, queued):
    seen, reached = 0, set()
    for I, J, R in itertools.product(SWEEP_I, SWEEP_J, SWEEP_R):
        M, N, K = C.mnk(op, I, J, R)
        if lib.query("adnm_skgemm_supported", op, M, N, K) != 1:
            continue
        ws, cb = lib.query("adnm_skgemm_ws_bytes", op, M, N, K), lib.query("adnm_skgemm_counter_bytes", op, M, N, K)
        for bf16, direct in itertools.product((0, 1), (0, 1)):
            p = C.plan(op, I, J, R, bf16, direct)
            check_plan(op, I, J, R, bf16, direct, p, "sweep" + (" (queued)" if queued else ""))
            if not direct and not queued:   # (the byte queries plan without a queue bound, as ops._skgemm asks them)
                need, tick = needs(op, I, J, p)
                assert ws >= need and cb >= tick, f"{C.OPS[op]} I={I} J={J} R={R} bf16={bf16}: ws {ws} / counters {cb} < {need} / {tick} of {C.show(p)}"
            reached.add(C.key(p))
            seen += 1
    return seen, reached


@pytest.mark.parametrize("op", [NT, NN, TN])
def test_the_invariants_hold_over_the_rule_boundaries(op):
    seen, reached = _sweep(op, False)
    print(f"{C.OPS[op]}: {seen} plans, {len(reached)} distinct")
    assert seen > 4000
    kinds = {k[:4] for k in reached}
    if op == NT:
        assert kinds == {(0, 1, 1, 4), (0, 2, 2, 2), (1, 4, 4, 2)}, "the sweep reaches both streaming tiles of the rules and the LDS-tiled kernel"
        # (a reduction of <= 128 steps takes the LDS-tiled kernel: the streaming one never sees a single chunk here, nor NN fewer than five)
        assert {k[5] for k in reached if k[0] == 1} >= {1, 2, 4, 8} and {k[4] for k in reached if k[0] == 0} == {2, 4, 8}
    elif op == NN:
        assert kinds == {(0, 1, 4, 2), (0, 2, 4, 2), (1, 4, 4, 2)} and {k[4] for k in reached if k[0] == 0} == {4, 8}
    else:
        assert {k[4] for k in reached} == {1, 2, 4, 8} and {1, 2, 64} <= {k[5] for k in reached} and max(k[5] for k in reached) == 64


def test_the_invariants_hold_for_the_queued_weight_gradient():
    alone = {s: C.plan(TN, *s, 0) for s in ((64, 64, 16384), (128, 128, 4096), (256, 512, 1024))}
    with C.bound_queues():
        seen, reached = _sweep(TN, True)
        queued = {s: C.plan(TN, *s, 0) for s in alone}
    assert seen > 4000
    for s in alone:   # 256 waves wanted instead of 2048: fewer slices for the same shape, and the binding does not outlive its scope
        assert queued[s]["nbs"] < alone[s]["nbs"] and C.plan(TN, *s, 0) == alone[s], f"{s}: alone {C.show(alone[s])}, queued {C.show(queued[s])}"


# ------------------------------------------------------------------------------------------------ the census of the GPU file's cases
def test_the_case_list_contains_every_table_row():
    cases = set(C.all_cases())
    for op, I, J, R, bf16, _ in C.table_rows():
        assert (op, I, J, R) in cases, f"table row {C.case_id(op, I, J, R)} (bf16={bf16}) is not a case"
        assert C.plan(op, I, J, R, bf16)["source"] == 0
    assert len(C.all_cases()) == len(cases), "a case twice"


@pytest.mark.parametrize("case", C.RULE_CASES, ids=lambda c: c.id)
def test_each_rule_case_reaches_its_branch(case):
    for bf16 in (0, 1):
        p = C.plan(*case.shape, bf16)
        assert p["source"] == 1, f"{case.id} is a table row"
        assert case.reaches(p), f"{case.id} (bf16={bf16}) is there for '{case.branch}' but plans {C.show(p)}"
        check_plan(*case.shape, bf16, 0, p, case.id)
    if case.shape in C.MISALIGNED:   # the same shape with an aligned J would split
        op, I, J, R = case.shape
        assert J % 4 and C.plan(op, I, J + 2, R, 0)["nbs"] > 1 and C.plan(op, I, J + 2, R, 1)["nbs"] > 1


@pytest.mark.parametrize("case", C.TN_CASES, ids=lambda c: c.id)
def test_each_weight_gradient_case_reaches_its_branch(case):
    for bf16 in (0, 1):
        p = C.plan(*case.shape, bf16)
        assert p["source"] == 1 and case.alone(p), f"{case.id} (bf16={bf16}) is there for '{case.branch}' but plans {C.show(p)}"
        check_plan(*case.shape, bf16, 0, p, case.id)
        with C.bound_queues():
            q = C.plan(*case.shape, bf16)
        assert case.queued(q), f"{case.id} (bf16={bf16}, queued) plans {C.show(q)}"
        check_plan(*case.shape, bf16, 0, q, case.id + " queued")
        if case.direct:
            assert p["nbs"] > 1 and C.plan(*case.shape, bf16, 1)["nbs"] == 1, f"{case.id}: the direct path is tested where the shape would split"


def test_the_case_list_reaches_the_distinct_plans():
    """what section by section of the case list must be there, from the plans themselves (f32 and bf16 alike)"""
    for bf16 in (0, 1):
        rule = {c.shape: C.plan(*c.shape, bf16) for c in C.RULE_CASES}
        nt = {C.key(p) for s, p in rule.items() if s[0] == NT}
        nn = {C.key(p) for s, p in rule.items() if s[0] == NN}
        assert {(1, 4, 4, 2, 1, n) for n in (1, 2, 4, 7, 8)} <= nt, "NT LDS-tiled: unsplit and the rule-made splits"
        assert {(0, 2, 2, 2, 8, 1), (0, 1, 1, 4, 8, 1), (0, 1, 1, 4, 4, 1), (0, 1, 1, 4, 2, 1)} <= nt, "NT streaming: 32x32, 16x16, the wpt shrink"
        assert {(1, 4, 4, 2, 1, 1), (0, 1, 4, 2, 8, 1), (0, 2, 4, 2, 8, 1), (0, 2, 4, 2, 4, 1)} <= nn
        tn = [C.plan(*c.shape, bf16) for c in C.TN_CASES]
        with C.bound_queues():
            tq = [C.plan(*c.shape, bf16) for c in C.TN_CASES]
        assert {p["wpt"] for p in tn} == {1, 2, 4, 8} and {p["wpt"] for p in tq} == {1, 2, 4, 8}
        assert len({p["nbs"] for p in tn if 1 < p["nbs"] < 64}) >= 2 and len({p["nbs"] for p in tq if 1 < p["nbs"] < 64}) >= 2
        assert any(p["nbs"] == 64 for p in tn) and any(p["cpw"] > 1 and p["nbs"] > 1 for p in tn)
        assert sum(c.direct for c in C.TN_CASES) == 2 and sum(c.bias for c in C.TN_CASES) == len(C.TN_CASES) // 2
        # the table: the streaming 32 x 32 NT tile with 4 waves per tile exists only there, as do streaming splits of NT / NN
        table = {C.key(C.plan(op, I, J, R, bf16)) for op, I, J, R in C.table_cases()}
        assert (0, 2, 2, 2, 4, 1) in {C.key(C.plan(op, I, J, R, 0)) for op, I, J, R in C.table_cases()}
        assert any(k[0] == 0 and k[5] > 1 for k in table) and any(k[0] == 1 and k[5] > 1 for k in table)
    assert max(max(I * J, I * R, J * R) for _, I, J, R in C.all_cases()) == 4672 * 1024, "the largest tensor of any case: 19 MB"
    assert max(R for _, _, _, R in C.all_cases()) <= 16384, "64 R < 2^20 + 1: every partial sum of products of integers in -8 .. 8 is exact in fp32"
