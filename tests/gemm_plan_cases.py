"""The short-GEMM planner's cases, shared by test_gemm_plans_host.py (which plan does each case reach: the census) and
test_gemm_plans_gpu.py (is the product of that plan exact).  No GPU is needed to import this module or to query a plan.

A plan is what adnm_skgemm_plan (include/adnm_hip.h) reports: the library's own planner, not a transcription.  A case names the branch
of the planner it is there for as a predicate over that plan; the census asserts the predicate for the f32 and for the bf16 plan, so a
case that stops reaching its branch after a planner change fails there by name.

Shapes: NT as (M, N, K) of c[M,N] = a[M,K] b[N,K]^T; NN as (M, J, R) of c[M,J] = a[M,R] b[R,J]; TN as (N, K, M) of c[N,K] = a[M,N]^T b[M,K]
— output rows, output columns, reduction length in each."""
import contextlib
import ctypes
import os
import re

from adnm_hip import lib

NT, NN, TN = 0, 1, 2
OPS = ("NT", "NN", "TN")
STREAM, LDS = 0, 1
FIELDS = ("kernel", "tm", "tn", "kc", "wpt", "nbs", "cpw", "nchunks", "combine", "source")
TABLE_INC = os.path.join(os.path.dirname(lib.HERE), "csrc", "skgemm_tuned.inc")


def mnk(op, I, J, R):
    """the (M, N, K) adnm_skgemm takes for an op with I output rows, J output columns and a reduction of R"""
    return ((I, J, R), (I, R, J), (R, I, J))[op]


def plan(op, I, J, R, bf16, direct=0):
    """the plan adnm_skgemm launches with, as a dict over FIELDS; raises for a shape the library refuses"""
    out = (ctypes.c_int * 10)(*([-7] * 10))
    rc = lib.load().adnm_skgemm_plan(op, *mnk(op, I, J, R), int(bf16), int(direct), ctypes.cast(out, ctypes.c_void_p))
    if rc != 0:
        raise RuntimeError(f"adnm_skgemm_plan({OPS[op]}, I={I}, J={J}, R={R}) failed ({rc}): {lib.last_error()}")
    return dict(zip(FIELDS, out))


def show(p):
    kind = ("streaming", "LDS-tiled")[p["kernel"]]
    return (f"{kind} {16 * p['tm']}x{16 * p['tn']} kc={p['kc']} wpt={p['wpt']} nbs={p['nbs']} cpw={p['cpw']} nchunks={p['nchunks']} "
            f"combine={p['combine']} from {('the table', 'the rules', 'a forced plan')[p['source']]}")


def key(p):
    """what distinguishes two plans as launches: the kernel instantiation, the waves per tile and the slices"""
    return (p["kernel"], p["tm"], p["tn"], p["kc"], p["wpt"], p["nbs"])


@contextlib.contextmanager
def bound_queues():
    """a leaf queue and a fold queue bound to this thread, as around a weight-gradient call of a backward pass: the TN planner then plans
    for the grouped launch.  Host objects only; nothing is pushed."""
    L = lib.load()
    L.adnm_foldq_create.restype = L.adnm_leafq_create.restype = ctypes.c_void_p
    fq, lq = ctypes.c_void_p(L.adnm_foldq_create()), ctypes.c_void_p(L.adnm_leafq_create())
    L.adnm_foldq_bind(fq), L.adnm_leafq_bind(lq)
    try:
        yield
    finally:
        L.adnm_foldq_bind(None), L.adnm_leafq_bind(None)
        L.adnm_leafq_destroy(lq), L.adnm_foldq_destroy(fq)


# ------------------------------------------------------------------------------------------------ the measured table
_ROW = re.compile(r"^\s*\{\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*\{\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\}\s*\}\s*,")


def table_rows():
    """[(op, I, J, R, bf16, (kernel, tm, tn, kc, wpt, nbs))] — csrc/skgemm_tuned.inc read as text; every non-comment line must parse"""
    rows = []
    for n, line in enumerate(open(TABLE_INC), 1):
        if not line.strip() or line.lstrip().startswith("//"):
            continue
        m = _ROW.match(line)
        assert m, f"{TABLE_INC}:{n}: not a table row: {line!r}"
        v = [int(g) for g in m.groups()]
        rows.append((v[0], v[1], v[2], v[3], v[4], tuple(v[5:])))
    return rows


def table_cases():
    """the distinct (op, I, J, R) of the table in file order; each runs at both precisions, which covers both of its rows"""
    seen = []
    for op, I, J, R, _, _ in table_rows():
        if (op, I, J, R) not in seen:
            seen.append((op, I, J, R))
    return seen


def case_id(op, I, J, R):
    return f"{OPS[op]}-{I}x{J}x{R}"


# ------------------------------------------------------------------------------------------------ shapes outside the table
def _stream(tm, tn, kc, wpt=None, nbs=None):
    return lambda p: (p["kernel"] == STREAM and (p["tm"], p["tn"], p["kc"]) == (tm, tn, kc) and (wpt is None or p["wpt"] == wpt)
                      and (nbs is None or p["nbs"] == nbs))


def _lds(nbs):
    return lambda p: p["kernel"] == LDS and p["nbs"] == nbs


class Rule:
    """a shape the rules plan: `branch` names what it is there for, `reaches` is that as a predicate over the reported plan"""

    def __init__(self, op, I, J, R, branch, reaches):
        self.op, self.I, self.J, self.R, self.branch, self.reaches = op, I, J, R, branch, reaches
        self.id = case_id(op, I, J, R)

    @property
    def shape(self):
        return self.op, self.I, self.J, self.R


RULE_CASES = [
    # NT (M, N, K)
    Rule(NT, 520, 1028, 200, "NT LDS-tiled by tile count", _lds(1)),
    Rule(NT, 512, 1024, 1024, "NT LDS-tiled by tile count, at t64 = 128 and R = 1024: one slice", _lds(1)),
    Rule(NT, 68, 132, 128, "NT LDS-tiled by short reduction (R = 128)", _lds(1)),
    Rule(NT, 68, 132, 132, "NT streaming 16x16 just past the short reduction, wpt shrunk to 2", _stream(1, 1, 4, wpt=2, nbs=1)),
    Rule(NT, 64, 520, 1252, "NT rule-made split of the LDS-tiled kernel, 8 slices (40 step tiles, the last one ragged)", _lds(8)),
    Rule(NT, 64, 520, 1028, "NT rule-made split of the LDS-tiled kernel, 8 slices asked, 7 left by the kernel's clamp (33 step tiles)", _lds(7)),
    Rule(NT, 200, 520, 1024, "NT rule-made split of the LDS-tiled kernel, 4 slices", _lds(4)),
    Rule(NT, 260, 1000, 2052, "NT rule-made split of the LDS-tiled kernel, 2 slices", _lds(2)),
    Rule(NT, 64, 448, 1024, "NT just under the split threshold (t64 = 7): streaming 16x16", _stream(1, 1, 4, wpt=8, nbs=1)),
    Rule(NT, 256, 512, 516, "NT streaming 32x32 made by the rules", _stream(2, 2, 2, wpt=8, nbs=1)),
    Rule(NT, 72, 100, 2144, "NT streaming 16x16, ragged in every direction", _stream(1, 1, 4, wpt=8, nbs=1)),
    Rule(NT, 36, 520, 1020, "NT streaming 16x16 just under R = 1024", _stream(1, 1, 4, wpt=8, nbs=1)),
    Rule(NT, 40, 24, 132, "NT wpt shrunk to 2 by a reduction of 3 chunks", _stream(1, 1, 4, wpt=2, nbs=1)),
    Rule(NT, 40, 24, 260, "NT wpt shrunk to 4 by a reduction of 5 chunks", _stream(1, 1, 4, wpt=4, nbs=1)),
    Rule(NT, 64, 518, 1028, "NT N % 4 != 0 on a shape that would split 8 ways: one slice", _lds(1)),
    # NN (M, J, R)
    Rule(NN, 1030, 1028, 260, "NN LDS-tiled by tile count", _lds(1)),
    Rule(NN, 64, 4100, 128, "NN LDS-tiled by short reduction (R = 128)", _lds(1)),
    Rule(NN, 100, 520, 260, "NN streaming 16x64", _stream(1, 4, 2, wpt=8, nbs=1)),
    Rule(NN, 68, 260, 2052, "NN streaming 16x64, long reduction", _stream(1, 4, 2, wpt=8, nbs=1)),
    Rule(NN, 300, 1300, 516, "NN streaming 32x64 made by the rules", _stream(2, 4, 2, wpt=8, nbs=1)),
    Rule(NN, 256, 1600, 132, "NN streaming 32x64 with wpt shrunk to 4", _stream(2, 4, 2, wpt=4, nbs=1)),
]
MISALIGNED = {(NT, 64, 518, 1028)}   # J % 4 != 0: the GPU file reaches it through a column view of a 4-aligned buffer


class Wgrad:
    """a weight-gradient (TN) shape.  alone / queued: predicates over the plan with no queue bound (2048 waves wanted) and with a leaf queue
    bound (256 waves wanted); bias: the case also asks for the bias gradient; direct: also run with a strided destination"""

    def __init__(self, I, J, R, branch, alone, queued=None, bias=False, direct=False):
        self.op, self.I, self.J, self.R, self.branch, self.alone, self.queued = TN, I, J, R, branch, alone, queued or (lambda p: True)
        self.bias, self.direct, self.id = bias, direct, case_id(TN, I, J, R)

    @property
    def shape(self):
        return self.op, self.I, self.J, self.R


def _tn(wpt=None, nbs=None, fold=False):
    return lambda p: (p["kernel"] == STREAM and (p["tm"], p["tn"], p["kc"]) == (4, 4, 1) and (wpt is None or p["wpt"] == wpt)
                      and (nbs is None or p["nbs"] == nbs) and (not fold or (1 < p["nbs"] < 64 and p["combine"] == 0)))


TN_CASES = [
    Wgrad(64, 64, 16, "TN wpt 1 (one chunk)", _tn(wpt=1, nbs=1), _tn(wpt=1, nbs=1), bias=True),
    Wgrad(64, 64, 40, "TN wpt 2 (three chunks)", _tn(wpt=2), _tn(wpt=2)),
    Wgrad(64, 64, 100, "TN wpt 4 (seven chunks)", _tn(wpt=4), _tn(wpt=4), bias=True),
    Wgrad(36, 100, 300, "TN wpt 8, ragged tiles", _tn(wpt=8), _tn(wpt=8)),
    Wgrad(256, 512, 1024, "TN 1 < nbs < 64 through the fold", _tn(wpt=8, fold=True), bias=True, direct=True),
    Wgrad(512, 128, 4096, "TN 1 < nbs < 64 through the fold", _tn(wpt=8, fold=True)),
    Wgrad(1024, 2048, 64, "TN the 2 MB partial cap forcing nbs 1", _tn(nbs=1), _tn(nbs=1), bias=True),
    Wgrad(4672, 1024, 64, "TN the 2 MB partial cap forcing nbs 1 (the largest operand)", _tn(nbs=1), _tn(nbs=1)),
    Wgrad(64, 64, 16384, "TN nbs at the cap of 64, two chunks per wave", _tn(wpt=8, nbs=64), bias=True),
    Wgrad(128, 128, 4096, "TN 1 < nbs < 64 through the fold", _tn(wpt=8, fold=True), direct=True),
    Wgrad(608, 256, 1024, "TN 1 < nbs < 64 through the fold, 7 slices wanted and 3 left by the 2 MB partial cap, ragged I", _tn(wpt=8, nbs=3, fold=True), bias=True),
    Wgrad(20, 64, 4096, "TN ragged I", _tn(wpt=8)),
]


def all_cases():
    """every (op, I, J, R) the GPU file runs"""
    return table_cases() + [c.shape for c in RULE_CASES] + [c.shape for c in TN_CASES]
