"""Every plan the short-GEMM planner can pick, with exact products.  The operands are integers in -8 .. 8 (exact in fp32 and in bf16) and the
reduction is at most 16384 long, so every product is an integer of magnitude <= 64 and every partial sum one of magnitude <= 2^20: exact in
fp32 in ANY order of summation, through any tile, any number of waves per tile, any number of slabs.  The result must therefore equal the
fp64 product of the same integers bit for bit; a chunk of the reduction nobody owns, a slab summed twice, a lost arrival or a load that
leaves the payload cannot hide behind a tolerance.

The cases (gemm_plan_cases.py, whose census test_gemm_plans_host.py checks without a GPU): every row of the measured table, the rule-made
plans outside it, the weight-gradient rules alone and queued, the same through strided column views of poisoned buffers, and the split
launches of one stream in changing order (the arrival counters of the stream's region must be back at zero after each)."""
import contextlib
import zlib

import pytest
import torch

import gemm_plan_cases as C
from adnm_hip import ops, lib
from util import embed, assert_pads_untouched

pytestmark = pytest.mark.gpu

DEV = "cuda"
NT, NN, TN = C.NT, C.NN, C.TN
PRECS = ("f32", "bf16")


@pytest.fixture
def bf16_mfma():
    ops.set_mfma_precision("bf16")
    yield
    ops.set_mfma_precision("f32")


@pytest.fixture(params=PRECS)
def prec(request):
    if request.param == "bf16":
        request.getfixturevalue("bf16_mfma")
    return request.param


@contextlib.contextmanager
def precision(name):
    ops.set_mfma_precision(name)
    try:
        yield int(name == "bf16")
    finally:
        ops.set_mfma_precision("f32")


# ------------------------------------------------------------------------------------------------ operands and the check
_POOL_N = 1 << 23
_pool = []


def ints(tag, shape):
    """integers drawn uniformly from -8 .. 8 as fp32, a pure function of (tag, shape): a window of one seeded pool, in its own memory"""
    if not _pool:
        g = torch.Generator().manual_seed(0x5EED)
        _pool.append(torch.randint(-8, 9, (_POOL_N,), generator=g, dtype=torch.int8).to(DEV).float())
    n = 1
    for s in shape:
        n *= s
    assert n < _POOL_N
    off = zlib.crc32(tag.encode()) % (_POOL_N - n)
    return _pool[0][off:off + n].view(shape).clone()


class Problem:
    """operands and the fp64 reference of one (op, I, J, R): made once per shape and shared by the precisions and forms that run it"""

    def __init__(self, op, I, J, R, bias):
        self.op, self.I, self.J, self.R, self.id = op, I, J, R, C.case_id(op, I, J, R)
        if op == NT:      # x (M, K), w (N, K): y = x w^T + b
            self.a, self.b = ints(self.id + ".a", (I, R)), ints(self.id + ".b", (J, R))
            self.bias = ints(self.id + ".bias", (J,)) if bias else None
            self.ref = self.a.double() @ self.b.double().t()
            if bias:
                self.ref += self.bias.double()
        elif op == NN:    # dy (M, N), w (N, K): dx = dy w
            self.a, self.b, self.bias = ints(self.id + ".a", (I, R)), ints(self.id + ".b", (R, J)), None
            self.ref = self.a.double() @ self.b.double()
        else:             # dy (M, N), x (M, K): dw = dy^T x, db = column sums of dy
            self.a, self.b, self.bias = ints(self.id + ".a", (R, I)), ints(self.id + ".b", (R, J)), bias
            self.ref = self.a.double().t() @ self.b.double()
            self.ref_db = self.a.double().sum(0)
        assert float(self.ref.abs().max()) <= 64.0 * R + 8 and bool((self.ref == self.ref.round()).all())

    def launch(self, out=None, narrow=False, a=None, b=None):
        """NT / NN through the wrappers the model calls; narrow: the weight read from its bf16 shadow"""
        a, b = (self.a if a is None else a), (self.b if b is None else b)
        nw = None
        if narrow:
            self._w16 = b.to(torch.bfloat16).contiguous()
            nw = (self._w16.data_ptr(), 1, None)
        if self.op == NT:
            return ops.k_linear(a, b, self.bias, out=out, narrow=nw)
        return ops.k_linear_dx(a, b, out=out, narrow=nw)


_problems = {}


def problem(op, I, J, R, bias=False):
    k = (op, I, J, R, bool(bias))
    if k not in _problems:
        if len(_problems) >= 8:   # a test touches few shapes; keep the last ones for the precision / form that comes next
            _problems.pop(next(iter(_problems)))
        _problems[k] = Problem(op, I, J, R, bias)
    return _problems[k]


def assert_exact(got, ref, case, p, what):
    g = got.double()
    if g.shape == ref.shape and torch.equal(g, ref):
        return
    assert g.shape == ref.shape, f"{case} {what}: shape {tuple(g.shape)}, expected {tuple(ref.shape)}"
    bad = ~(g == ref)   # (a NaN differs)
    g2, r2, b2 = (t.reshape(t.shape[0], -1) if t.dim() > 1 else t.reshape(1, -1) for t in (g, ref, bad))
    r, c = (int(v) for v in b2.nonzero()[0])
    raise AssertionError(f"{case} {what}: plan [{C.show(p)}]: {int(bad.sum())} of {bad.numel()} elements differ from the fp64 product, "
                         f"first at (row {r}, column {c}): got {float(g2[r, c])!r}, expected {float(r2[r, c])!r}")


def with_bias(index):
    return index % 4 == 0


# ------------------------------------------------------------------------------------------------ 3a: every row of the measured table
TABLE = C.table_cases()
ROWS = {(op, I, J, R, bf16): cfg for op, I, J, R, bf16, cfg in C.table_rows()}


@pytest.mark.parametrize("index", range(len(TABLE)), ids=[C.case_id(*s) for s in TABLE])
def test_table_rows_give_exact_products(index):
    """NT rows through ops.k_linear (one in four with a bias), NN rows through ops.k_linear_dx; the f32 row and the bf16 row of the shape;
    in the bf16 mode once more with the weight read from its bf16 shadow"""
    op, I, J, R = TABLE[index]
    pr = problem(op, I, J, R, bias=op == NT and with_bias(index))
    for name in PRECS:
        with precision(name) as bf16:
            p = C.plan(op, I, J, R, bf16)
            assert p["source"] == 0 and (op, I, J, R, bf16) in ROWS, f"{pr.id} {name}: not planned from the table: {C.show(p)}"
            assert_exact(pr.launch(), pr.ref, pr.id, p, f"{name}, row {ROWS[(op, I, J, R, bf16)]}")
            if bf16:
                assert_exact(pr.launch(narrow=True), pr.ref, pr.id, p, "bf16, weight from its bf16 shadow")


# ------------------------------------------------------------------------------------------------ 3b: the rules, NT / NN
def _out_buffer(I, J):
    """an (I, J) output as a column view of a bit-poisoned buffer whose row stride is a multiple of 4 whatever J is"""
    left, right = 4, 8 + (-J) % 4
    buf, view = embed(torch.zeros((I, J), device=DEV), left, right, poison="bits")
    return buf, view, left


@pytest.mark.parametrize("index", range(len(C.RULE_CASES)), ids=[c.id for c in C.RULE_CASES])
def test_rule_made_plans_give_exact_products(index):
    case = C.RULE_CASES[index]
    op, I, J, R = case.shape
    pr = problem(op, I, J, R, bias=op == NT and index % 2 == 0)
    for name in PRECS:
        with precision(name) as bf16:
            p = C.plan(op, I, J, R, bf16)
            assert p["source"] == 1 and case.reaches(p), f"{case.id} {name}: there for '{case.branch}' but plans {C.show(p)}"
            for narrow in ((False, True) if bf16 else (False,)):
                what = name + (", weight from its bf16 shadow" if narrow else "")
                if case.shape in C.MISALIGNED:   # J % 4 != 0: only a column view of a wider buffer gives rows 4-aligned
                    buf, view, left = _out_buffer(I, J)
                    y = pr.launch(out=view, narrow=narrow)
                    assert y is view
                    assert_pads_untouched(buf, left, J, f"{case.id} {what}")
                else:
                    y = pr.launch(narrow=narrow)
                assert_exact(y, pr.ref, case.id, p, what)


# ------------------------------------------------------------------------------------------------ 3c: views
@pytest.mark.parametrize("index", range(len(C.RULE_CASES)), ids=[c.id for c in C.RULE_CASES])
def test_rule_made_plans_on_column_views(index):
    """both operands column views of NaN-filled wider buffers, the output a column view of a bit-poisoned one: a clamped load may not leave
    the payload, a zeroed reduction step may not meet a NaN, no store may leave the view"""
    case = C.RULE_CASES[index]
    op, I, J, R = case.shape
    pr = problem(op, I, J, R, bias=op == NT and index % 2 == 0)
    _, av = embed(pr.a, 8, 4, poison="nan")
    _, bv = embed(pr.b, 4, 12, poison="nan")
    for name in PRECS:
        with precision(name) as bf16:
            p = C.plan(op, I, J, R, bf16)
            assert case.reaches(p)
            buf, view, left = _out_buffer(I, J)
            y = pr.launch(out=view, a=av, b=bv)
            assert y is view and av.stride(0) != av.shape[1] and bv.stride(0) != bv.shape[1]
            assert_exact(y, pr.ref, case.id, p, f"{name}, column views")
            assert_pads_untouched(buf, left, J, f"{case.id} {name}")


# ------------------------------------------------------------------------------------------------ 3b: the weight-gradient rules
def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


@pytest.mark.parametrize("index", range(len(C.TN_CASES)), ids=[c.id for c in C.TN_CASES])
def test_weight_gradient_plans_alone(index):
    """ops.k_linear_dw(..., now=True): launched where it is produced, 2048 waves wanted; the direct path (a strided destination takes no
    partials) on the cases that would otherwise split"""
    case = C.TN_CASES[index]
    _, I, J, R = case.shape
    pr = problem(TN, I, J, R, bias=case.bias)
    dev = pr.a.device
    for name in PRECS:
        with precision(name) as bf16, torch.no_grad():
            p = C.plan(TN, I, J, R, bf16)
            assert p["source"] == 1 and case.alone(p), f"{case.id} {name}: there for '{case.branch}' but plans {C.show(p)}"
            dw, db = ops.k_linear_dw(pr.a, pr.b, case.bias, dw_out=_nan(I, J), now=True)
            assert_exact(dw, pr.ref, case.id, p, f"{name}, dw")
            if case.bias:
                assert_exact(db, pr.ref_db, case.id, p, f"{name}, dbias")
            if case.direct:
                d = C.plan(TN, I, J, R, bf16, direct=1)
                assert p["nbs"] > 1 and d["nbs"] == 1
                buf, view = embed(_nan(I, J), 8, 4, poison="bits")
                dw, db = ops.k_linear_dw(pr.a, pr.b, case.bias, dw_out=view, now=True)
                assert dw is view
                assert_exact(dw, pr.ref, case.id, d, f"{name}, dw into a strided destination")
                assert_pads_untouched(buf, 8, J, f"{case.id} {name}")
                if case.bias:
                    assert_exact(db, pr.ref_db, case.id, d, f"{name}, dbias beside a strided dw")
    assert ops.FOLDS.deferring(dev) is False


def test_weight_gradient_plans_queued(prec):
    """inside a backward scope (ops.FOLDS.active) a weight gradient that nobody reads at once waits in the leaf queue: it is planned for
    256 waves, and the scope's flush launches the queued problems grouped, their folds behind them"""
    dev = torch.device(DEV, torch.cuda.current_device())
    prs = [Problem(TN, c.I, c.J, c.R, c.bias) for c in C.TN_CASES]
    outs, plans, name, bf16 = [], [], prec, int(prec == "bf16")
    with torch.no_grad():
        with ops.FOLDS.active(dev, on=True):
            ent = ops.FOLDS._q[dev.index]
            assert ent["lh"] is not None, "the leaf queue is on by default"
            for case, pr in zip(C.TN_CASES, prs):
                with ops.FOLDS.defer(dev):   # the queues bound, as around the library call itself
                    q = C.plan(TN, case.I, case.J, case.R, bf16)
                assert q["source"] == 1 and case.queued(q), f"{case.id} {name} queued: plans {C.show(q)}"
                plans.append(q)
                outs.append(ops.k_linear_dw(pr.a, pr.b, case.bias, dw_out=_nan(case.I, case.J)))
            assert lib.query("adnm_leafq_pending", ent["lh"]) == len(prs), "every weight gradient waits for the grouped launch"
        assert lib.query("adnm_leafq_pending", ent["lh"]) == 0
        assert len({q["nbs"] for q in plans if 1 < q["nbs"] < 64}) >= 2
        for case, pr, q, (dw, db) in zip(C.TN_CASES, prs, plans, outs):
            assert_exact(dw, pr.ref, case.id, q, f"{name}, queued, dw")
            if case.bias:
                assert_exact(db, pr.ref_db, case.id, q, f"{name}, queued, dbias")


# ------------------------------------------------------------------------------------------------ 3d: the counters return to idle
def _split_cases(bf16):
    shapes = TABLE + [c.shape for c in C.RULE_CASES if c.shape not in C.MISALIGNED]
    return [s for s in shapes if s[0] != TN and C.plan(*s, bf16)["nbs"] > 1]


@pytest.mark.parametrize("uc", ["1", "0"], ids=["uncached-slabs", "fenced-slabs"])
def test_split_launches_leave_the_counters_idle(prec, uc, monkeypatch):
    """every split NT / NN case on one stream: in order, reversed, then each twice in a row.  The stream's split region is shared by all
    shapes (ops.SPLITWS): arrival counters one shape leaves behind show in the next one's result.  Both slab protocols."""
    monkeypatch.setenv("ADNM_SK_UC_SLABS", uc)
    name, bf16 = prec, int(prec == "bf16")
    shapes = _split_cases(bf16)
    kernels = {C.plan(*s, bf16)["kernel"] for s in shapes}
    assert len(shapes) >= 20 and kernels == {C.STREAM, C.LDS}, "split launches of both kernels"
    prs = [Problem(*s, bias=s[0] == NT and with_bias(k)) for k, s in enumerate(shapes)]
    order = list(range(len(prs))) + list(reversed(range(len(prs)))) + [k for k in range(len(prs)) for _ in (0, 1)]
    outs = [(k, prs[k].launch()) for k in order]
    for n, (k, y) in enumerate(outs):
        assert_exact(y, prs[k].ref, prs[k].id, C.plan(*shapes[k], bf16), f"{name}, launch {n} of {len(order)} on the stream")
