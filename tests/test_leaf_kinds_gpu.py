"""The three weight-gradient kinds that joined the leaf queue (include/adnm_hip.h: adnm_leafq_*): the 3x3 column walker (csrc/dwconv.hip), the
dense 3x3 conv's weight gradient (csrc/conv3.hip) and the tall column sum (csrc/core.hip).  Queued, a problem keeps the plan of its single
launch, so every gradient is, bit for bit, what the same call gives with no queue bound; n queued problems of one kind and instantiation
take ceil(n / 16) launches; the operands of a queued problem live until the flush; ADNM_LEAF_INLINE sends a kind back inline."""
import ctypes
import os

import pytest
import torch

from adnm_hip import lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 16   # problems per grouped launch (kMaxWg, kMaxWgLeaf, kMaxColsum)
KIND_WALK3, KIND_CONV3, KIND_COLSUM = 4, 5, 6   # csrc/adnm_common.h: ADNM_LEAF_*
NEW_KINDS_MASK = (1 << KIND_WALK3) | (1 << KIND_CONV3) | (1 << KIND_COLSUM)


def _dev():
    return torch.device(DEV, torch.cuda.current_device())


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(DEV)


class _Events:
    """with _Events() as ev: ...  -> ev.count[scope] = launches the library's opt-in profiler saw under that scope (one event per launch,
    merged or not: include/adnm_hip.h, adnm_prof_*)"""

    def _collect(self):
        buf = ctypes.create_string_buffer(1 << 20)
        lib.query("adnm_prof_collect", buf, len(buf))   # (collecting also clears the records)
        count = {}
        for line in buf.value.decode().splitlines():
            name, cnt = line.split("\t")[:2]
            count[name.split("@")[0]] = count.get(name.split("@")[0], 0) + int(cnt)
        return count

    def __enter__(self):
        self._collect()
        self.count = {}
        lib.query("adnm_prof_enable", 1)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        lib.query("adnm_prof_enable", 0)
        self.count = self._collect()
        return False


class _Inline:
    """with _Inline(mask): the kinds of the mask launch where they are produced although a queue is bound (ADNM_LEAF_INLINE)"""

    def __init__(self, mask):
        self.mask = mask

    def __enter__(self):
        self.old = os.environ.get("ADNM_LEAF_INLINE")
        os.environ["ADNM_LEAF_INLINE"] = str(self.mask)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("ADNM_LEAF_INLINE", None)
        else:
            os.environ["ADNM_LEAF_INLINE"] = self.old
        return False


# ---- problems: a callable that makes its library call(s) through the package's own wrappers and returns the gradients it produced
def walker(seed, B, H, W, C, bias=False, chan_major=False, act=lib.ACT_NONE, K=3):
    M = B * H * W
    x, dy = _rand((M, C), seed), _rand((M, C), seed + 1)
    wt = _rand((C, K * K) if chan_major else (K * K, C), seed + 2, 0.3)
    b = _rand((C,), seed + 3, 0.3) if bias else None

    def run():
        dx, dwt, db = ops.k_dwconv_bwd(dy, x, wt, b, B, H, W, C, K, act, want_bias=bias, chan_major=chan_major)
        return [dx, dwt] + ([db] if bias else [])
    return run


def conv3(seed, B, H, W, K, N, prec, bias=True):
    M = B * H * W
    x, dy = _rand((M, K), seed), _rand((M, N), seed + 1)

    def run():
        dw = torch.full((N, 3, 3, K), float("nan"), device=DEV)
        db = torch.full((N,), float("nan"), device=DEV) if bias else None
        nb = lib.query("adnm_conv3_wgrad_ws_bytes", B, H, W, K, N)
        ws = ops._ws(nb, x.device)
        with ops.FOLDS.defer(x.device, ws, dy, x):
            lib.call("adnm_conv3_wgrad", dy.data_ptr(), N, x.data_ptr(), K, dw.data_ptr(), ops._p(db), ws.data_ptr(), nb, B, H, W, K, N, prec,
                     ops._stream())
        return [dw] + ([db] if bias else [])
    return run


def colsum(seed, M, N):
    t = _rand((M, N), seed)
    return lambda: [ops.colsum(t, defer=True)]


def linear_dw(seed, M, N, K):
    """M >= 32768: the tall-skinny TN GEMM; below: the short one"""
    dy, x = _rand((M, N), seed), _rand((M, K), seed + 1)
    return lambda: list(ops.k_linear_dw(dy, x, True))


def run(problems, queued, events=None, inline=0):
    """every problem's gradients; queued: inside a trainer's backward scope (fold and leaf queues bound around the calls, flushed on the way
    out); events: receives the launch counts per scope, flush included"""
    dev = _dev()
    with torch.no_grad(), _Events() as ev, _Inline(inline):
        with ops.FOLDS.active(dev, on=queued):
            outs = [p() for p in problems]
    if events is not None:
        events.append(ev.count)
    return outs


def same(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w)
        for j, (a, b) in enumerate(zip(g, w)):
            assert a.shape == b.shape and torch.equal(a, b), f"{what}: result {j} of problem {i}: max |diff| {float((a - b).abs().max())}"


@pytest.fixture(scope="module")
def inline_ref():
    """the results of a set of problems with no queue bound, computed once per set"""
    memo = {}

    def get(key, make):
        if key not in memo:
            problems = make()
            memo[key] = (problems, run(problems, False))
        return memo[key]
    return get


# ---------------------------------------------------------------------------------------------------------------- 3x3 column walker
# H * W >= 16 384 takes the walker.  One and two channel quads; W no multiple of the 4-pixel strip with three quads and two images; a tall map.
WALK_SHAPES = [(1, 128, 128, 4), (1, 128, 128, 8), (2, 128, 130, 12), (1, 256, 64, 8)]


def _walk_set(shape):
    """the eight combinations of bias, weight layout and fused SiLU (a dpre operand) in one queue"""
    return [walker(100 * i + shape[3], *shape, bias=bool(i & 1), chan_major=bool(i & 2), act=lib.ACT_SILU if i & 4 else lib.ACT_NONE)
            for i in range(8)]


@pytest.mark.parametrize("shape", WALK_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_walker_queued_equals_inline(inline_ref, shape):
    problems, want = inline_ref(("walk", shape), lambda: _walk_set(shape))
    ev = []
    same(run(problems, True, ev), want, f"walker {shape}")
    assert ev[0].get("dwconv_wgrad_k3") == 1, ev[0]   # eight problems, one launch
    ev = []
    run(problems, False, ev)
    assert ev[0].get("dwconv_wgrad_k3") == 8, ev[0]


def test_walker_more_problems_than_a_table_holds(inline_ref):
    make = lambda: [walker(7000 + 10 * i, 1, 128, 128, 4, bias=bool(i & 1)) for i in range(CAP + 1)]
    problems, want = inline_ref("walk17", make)
    ev = []
    same(run(problems, True, ev), want, "17 walker problems")
    assert ev[0].get("dwconv_wgrad_k3") == 2, ev[0]   # 16 + 1


# ---------------------------------------------------------------------------------------------------------------- conv3 weight gradient
# (B, H, W, Cin, Cout): the smallest shape; W no multiple of the 16-pixel block, ragged channels; two images (the zero row between them) on the
# 8-wide geometry; 68 pixel tiles walked by 28 row bands (several tiles per workgroup, many partial rows); NB = 1 and NB = 2 instantiations
CONV3_SHAPES = [(1, 1, 1, 1, 1), (1, 5, 18, 3, 5), (2, 6, 8, 16, 20), (2, 64, 64, 64, 128)]


@pytest.mark.parametrize("prec", [0, 1], ids=["f32", "bf16"])
def test_conv3_queued_equals_inline(inline_ref, prec):
    make = lambda: [conv3(300 + 10 * i, *s, prec, bias=(i != 1)) for i, s in enumerate(CONV3_SHAPES)]
    problems, want = inline_ref(("conv3", prec), make)
    for g in want:
        assert all(bool(torch.isfinite(t).all()) for t in g)   # every element of dw / dbias is written
    ev = []
    same(run(problems, True, ev), want, f"conv3 prec {prec}")
    assert ev[0].get("conv3_wgrad") == 2, ev[0]   # Cout <= 16 (NB = 1): two problems, one launch; NB = 2: the other two
    ev = []
    run(problems, False, ev)
    assert ev[0].get("conv3_wgrad") == 4, ev[0]


def test_conv3_instantiations_share_a_queue(inline_ref):
    """f32 and bf16 problems of both NB in one queue: one launch per (NB, PREC) present, 17 problems of one instantiation take two"""
    def make():
        ps = [conv3(500 + 10 * i, *CONV3_SHAPES[i % 3], i & 1) for i in range(6)]
        return ps + [conv3(900 + 10 * i, 1, 5, 18, 3, 5, 0) for i in range(CAP + 1)]
    problems, want = inline_ref("conv3mix", make)
    ev = []
    same(run(problems, True, ev), want, "conv3 mixed instantiations")
    # shapes 0 and 1 are NB = 1, shape 2 is NB = 2; i & 1 alternates the precision: (1, f32) x 2 + 17 -> 2 launches, (1, bf16) x 2 -> 1,
    # (2, f32) x 1 -> 1, (2, bf16) x 1 -> 1
    assert ev[0].get("conv3_wgrad") == 5, ev[0]


# ---------------------------------------------------------------------------------------------------------------- tall column sum
# 2048 rows: the smallest two-stage problem (8 bands of 256); 2085 rows: bands of 261 with a short last one; 36 columns: more than a power of two
COLSUM_SHAPES = [(2048, 32), (2048, 36), (2085, 32), (2085, 36), (70000, 32)]


def test_colsum_queued_equals_inline(inline_ref):
    make = lambda: [colsum(40 + i, *s) for i, s in enumerate(COLSUM_SHAPES)] + [colsum(60, 2047, 32)]   # (one below: a single fold, no leaf)
    problems, want = inline_ref("colsum", make)
    for (M, N), g in zip(COLSUM_SHAPES, want):
        ref = _rand((M, N), 40 + COLSUM_SHAPES.index((M, N))).double().sum(0)
        assert float((g[0].double() - ref).abs().max()) <= 1e-5 * M ** 0.5 * 8, (M, N)   # sanity: it IS the column sum
    ev = []
    same(run(problems, True, ev), want, "colsum")
    assert ev[0].get("colsum_partial") == 1, ev[0]
    ev = []
    run(problems, False, ev)
    assert ev[0].get("colsum_partial") == len(COLSUM_SHAPES), ev[0]


# ---------------------------------------------------------------------------------------------------------------- all seven kinds together
def _new_kinds():
    return [walker(1, 1, 128, 128, 8, bias=True, act=lib.ACT_SILU), conv3(11, 2, 6, 8, 16, 20, 0), colsum(21, 2085, 36),
            walker(31, 1, 128, 128, 4, chan_major=True), conv3(41, 1, 5, 18, 3, 5, 1), colsum(51, 2048, 32), conv3(61, 1, 5, 18, 3, 5, 0)]


def _old_kinds():
    # the short TN GEMM, the tap-row 3x3 kernel (a map below 128 x 128), the 5x5 walker, the tall-skinny TN GEMM
    return [linear_dw(71, 512, 32, 64), walker(81, 1, 16, 16, 8, bias=True), walker(91, 1, 16, 16, 8, K=5), linear_dw(101, 32768, 32, 32)]


def test_all_kinds_in_one_queue(inline_ref):
    new, want_new = inline_ref("mixed_new", _new_kinds)
    # the four older kinds plan for the group when a queue is bound (fewer, longer slices): their reference is the same call under a bound
    # queue with the kind sent inline — same plan, launched alone
    old = _old_kinds()
    want_old = run(old, True, inline=15)
    problems, want = new + old, want_new + want_old
    for round_ in range(3):   # once, then twice back to back
        ev = []
        got = run(problems, True, ev)
        same(got, want, f"round {round_}")
        c = ev[0]
        # walker: 2 problems, 1 launch, + the tap-row kernel's own grouped launch under the same scope
        assert c.get("dwconv_wgrad_k3") == 2 and c.get("dwconv_wgrad_k5") == 1, c
        assert c.get("conv3_wgrad") == 3, c   # (2, f32), (1, bf16), (1, f32)
        assert c.get("colsum_partial") == 1 and c.get("skgemm_tn") == 1 and c.get("tsgemm_tn") == 1, c


def test_inline_switch_sends_a_kind_back(inline_ref):
    new, want = inline_ref("mixed_new", _new_kinds)
    for kind, scope, n in ((KIND_WALK3, "dwconv_wgrad_k3", 2), (KIND_CONV3, "conv3_wgrad", 3), (KIND_COLSUM, "colsum_partial", 2)):
        ev = []
        same(run(new, True, ev, inline=1 << kind), want, f"kind {kind} inline")
        grouped = {"dwconv_wgrad_k3": 1, "conv3_wgrad": 3, "colsum_partial": 1}
        for s, g in grouped.items():
            assert ev[0].get(s) == (n if s == scope else g), (kind, ev[0])   # that kind per problem, the others grouped
    ev = []
    same(run(new, True, ev, inline=NEW_KINDS_MASK), want, "all three inline")
    assert (ev[0].get("dwconv_wgrad_k3"), ev[0].get("conv3_wgrad"), ev[0].get("colsum_partial")) == (2, 3, 2), ev[0]


def test_error_between_push_and_flush_launches_nothing():
    dev = _dev()
    problems = _new_kinds()
    ops.FOLDS.enable(dev, False)   # (creates the device's queues)
    ent = ops.FOLDS._q[dev.index]
    with torch.no_grad(), _Events() as ev:
        with pytest.raises(RuntimeError, match="the body fails"):
            with ops.FOLDS.active(dev):   # a backward scope whose body raises drops what is queued (FoldRegistry.abort: adnm_leafq_clear)
                for p in problems[1:4]:   # conv3, colsum, a walker without activation: nothing of them launches before the flush
                    p()
                assert lib.query("adnm_leafq_pending", ent["lh"]) == 3 and lib.query("adnm_foldq_pending", ent["h"]) == 3
                raise RuntimeError("the body fails")
    assert lib.query("adnm_leafq_pending", ent["lh"]) == 0 and lib.query("adnm_foldq_pending", ent["h"]) == 0 and not ent["keep"]
    for scope in ("dwconv_wgrad_k3", "conv3_wgrad", "colsum_partial", "dwconv_wgrad_fold", "conv3_wgrad_fold", "colsum", "fold_batch"):
        assert scope not in ev.count, ev.count
    # the queues work again afterwards
    want = run(problems, False)
    same(run(problems, True), want, "after the aborted pass")


# ---------------------------------------------------------------------------------------------------------------- operand lifetime
def test_operands_live_until_the_flush():
    """a queued problem reads its operands at the flush: Conv3Fn.backward and k_dwconv_bwd_w must keep them although the caller lets go"""
    dev = _dev()
    B, H, W, K, N = 1, 128, 128, 8, 8
    M = B * H * W

    def node(with_queue):
        # everything the two backward wrappers read is created here and referenced by nobody else when they return
        x, w, pre, dy = _rand((M, K), 1), _rand((N, K, 3, 3), 2, 0.2), _rand((M, N), 3), _rand((B, H * W, N), 4)
        ctx = ops._SubCtx(6)
        ctx.needs_input_grad = (False, True, False, False, False, False)   # the weight gradient alone
        ctx.save_for_backward(x, w, pre)
        ctx.meta = (B, H, W, K, N, lib.ACT_GELU, ops._conv3_wstrides(w), 0, False)   # with GELU: dy2 is a dpre made inside backward
        xs, dys, taps = _rand((M, K), 5), _rand((M, K), 6), _rand((9, K), 7, 0.3)
        with ops.FOLDS.active(dev, on=with_queue):
            _, g, _, _, _, _ = ops.Conv3Fn.backward(ctx, dy)
            _, dwt, _ = ops.k_dwconv_bwd(dys, xs, taps, None, B, H, W, K, 3, lib.ACT_SILU)
            del ctx, x, pre, dy, xs, dys
            # fresh tensors of the operands' sizes: the allocator hands out the memory of whatever was let go
            junk = [torch.full((M, K), float("nan"), device=DEV) for _ in range(8)]
            junk += [torch.full((B, H * W, N), float("nan"), device=DEV) for _ in range(4)]
        del junk
        return g.clone(), dwt.clone()

    with torch.no_grad():
        want = node(False)
        got = node(True)
    torch.cuda.synchronize()
    assert torch.isfinite(want[0]).all() and torch.isfinite(want[1]).all()
    assert torch.equal(got[0], want[0]), "conv3 weight gradient: an operand was released before the flush"
    assert torch.equal(got[1], want[1]), "walker tap gradient: an operand was released before the flush"
