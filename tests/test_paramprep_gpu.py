"""The parameter-prep kernels (csrc/paramprep.hip: adnm_adnprep_* / adnm_wtprep_*, single and grouped) against the same map stated in plain
torch on the CPU, element by element.

The kernels are permutations, single fp32 multiplies and short sums, so almost everything is checked EXACTLY:
  * integer-valued inputs (small integers stored as fp32): every product and every partial sum is an integer below 2^24, fp32 arithmetic
    is exact in any order, and EVERY output of forward and backward — the reductions included — must equal the fp64 reference cast to fp32;
  * real-valued inputs (normal draws, per-tensor scales 1e-3 .. 1e+2): copies and single fp32 multiplies must equal the fp32 torch statement
    of the same copy / multiply bit for bit; the short sums are held to k * eps32 * sum|terms| per element (the sum taken in fp64), k being the
    number of roundings a term can pass through, read off the kernel (see the comments at CHAIN_K, _alpha_k and wt's ds).
No bound in this file is fitted to a run."""
import functools
import math

import pytest
import torch

from adnm_hip import ops, lib
from util import _e4m3_bytes

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS32 = float(torch.finfo(torch.float32).eps)

ADN_SMALL = [(8, 8, 4, 4),        # the minimum adn_check admits
             (20, 40, 12, 4),     # dm no multiple of 8, half = 6, 10 heads
             (36, 72, 20, 12),    # head width no power of two
             (32, 64, 8, 4)]      # the golden's own dimensions
ADN_BIG = (512, 1024, 16, 64)     # > 1024 x 256 items: the single launch's grid-stride loop; > 512 blocks: the grouped launch's per-module cap
ADN_SHAPES = ADN_SMALL + [ADN_BIG]
WT_SHAPES = [(1, 4, 3, 0, True),      # levels = 0
             (5, 8, 5, 3, False), (8, 8, 5, 2, True), (4, 4, 3, 3, True),
             (6, 8, 3, 4, False),     # levels = 4, the maximum
             (70, 72, 5, 1, True)]    # 360 work items: more than one workgroup
KINDS = ["int", "real"]
SCALES = [1e-3, 1e-2, 1e-1, 1.0, 1e+1, 1e+2]      # per-tensor scales of the real-valued draws
INT_ALPHA, REAL_ALPHA = [-2.0, 0.5, 1.0], [-1.7, 0.6, 1.3, -0.4]
# indices (ABI order of params[15]) of the gradients that are sums: conv_31_* (2..5), conv_13_* (6..9), alpha1 (14); the rest are copies or one multiply
CHAIN_IDX, ALPHA_IDX = range(2, 10), 14
# d conv_31[row, a] = sum_b g[3a+b] * c13[row, b] (and the transpose for conv_13): 3 products, each rounded once, added one after the other
# to s = 0 -> no term passes more than 4 roundings: k = number of terms + 1
CHAIN_K = 4


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ ADN-SSD: inputs and reference
@functools.lru_cache(maxsize=None)
def index_maps(di, gn, P):
    """the formulas of Mamba2._build_index_maps from (di, gn, P) alone -> (rows_in, perm_x, perm_xbc, cols_out)"""
    nh = di // P
    perm_x = torch.tensor([2 * ((h // 2) * P + p) + (h % 2) for h in range(nh) for p in range(P)])
    perm_b = torch.tensor([di + 2 * n + e for e in (0, 1) for n in range(gn // 2)])
    perm_xbc = torch.cat([perm_x, perm_b, perm_b + gn])
    rows_in = torch.cat([torch.arange(di), di + perm_xbc, torch.arange(2 * di + 2 * gn, 2 * di + 2 * gn + nh)])
    cols_out = torch.cat([perm_x, torch.arange(di, 2 * di)])
    return rows_in, perm_x, perm_xbc, cols_out


def adn_shapes(dm, di, gn, P):
    """-> (shapes of params[15] in ABI order, shapes of the five prepped tensors (w_in, taps, ln_w, ln_b, w_out))"""
    nh, cx, qx, qbc = di // P, di + 2 * gn, di // 4, gn // 2
    dinp = 2 * di + 2 * gn + nh
    chains = [qx, qbc, qx, qbc]   # x1, bc1, x2, bc2
    ps = [(dinp, dm), (cx // 2, 1, 3, 3)] + [(q, 1, 3, 1) for q in chains] + [(q, 1, 1, 3) for q in chains] + [(di, 1, 3, 3), (di,), (di,), (dm, 2 * di), ()]
    return ps, [(dinp, dm), (9, di + cx), (di,), (di,), (dm, 2 * di)]


def _distinct(shape, mod=None):
    """distinct integers per element, centred on 0 (reduced modulo `mod` when the tensor has more elements than that)"""
    n = math.prod(shape)
    mod = n if mod is None else min(mod, n)
    return (torch.arange(n, dtype=torch.int64) % mod - mod // 2).to(torch.float32).reshape(shape)


def adn_inputs(kind, dims, seed):
    """-> (params[15], cotangents[5]) as fp32 CPU tensors"""
    gen = torch.Generator().manual_seed(1000 * seed + 17 * dims[0] + dims[3])
    ps, os_ = adn_shapes(*dims)
    if kind == "int":
        ri = lambda lo, hi, s: torch.randint(lo, hi + 1, s, generator=gen).to(torch.float32)
        params = [ri(-3, 3, s) for s in ps]
        # the tensors that are only copied (or scaled by alpha1) hold distinct integers: a misplaced row / column / tap cannot coincide with the
        # right one.  in_proj.weight: below 2^20.  out_proj.weight also feeds d alpha1 = sum g * w with |g| <= 1: its values are reduced modulo an
        # odd M with numel * (M // 2) < 2^24, so that no partial sum in any order leaves the integers fp32 holds exactly (M = numel, all
        # distinct, at the four small shapes; M = 31 at the large one, where test_adnprep_single adds a run with distinct values and a zero
        # gradient of w_out, and the real-valued draws pin the permutation as well)
        n_out = math.prod(ps[13])
        params[0] = _distinct(ps[0], (1 << 20) - 3)
        params[13] = _distinct(ps[13], 2 * (((1 << 24) - 1) // n_out) + 1)
        for k in (1, 10, 11, 12):
            params[k] = _distinct(ps[k])
        params[14] = torch.tensor(INT_ALPHA[seed % 3])
        cots = [ri(-1, 1, s) for s in os_]
    else:
        rn = lambda s, k: torch.randn(s, generator=gen) * SCALES[(k + seed) % len(SCALES)]
        params = [rn(s, k) for k, s in enumerate(ps)]
        params[14] = torch.tensor(REAL_ALPHA[seed % 4])
        cots = [rn(s, k + 3) for k, s in enumerate(os_)]
    return params, cots


def adn_ref(p, dims):
    """the map in plain torch (Mamba2._rows_in / _perm_xbc / _cols_out / _effective_taps), in the dtype of `p`"""
    dm, di, gn, P = dims
    rows_in, perm_x, perm_xbc, cols_out = index_maps(di, gn, P)
    outer = lambda c31, c13: c31.reshape(-1, 3, 1) * c13.reshape(-1, 1, 3)
    k_oe = torch.cat([outer(p[2], p[6]), outer(p[3], p[7])], 0)
    k_oo = torch.cat([outer(p[4], p[8]), outer(p[5], p[9])], 0)
    k_odd = torch.stack((k_oe, k_oo), dim=1).reshape(-1, 3, 3)
    k_all = torch.stack((p[1].reshape(-1, 3, 3), k_odd), dim=1).reshape(-1, 3, 3)[perm_xbc]
    taps = torch.cat([p[10].reshape(-1, 9).t(), k_all.reshape(-1, 9).t()], 1)        # [conv2d_z taps | effective xBC taps]
    return p[0][rows_in], taps, p[11][perm_x], p[12][perm_x], p[14] * p[13][:, cols_out]


def _ref_run(fn, params, cots, dtype, absolute=False):
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    leaves = [f(t).to(dtype, copy=True).requires_grad_(True) for t in params]   # (a copy: the inputs themselves stay plain tensors)
    outs = fn(leaves)
    grads = torch.autograd.grad(outs, leaves, [f(c).to(dtype) for c in cots])
    return [o.detach() for o in outs], list(grads)


class Expect:
    """inputs and references of one case: fp64 (the truth), fp32 (the same copies / single multiplies in fp32 torch) and, for the bounds,
    the fp64 gradients of the map on |inputs| = sum|terms| of every gradient element (the map is a permutation with products)"""

    def __init__(self, fn, params, cots):
        self.params, self.cots = params, cots
        self.out64, self.g64 = _ref_run(fn, params, cots, torch.float64)
        self.out32, self.g32 = _ref_run(fn, params, cots, torch.float32)
        _, self.gabs = _ref_run(fn, params, cots, torch.float64, absolute=True)


@functools.lru_cache(maxsize=None)
def adn_expect(kind, dims, seed=0):
    params, cots = adn_inputs(kind, dims, seed)
    return Expect(lambda p: adn_ref(p, dims), params, cots)


# ---- the depth of d alpha1's summation tree, read off csrc/paramprep.hip and csrc/core.hip
def _adn_bwd_items(dm, di, gn, P):   # adn_items_bwd
    nh, cx = di // P, di + 2 * gn
    return (2 * di + 2 * gn + nh) * dm + (cx // 2) * 9 + 2 * 2 * (di // 4 + gn // 2) * 3 + 9 * di + 2 * di + dm * 2 * di


def blocks_single(dims):   # grid_for: 256 threads per block, at most kMaxBlocks = 1024
    return min(1024, max(1, _cdiv(_adn_bwd_items(*dims), 256)))


def blocks_multi(dims):    # multi_blocks: a quarter of the items, at most 512 per module
    return min(512, max(1, _cdiv(_adn_bwd_items(*dims) // 4 + 1, 256)))


def _fold_depth(rows):
    """adnm_launch_fold of `rows` partials into n = 1 column.  The thresholds below MIRROR fold_lc(rows, n) of csrc/core.hip for n = 1 (its
    `rows >= 1024 && n <= 64`, `rows >= 256 && n <= 2048` and `rows <= 4 / 8 / 16 / 32` lines): if that geometry changes, change this with
    it.  fold_rows_kernel then has kFoldThreads >> lc = 1024 >> lc row slices; a slice adds its ceil(rows / slices) partials one after the
    other (an upper bound: the unrolled form is shallower) and its second accumulator, then a binary tree over the slices."""
    if rows >= 1024:
        lc = 2
    elif rows >= 256:
        lc = 4
    else:
        lc = 10 if rows <= 4 else 9 if rows <= 8 else 8 if rows <= 16 else 7 if rows <= 32 else 6
    slices = 1024 >> lc
    return _cdiv(rows, slices) + 1 + int(math.log2(slices))


def _alpha_k(dims, nblk):
    """roundings a term g * w of d alpha1 can pass through.  A lane visits at most ceil(dm * di / 2 / (nblk * 256)) quads of out_proj.weight
    (its items lie nblk * 256 apart) and chains 4 fmas per quad: that many roundings; then wave_sum's 6 shuffle levels, 2 levels over the block's
    4 waves, the fold of the nblk block partials, and one for the reference's own cast"""
    dm, di = dims[0], dims[1]
    return 4 * _cdiv(dm * (di // 2), nblk * 256) + 6 + 2 + _fold_depth(nblk) + 1


def assert_equal(got, want, what):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}"
    if not torch.equal(got, want):
        bad = (got != want) | (got.isnan() != want.isnan())
        idx = bad.nonzero()[0].tolist() if bad.dim() else []
        pick = lambda t: float(t[tuple(idx)]) if idx else float(t)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {idx}: {pick(got)} vs {pick(want)}")


def assert_bounded(got, ref64, absterms, k, what):
    err = (got.detach().cpu().double() - ref64).abs()
    bound = k * EPS32 * absterms
    worst = float((err - bound).max())
    print(f"{what}: max |err| {float(err.max()):.3e}, bound there {float(bound.flatten()[int((err - bound).argmax())]):.3e} (k = {k})")
    assert worst <= 0.0, f"{what}: |err| exceeds k eps32 sum|terms| (k = {k}) by {worst:.3e}"


def check_adn(kind, dims, e, outs, grads, nblk, what):
    for k, name in enumerate(("w_in", "taps", "ln_w", "ln_b", "w_out")):
        assert_equal(outs[k], (e.out64[k].float() if kind == "int" else e.out32[k]), f"{what} {name}")
    for k in range(15):
        if kind == "int":
            assert_equal(grads[k], e.g64[k].float(), f"{what} dparams[{k}]")
        elif k in CHAIN_IDX:
            assert_bounded(grads[k], e.g64[k], e.gabs[k], CHAIN_K, f"{what} dparams[{k}]")
        elif k == ALPHA_IDX:
            assert_bounded(grads[k], e.g64[k], e.gabs[k], _alpha_k(dims, nblk), f"{what} d alpha1")
        else:
            assert_equal(grads[k], e.g32[k], f"{what} dparams[{k}]")


def run_adn_single(dims, e, cots=None):
    leaves = [p.to(DEV).requires_grad_(True) for p in e.params]
    outs = ops.adn_prep(*dims, leaves)
    grads = torch.autograd.grad(outs, leaves, [c.to(DEV) for c in (e.cots if cots is None else cots)])
    return outs, grads


# ------------------------------------------------------------------------------------------------ WTConv2d: inputs and reference
def wt_inputs(kind, shape, seed):
    """-> (params = [bias]? + (1 + levels) conv weights + (1 + levels) scales, cotangents = [gbias_t]? + (1 + levels) tap images)"""
    C, Cp, K, levels, has_bias = shape
    gen = torch.Generator().manual_seed(2000 * seed + 31 * C + K + levels)
    cg = [C] + [4 * C] * levels
    cgp = [Cp] + [4 * Cp] * levels
    if kind == "int":
        ri = lambda lo, hi, s: torch.randint(lo, hi + 1, s, generator=gen).to(torch.float32)
        bias = [ri(-3, 3, (C,))] if has_bias else []
        w = [_distinct((c, 1, K, K)) for c in cg]                                  # at most 280 * 25 values: ds = sum of 26 terms stays far below 2^24
        s = [2.0 ** ri(-2, 3, (1, c, 1, 1)) * (1 - 2 * ri(0, 1, (1, c, 1, 1))) for c in cg]   # powers of two, either sign
        cots = ([ri(-1, 1, (Cp,))] if has_bias else []) + [ri(-1, 1, (K * K, c)) for c in cgp]
    else:
        rn = lambda sh, k: torch.randn(sh, generator=gen) * SCALES[(k + seed) % len(SCALES)]
        bias = [rn((C,), 5)] if has_bias else []
        w = [rn((c, 1, K, K), k) for k, c in enumerate(cg)]
        s = [rn((1, c, 1, 1), k + 2) for k, c in enumerate(cg)]
        cots = ([rn((Cp,), 1)] if has_bias else []) + [rn((K * K, c), k + 4) for k, c in enumerate(cgp)]
    return bias + w + s, cots


def wt_ref(p, shape):
    C, Cp, K, levels, has_bias = shape
    p = list(p)
    bias = p.pop(0) if has_bias else None
    w, s = p[:1 + levels], p[1 + levels:]
    outs = []
    if has_bias:
        outs.append(torch.cat([bias * s[0].reshape(C), bias.new_zeros(Cp - C)]))
    for g in range(1 + levels):
        cg, cgp = (C, Cp) if g == 0 else (4 * C, 4 * Cp)
        t = (w[g].reshape(cg, K * K) * s[g].reshape(cg, 1)).t()
        outs.append(torch.cat([t, t.new_zeros(K * K, cgp - cg)], 1))
    return outs


@functools.lru_cache(maxsize=None)
def wt_expect(kind, shape, seed=0):
    params, cots = wt_inputs(kind, shape, seed)
    return Expect(lambda p: wt_ref(p, shape), params, cots)


def check_wt(kind, shape, e, outs, grads, what):
    C, Cp, K, levels, has_bias = shape
    nb = 1 if has_bias else 0
    for k, o in enumerate(outs):
        assert_equal(o, (e.out64[k].float() if kind == "int" else e.out32[k]), f"{what} out[{k}]")
        width = Cp if k < nb + 1 else 4 * Cp   # bias_t and the base taps are Cp wide, the level taps 4 Cp
        live = C if k < nb + 1 else 4 * C
        pad = o.detach()[..., live:width]
        assert float(pad.abs().sum()) == 0.0 and not bool(pad.isnan().any()), f"{what} out[{k}]: padded channels must be exactly 0"
    for k, g in enumerate(grads):
        if kind == "int":
            assert_equal(g, e.g64[k].float(), f"{what} grad[{k}]")
        elif k >= nb + 1 + levels:
            # ds[c] = sum over the K*K taps of g * w (+ g_bias * bias for the base conv): an fma chain from 0, one rounding per term;
            # k = K*K + 2 covers the K*K + 1 terms and the reference's cast
            assert_bounded(g, e.g64[k], e.gabs[k], K * K + 2, f"{what} ds[{k - nb - 1 - levels}]")
        else:
            assert_equal(g, e.g32[k], f"{what} grad[{k}]")   # dw = g * s, dbias = g * s: one multiply


def run_wt_single(shape, e):
    C, Cp, K, levels, has_bias = shape
    leaves = [p.to(DEV).requires_grad_(True) for p in e.params]
    nb = 1 if has_bias else 0
    bias_t, base, lv = ops.wt_prep(C, Cp, K, levels, leaves[0] if has_bias else None, leaves[nb:nb + 1 + levels], leaves[nb + 1 + levels:])
    outs = ([bias_t] if has_bias else []) + [base] + lv
    grads = torch.autograd.grad(outs, leaves, [c.to(DEV) for c in e.cots])
    return outs, grads


# ------------------------------------------------------------------------------------------------ single launches
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dims", ADN_SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_adnprep_single(dims, kind):
    e = adn_expect(kind, dims)
    outs, grads = run_adn_single(dims, e)
    check_adn(kind, dims, e, outs, grads, blocks_single(dims), f"adn_prep{dims} {kind}")
    if kind == "int" and len(e.params[13].unique()) < e.params[13].numel():
        # out_proj.weight had to be reduced modulo M for d alpha1's sake (the large shape): the same launches once more with DISTINCT
        # integers below 2^20 there and a zero gradient for w_out, so that d alpha1 is an exact 0 and no column can stand in for another
        params = list(e.params)
        params[13] = _distinct(e.params[13].shape, 1 << 20)
        cots = e.cots[:4] + [torch.zeros_like(e.cots[4])]
        e2 = Expect(lambda p: adn_ref(p, dims), params, cots)
        assert len(e2.params[13].unique()) == e2.params[13].numel()
        outs, grads = run_adn_single(dims, e2)
        check_adn(kind, dims, e2, outs, grads, blocks_single(dims), f"adn_prep{dims} int, distinct out_proj.weight")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", WT_SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_wtprep_single(shape, kind):
    e = wt_expect(kind, shape)
    outs, grads = run_wt_single(shape, e)
    check_wt(kind, shape, e, outs, grads, f"wt_prep{shape} {kind}")


def test_index_maps_match_mamba2():
    """the test's own builder against the buffers of a real module (two head widths, gn = 32 and 24)"""
    from models.ADNssd import Mamba2
    for kw in (dict(d_model=32, headdim=4), dict(d_model=48, headdim=12, ngroups=2, d_state=12)):
        m = Mamba2(**kw)
        rows_in, perm_x, perm_xbc, cols_out = index_maps(m.d_inner, m.ngroups * m.d_state, m.headdim)
        for mine, theirs in ((rows_in, m._rows_in), (perm_x, m._perm_x), (perm_xbc, m._perm_xbc), (cols_out, m._cols_out)):
            assert torch.equal(mine, theirs)
        # ... and the reference's tap builder against the module's
        dims, params = m.adnm_prep_args()
        with torch.no_grad():
            assert torch.equal(adn_ref([p.detach() for p in params], dims)[1][:, m.d_inner:], m._effective_taps())


# ------------------------------------------------------------------------------------------------ the C ABI's other forms
def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def test_adnprep_abi_forms():
    dims = dm, di, gn, P = (20, 40, 12, 4)
    cx = di + 2 * gn
    e = adn_expect("int", dims)
    ps, os_ = adn_shapes(*dims)
    params = [p.to(DEV) for p in e.params]
    taps_ref, gtaps = e.out64[1].float(), e.cots[1]
    ws_bytes = int(lib.query("adnm_adnprep_bwd_ws_bytes"))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)

    def forward(tap_ld, cw, czw):
        out = [_nan(*os_[0]), cw, czw, _nan(di), _nan(di), _nan(*os_[4])]
        lib.call("adnm_adnprep_fwd", lib.ptr_table(params), lib.ptr_table(out), dm, di, gn, P, tap_ld, _stream())
        for k, j in ((0, 0), (3, 2), (4, 3), (5, 4)):
            assert_equal(out[k], e.out64[j].float(), f"tap_ld={tap_ld} prepped[{k}]")

    def backward(tap_ld, gcw, gczw, nbytes=ws_bytes):
        gout = [e.cots[0].to(DEV), gcw, gczw, e.cots[2].to(DEV), e.cots[3].to(DEV), e.cots[4].to(DEV)]
        dparams = [_nan(*s) for s in ps]
        lib.call("adnm_adnprep_bwd", lib.ptr_table(params), lib.ptr_table(gout), lib.ptr_table(dparams), dm, di, gn, P, tap_ld, ws.data_ptr(), nbytes, _stream())
        for k in range(15):
            assert_equal(dparams[k], e.g64[k].float(), f"tap_ld={tap_ld} dparams[{k}]")

    # tap_ld = 0: two separate images at their own widths
    cw, czw = _nan(9, cx), _nan(9, di)
    forward(0, cw, czw)
    assert_equal(czw, taps_ref[:, :di].contiguous(), "tap_ld=0 czw")
    assert_equal(cw, taps_ref[:, di:].contiguous(), "tap_ld=0 cw")
    backward(0, gtaps[:, di:].contiguous().to(DEV), gtaps[:, :di].contiguous().to(DEV))
    # tap_ld beyond 2 di + 2 gn: the columns past the image keep what they held (forward) and are not read (backward)
    ld = di + cx + 12
    image = _nan(9, ld)
    forward(ld, image[:, di:], image)
    assert_equal(image[:, :di + cx].contiguous(), taps_ref, "wide tap_ld image")
    assert bool(image[:, di + cx:].isnan().all()), "columns beyond the tap image were written"
    gimage = _nan(9, ld)
    gimage[:, :di + cx] = gtaps.to(DEV)
    backward(ld, gimage[:, di:], gimage)

    # rejections: only the raised error; nothing is launched (the tables are nevertheless full-size and valid for every dimension tried)
    g0 = gtaps.to(DEV)
    with pytest.raises(RuntimeError, match=r"\(-3\).*workspace too small"):
        backward(di + cx, g0[:, di:], g0, nbytes=ws_bytes - 4)
    out = [_nan(*os_[0]), _nan(9, cx), _nan(9, di), _nan(di), _nan(di), _nan(*os_[4])]
    with pytest.raises(RuntimeError, match="tap_ld"):
        lib.call("adnm_adnprep_fwd", lib.ptr_table(params), lib.ptr_table(out), dm, di, gn, P, cx - 4, _stream())
    with pytest.raises(RuntimeError, match="tap_ld"):
        backward(cx - 4, g0[:, di:], g0)
    for bad in ((18, 40, 12, 4),    # dm % 4
                (20, 36, 12, 4),    # di % 8
                (20, 40, 10, 4),    # gn % 4
                (20, 40, 12, 8)):   # 5 heads
        with pytest.raises(RuntimeError, match="unsupported ADN-SSD dimensions"):
            lib.call("adnm_adnprep_fwd", lib.ptr_table(params), lib.ptr_table(out), *bad, 0, _stream())
        with pytest.raises(RuntimeError, match="unsupported ADN-SSD dimensions"):
            lib.call("adnm_adnprep_bwd", lib.ptr_table(params), lib.ptr_table([g0] * 6), lib.ptr_table([_nan(*s) for s in ps]), *bad, 0,
                     ws.data_ptr(), ws_bytes, _stream())
    torch.cuda.synchronize()
    assert all(bool(t.isnan().all()) for t in out), "a rejected call wrote something"


# ------------------------------------------------------------------------------------------------ grouped launches
S = ADN_SMALL
# 11 mixers: the four small shapes in mixed order, the large one at index 9 — in the second launch of the 8-module chunking (kMaxMulti)
ADN_GROUP = [S[0], S[2], S[1], S[3], S[1], S[0], S[3], S[2], S[2], ADN_BIG, S[1]]
# gradients handed over as None (AdnPrepMultiFn.backward zero-fills them): per module index, the prepped entries left out
ADN_NONE = {1: (1, 3), 4: (4,), 6: (0, 2), 10: (0, 1, 2, 3, 4)}


@pytest.mark.parametrize("kind", KINDS)
def test_adnprep_multi_equals_single(kind):
    # (seed 0 for the large one and each shape's first use: shared with test_adnprep_single's references)
    seen, es = {}, []
    for d in ADN_GROUP:
        es.append(adn_expect(kind, d, seen.get(d, 0)))
        seen[d] = seen.get(d, 0) + 1
    leaves = [[p.to(DEV).requires_grad_(True) for p in e.params] for e in es]
    out = ops.AdnPrepMultiFn.apply(list(ADN_GROUP), *[t for l in leaves for t in l])
    assert len(out) == 9 * len(ADN_GROUP) and all(t is None for i in range(len(es)) for t in out[9 * i + 5:9 * i + 9])
    used, cots = [], []
    for i, e in enumerate(es):
        for j in range(5):
            if j not in ADN_NONE.get(i, ()):
                used.append(out[9 * i + j])
                cots.append(e.cots[j].to(DEV))
    grads = torch.autograd.grad(used, [t for l in leaves for t in l], cots, allow_unused=False)
    for i, (d, e) in enumerate(zip(ADN_GROUP, es)):
        what = f"module {i} {d} {kind}"
        zc = [torch.zeros_like(c) if j in ADN_NONE.get(i, ()) else c for j, c in enumerate(e.cots)]   # the explicit zeros of the single call
        souts, sgrads = run_adn_single(d, e, zc)
        mg = grads[15 * i:15 * i + 15]
        for j in range(5):
            assert_equal(out[9 * i + j], souts[j], f"{what} prepped[{j}]")
        for k in range(15):
            if k == ALPHA_IDX and kind == "real" and 4 not in ADN_NONE.get(i, ()):
                # the block partition differs between the two launches: each within its own bound of the fp64 value (which depends on the
                # gradient of w_out alone; where that one is None both sums are over zeros and must agree exactly, below)
                assert_bounded(mg[k], e.g64[k], e.gabs[k], _alpha_k(d, blocks_multi(d)), f"{what} d alpha1 (grouped)")
                assert_bounded(sgrads[k], e.g64[k], e.gabs[k], _alpha_k(d, blocks_single(d)), f"{what} d alpha1 (single)")
            else:
                assert_equal(mg[k], sgrads[k], f"{what} dparams[{k}]")
        if i not in ADN_NONE:   # and against the reference itself (the large module's grouped launch is capped at 512 blocks)
            check_adn(kind, d, e, out[9 * i:9 * i + 5], mg, blocks_multi(d), what + " grouped")


WT_GROUP = [WT_SHAPES[k] for k in (0, 1, 2, 3, 4, 5, 3, 1, 5, 0, 2)]   # K = 3 and 5, bias and none, inside each of the two launches


@pytest.mark.parametrize("kind", KINDS)
def test_wtprep_multi_equals_single(kind):
    seen, es = {}, []
    for s in WT_GROUP:
        es.append(wt_expect(kind, s, seen.get(s, 0)))
        seen[s] = seen.get(s, 0) + 1
    leaves = [[p.to(DEV).requires_grad_(True) for p in e.params] for e in es]
    out = list(ops.WtPrepMultiFn.apply(list(WT_GROUP), *[t for l in leaves for t in l]))
    grads = list(torch.autograd.grad(out, [t for l in leaves for t in l], [c.to(DEV) for e in es for c in e.cots]))
    for i, (s, e) in enumerate(zip(WT_GROUP, es)):
        what = f"module {i} {s} {kind}"
        mo, mg = [out.pop(0) for _ in e.cots], [grads.pop(0) for _ in e.params]
        so, sg = run_wt_single(s, e)
        for k, (a, b) in enumerate(zip(mo, so)):
            assert_equal(a, b, f"{what} out[{k}]")
        for k, (a, b) in enumerate(zip(mg, sg)):
            assert_equal(a, b, f"{what} grad[{k}]")   # ds too: a channel's sum is one lane's chain in either launch
        check_wt(kind, s, e, mo, mg, what + " grouped")


# ------------------------------------------------------------------------------------------------ narrow copies of the two big matrices
def _narrow_call(dims, es, which, ndt, scales=None):
    """adnm_adnprep_fwd_multi with a narrow table.  which[i] = (w_in narrow?, w_out narrow?) -> per module (prepped[6], w_in_n, w_out_n, s_out_eff)"""
    dm, di, gn, P = dims
    cx = di + 2 * gn
    ps, os_ = adn_shapes(*dims)
    el = torch.bfloat16 if ndt == 1 else torch.uint8
    params, table, ntab, res = [], [], [], []
    for i, (e, (nin, nout)) in enumerate(zip(es, which)):
        params += [p.to(DEV) for p in e.params]
        taps = _nan(9, di + cx)
        pre = [None if nin else _nan(*os_[0]), taps[:, di:], taps[:, :di], _nan(di), _nan(di), None if nout else _nan(*os_[4])]
        w_in_n = torch.zeros(os_[0], dtype=el, device=DEV) if nin else None
        w_out_n = torch.zeros(os_[4], dtype=el, device=DEV) if nout else None
        s_in, s_out = scales[i] if ndt == 2 else (None, None)
        s_eff = _nan(1) if (ndt == 2 and nout) else None
        table += pre
        ntab += [w_in_n, w_out_n, s_in if nin else None, s_out if nout else None, s_eff]
        res.append((pre, taps, w_in_n, w_out_n, s_eff))
    lib.call("adnm_adnprep_fwd_multi", len(es), lib.ptr_table(params), lib.ptr_table(table), lib.i64_table([dm, di, gn, P, di + cx] * len(es)),
             lib.ptr_table(ntab), ndt, _stream())
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("dims", [ADN_SMALL[1], ADN_BIG], ids=lambda d: "x".join(map(str, d)))
def test_adnprep_narrow_copies(dims):
    es = [adn_expect("real", dims, 0), adn_expect("real", dims, 1)]        # alpha1 = -1.7 and 0.6
    assert float(es[0].params[14]) < 0 < float(es[1].params[14])
    bits16 = lambda t: t.view(torch.int16)

    def check_rest(e, pre, taps, nin, nout, what):
        assert_equal(taps, e.out32[1], what + " taps")
        assert_equal(pre[3], e.out32[2], what + " ln_w")
        assert_equal(pre[4], e.out32[3], what + " ln_b")
        if not nin:
            assert_equal(pre[0], e.out32[0], what + " fp32 w_in beside a narrow w_out")
        if not nout:
            assert_equal(pre[5], e.out32[4], what + " fp32 w_out beside a narrow w_in")

    # bf16: two calls, so that each module has both matrices narrow once and only one of them once
    for which in ([(True, True), (True, False)], [(False, True), (True, True)]):
        for i, ((pre, taps, w_in_n, w_out_n, _), (nin, nout)) in enumerate(zip(_narrow_call(dims, es, which, 1), which)):
            e, what = es[i], f"bf16 {which} module {i}"
            check_rest(e, pre, taps, nin, nout, what)
            if nin:
                assert_equal(bits16(w_in_n), bits16(e.out32[0].to(torch.bfloat16)), what + " w_in_n")
            if nout:
                assert_equal(bits16(w_out_n), bits16(e.out32[4].to(torch.bfloat16)), what + " w_out_n")   # out32[4] = alpha1 * out_proj.weight[:, cols_out] in fp32

    # fp8: scales that put the upper three quarters of each matrix's range beyond +-448 / s (saturation)
    scales = []
    for e in es:
        s_in = 448.0 / (0.25 * float(e.params[0].abs().max()))
        s_out = 448.0 / (0.25 * float(e.params[13].abs().max()))
        scales.append((torch.tensor([s_in], device=DEV), torch.tensor([s_out], device=DEV)))
    for which in ([(True, True), (False, True)], [(True, False), (True, True)]):
        for i, ((pre, taps, w_in_n, w_out_n, s_eff), (nin, nout)) in enumerate(zip(_narrow_call(dims, es, which, 2, scales), which)):
            e, what = es[i], f"fp8 {which} module {i}"
            check_rest(e, pre, taps, nin, nout, what)
            if nin:
                want = _e4m3_bytes(e.out32[0].to(DEV) * scales[i][0])
                assert int(((want & 0x7F) == 0x7E).sum()) > 0, "no element saturates: the case does not test the clamp"
                assert_equal(w_in_n, want, what + " w_in_n")
            if nout:
                expect = float(scales[i][1]) / abs(float(e.params[14]))
                assert abs(float(s_eff) - expect) <= 1e-6 * expect, f"{what}: s_out_eff {float(s_eff)} vs s_out / |alpha1| = {expect}"
                want = _e4m3_bytes(e.out32[4].to(DEV) * s_eff)
                assert int(((want & 0x7F) == 0x7E).sum()) > 0, "no element saturates: the case does not test the clamp"
                assert_equal(w_out_n, want, what + " w_out_n")
    # an fp8 copy without its scale pointers is rejected (nothing launched)
    for drop in (0, 1):
        bad = [tuple(None if k == drop else t for k, t in enumerate(sc)) for sc in scales]
        with pytest.raises(RuntimeError, match="scale pointers"):
            _narrow_call(dims, es, [(True, True), (True, True)], 2, bad)


@pytest.fixture
def bf16_mfma():
    ops.set_mfma_precision("bf16")
    yield
    ops.set_mfma_precision("f32")


def test_prep_group_hands_out_narrow_copies(bf16_mfma):
    """ops.prep_group in the bf16 mode: a projection too large for the tall-skinny kernel (N K > 8192) reaches its mixer as the bf16 copy plus a
    storage-less fp32 handle of its shape"""
    from models.ADNssd import Mamba2
    torch.manual_seed(5)
    mods = [Mamba2(d_model=48, headdim=4).to(DEV), Mamba2(d_model=64, headdim=4).to(DEV)]
    with torch.no_grad():
        mods[0].alpha1.fill_(-0.8)
        mods[1].alpha1.fill_(1.25)
    holder = torch.nn.ModuleList(mods)
    ops.prep_group(holder)
    for m in mods:
        pre = m.__dict__.pop("_adnm_prepped")
        dims, params = m.adnm_prep_args()
        dm, di, gn, P = dims
        n_in = 2 * di + 2 * gn + di // P
        assert n_in * dm > 8192 and dm * 2 * di > 8192
        assert len(pre) == 9
        w_in, taps, ln_w, ln_b, w_out, w_in_n, s_in, w_out_n, s_out = pre
        ref = adn_ref([p.detach().cpu() for p in params], dims)
        for h, shape in ((w_in, (n_in, dm)), (w_out, (dm, 2 * di))):
            assert tuple(h.shape) == shape and h.dtype == torch.float32 and h.requires_grad
            assert h.stride() == (0, 0) and h.untyped_storage().nbytes() == 4, "the fp32 entry of a narrow matrix is a handle without a matrix behind it"
        assert s_in is None and s_out is None
        assert w_in_n.dtype == torch.bfloat16 and w_out_n.dtype == torch.bfloat16 and not w_in_n.requires_grad and not w_out_n.requires_grad
        assert_equal(w_in_n.view(torch.int16), ref[0].to(torch.bfloat16).view(torch.int16), "prep_group w_in_n")
        assert_equal(w_out_n.view(torch.int16), ref[4].to(torch.bfloat16).view(torch.int16), "prep_group w_out_n")
        assert_equal(taps, ref[1], "prep_group taps")
        assert_equal(ln_w, ref[2], "prep_group ln_w")
        assert_equal(ln_b, ref[3], "prep_group ln_b")


# ------------------------------------------------------------------------------------------------ the product's grouped path, module level
def test_prep_group_matches_per_module(monkeypatch):
    """three mixers and two WTConv2d in a chain: one forward / backward with ops.prep_group, one with each module preparing itself"""
    from models.ADNssd import Mamba2
    from models.WTConv2d import WTConv2d
    torch.manual_seed(11)
    H = W = 12
    mods = [Mamba2(d_model=32, headdim=4), WTConv2d(32, 32, 5, 1, True, wt_levels=2), Mamba2(d_model=32, headdim=4),
            WTConv2d(32, 32, 3, 1, False, wt_levels=1), Mamba2(d_model=32, headdim=4)]
    net = torch.nn.ModuleList(mods).to(DEV)
    with torch.no_grad():
        for a, m in zip((0.7, -1.3, 1.9), (mods[0], mods[2], mods[4])):
            m.alpha1.fill_(a)
    gen = torch.Generator().manual_seed(3)
    u = torch.randn((2, H * W, 32), generator=gen).to(DEV)
    cot = torch.randn((2, H * W, 32), generator=gen).to(DEV)
    g_w_out, own_calls = {}, []
    real_adn_prep = ops.adn_prep

    def watched_adn_prep(dm, di, gn, P, params):
        """the module's own per-module call (Mamba2.forward), passed through unchanged; only the gradient that reaches w_out is recorded"""
        out = real_adn_prep(dm, di, gn, P, params)
        i = next(k for k, m in enumerate(mods) if isinstance(m, Mamba2) and m.alpha1 is params[14])
        out[4].register_hook(lambda g, i=i: g_w_out.__setitem__(i, g.detach().clone()))
        own_calls.append(i)
        return out

    monkeypatch.setattr(ops, "adn_prep", watched_adn_prep)

    def run(grouped):
        net.zero_grad(set_to_none=True)
        del own_calls[:]
        if grouped:
            ops.prep_group(net)
        x = u
        for m in mods:
            x = m(x, H, W) if isinstance(m, Mamba2) else m.forward_tokens(x, H, W)
        x.backward(cot)
        torch.cuda.synchronize()
        return x.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}, list(own_calls)

    y0, g0, calls0 = run(False)
    y1, g1, calls1 = run(True)
    assert calls0 == [0, 2, 4] and calls1 == [], "each mixer prepares itself without prep_group, and none does after it"
    assert_equal(y1, y0, "output")
    assert g0.keys() == g1.keys() and len(g0) >= 3 * 15 + 7 + 4   # at least every parameter that goes through the prep kernels
    for k in g0:
        if k.endswith("alpha1"):
            # d alpha1 = sum g_w_out * out_proj.weight[:, cols_out]: the two launches partition it differently, each is within its bound of the exact sum
            i = int(k.split(".")[0])
            m = mods[i]
            dims = m.adnm_prep_args()[0]
            terms = float((g_w_out[i].double() * m.out_proj.weight.detach().double()[:, m._cols_out]).abs().sum())
            bound = (_alpha_k(dims, blocks_single(dims)) + _alpha_k(dims, blocks_multi(dims))) * EPS32 * terms
            err = abs(float(g1[k]) - float(g0[k]))
            print(f"{k}: |grouped - single| {err:.3e}, bound {bound:.3e}")
            assert err <= bound, f"{k}: {float(g1[k])} vs {float(g0[k])}, bound {bound:.3e}"
        else:
            assert_equal(g1[k], g0[k], k)
