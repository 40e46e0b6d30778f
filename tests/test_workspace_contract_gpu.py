"""The workspace contract of the kernels: a launch stays inside the size its *_ws_bytes query names, and its fold / join reads no cell
that no workgroup wrote.

Every op that takes a scratch workspace runs twice on the same inputs (recipe.tensor): once as the suite runs it (ops._ws = torch.empty
from the caching allocator) and once under util.guarded_workspaces, where every workspace is a buffer of its own, filled — guards and
payload — with a payload NaN.  The guards must come back untouched and every output and gradient must be the first run's BIT FOR BIT and
free of NaN: the kernels are specified without atomics on floats and bitwise reproducible, and the other test files pin the first run
to the fp64 oracle, so one differing bit means the result depended on memory the launch did not write.  There is no tolerance in this file.

Shapes: for every op the smallest that reach each of its plans — one workgroup (one partial row); several with a ragged last one; just
past the cap on partial rows, where the fold is told the capped count.  The boundaries are read off the *_ws_bytes functions and the
launch code of csrc/ (noted at each table).  Every case prints one line `[ws-contract] op shape bytes calls verdict`
(profiles/workspace_contract.txt is that output of one run).

Left out: the branch of ops._skgemm that serves a stream capture nobody opened a scope for (the guard's allocator fills memory, which a
capture cannot hold); it hands the kernel the fenced layout that test_skgemm_fenced_workspace_called_directly passes in directly.

Found by this file and fixed with it: adnm_conv3_wgrad planned its partial rows without the bias sums where the query counts them, and at
the ~8 MB cap refused the workspace its own query had sized (the conv3 2x32x32x140x104 case); adnm_skgemm accepted a split shape's
workspace shorter than the query whenever its own precision's plan needed less."""
import ctypes

import pytest
import torch

from adnm_hip import lib, ops, recipe
from util import bits, guarded_workspaces, poison_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
NONE, SILU, GELU = lib.ACT_NONE, lib.ACT_SILU, lib.ACT_GELU
F32, BF16 = torch.float32, torch.bfloat16


def T(name, shape, scale=1.0):
    return recipe.tensor("wsc." + name, shape, scale)


def sc(v):
    return torch.tensor(float(v))


class Case:
    """one op at one shape.  ins: CPU tensors (None = absent operand), made once; f(*device leaves) -> tensor or tuple of tensors; every
    floating output gets a cotangent from recipe.tensor and every leaf's gradient is kept.  calls: the workspaces the op takes at least;
    patch: module attributes set for both runs; env: environment variables set for both runs; plan: asserted before the runs (the case
    reaches the plan it is in the table for)."""

    def __init__(self, op, shape, ins, f, calls=1, patch=(), env=(), plan=None, grad=True):
        self.op, self.shape, self.ins, self.f, self.calls, self.patch, self.env, self.plan, self.grad = op, shape, ins, f, calls, patch, env, plan, grad
        self.id = f"{op}-{'x'.join(str(s) for s in shape)}"
        self._made = None

    def make(self):
        if self._made is None:
            self._made = self.ins() if callable(self.ins) else self.ins
        return self._made

    def run(self):
        """-> [(name, tensor)]: outputs and gradients of one forward + backward on fresh device leaves"""
        leaves = [None if t is None else t.to(DEV).requires_grad_(self.grad and t.is_floating_point()) for t in self.make()]
        outs = self.f(*leaves)
        outs = [o for o in (outs if isinstance(outs, (tuple, list)) else (outs,)) if o is not None]
        res = [(f"out{i}", o.detach()) for i, o in enumerate(outs)]
        if self.grad:
            diff = [(i, o) for i, o in enumerate(outs) if o.requires_grad]
            cots = [T(f"{self.id}.cot{i}", tuple(o.shape)).to(DEV).to(o.dtype) for i, o in diff]
            torch.autograd.backward([o for _, o in diff], cots)
            res += [(f"grad{i}", l.grad) for i, l in enumerate(leaves) if l is not None and l.grad is not None]
            assert len(res) > len(outs), "no gradient came back"
        torch.cuda.synchronize()
        return res


def same_bits(a, b):
    if a.dtype in (F32, BF16):
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a.contiguous()), bits(b.contiguous()))
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def check_contract(monkeypatch, op, shape, run, calls):
    """steps 1-6 of the contract for run() -> [(name, tensor)]; prints the record line; -> the guard object"""
    plain = run()
    with guarded_workspaces(monkeypatch) as g:
        guarded = run()
        verdict, hit = "guards intact", None
        try:
            g.check()
        except AssertionError as e:
            verdict, hit = "GUARD HIT", e
    sizes = ",".join(str(r[2]) for r in g.records[:6]) + (",..." if g.calls > 6 else "")
    print(f"[ws-contract] {op:<18} {'x'.join(str(s) for s in shape):<28} bytes {sizes:<40} workspaces {g.calls:<4} {verdict}"
          f"   callers {sorted({r[3] for r in g.records})}")
    if hit is not None:
        raise hit
    assert [n for n, _ in plain] == [n for n, _ in guarded]
    for (name, a), (_, b) in zip(plain, guarded):
        assert not bool(torch.isnan(b.float()).any()), f"{op} {shape}: {name} holds a NaN under poisoned workspaces: a cell no workgroup wrote was read"
        assert same_bits(a, b), f"{op} {shape}: {name} differs between a plain and a poisoned workspace: the result depends on memory the launch did not write"
    assert g.calls >= calls, f"{op} {shape}: {g.calls} workspaces taken, the op takes {calls}: the guarded path was not the one meant"
    return g


# ================================================================================================ the cases
def _rownorm(M, d, mean, bias, affine):
    ins = lambda: [T(f"rn.x{M}.{d}", (M, d), 2.0), 1 + 0.2 * T(f"rn.w{d}", (d,)), 0.1 * T(f"rn.b{d}", (d,)) if bias else None,
                   sc(1.3) if affine else None, sc(-0.2) if affine else None]
    return Case("rownorm_bwd", (M, d, int(mean), int(bias), int(affine)), ins, lambda x, w, b, s, h: ops.rownorm(x, w, b, s, h, 1e-5, mean))


def _mixnorm(M, d, mean, gamma, affine):
    ins = lambda: [T(f"mn.a{M}.{d}", (M, d), 2.0), T(f"mn.b{M}.{d}", (M, d), 1.5), 1 + 0.2 * T(f"mn.w{d}", (d,)),
                   1 + 0.3 * T(f"mn.g{d}", (d,)) if gamma else None, torch.tensor([0.9]), torch.tensor([1.2]),
                   sc(1.3) if affine else None, sc(-0.2) if affine else None]
    return Case("mixnorm_bwd", (M, d, int(mean), int(gamma), int(affine)), ins,
                lambda x0, x1, w, g, s0, s1, s, h: ops.mixnorm([x0, x1], [s0, s1], g, w, None, s, h, 1e-5, mean))


def _lincomb(M, C, K, gamma):
    ins = lambda: ([T(f"lc.x{k}.{M}.{C}", (M, C)) for k in range(K)] + [None if (k == 0 and K > 1) else torch.tensor([0.7 + 0.3 * k]) for k in range(K)]
                   + [1 + 0.2 * T(f"lc.g{C}", (C,)) if gamma else None])
    return Case("lincomb_bwd", (M, C, K, int(gamma)), ins, lambda *a: ops.lincomb(list(a[:K]), list(a[K:2 * K]), a[2 * K]))


def _catmix(M, d, with_f):
    ins = lambda: [T(f"cm.{n}{M}.{d}", (2, M // 2, d)) for n in ("x", "r")] + [T(f"cm.f{M}.{d}", (2, M // 2, d)) if with_f else None] + \
                  [sc(1.1), sc(0.9)] + ([sc(0.7), sc(-0.4)] if with_f else [None, None])
    return Case("catmix_bwd", (M, d, int(with_f)), ins, lambda x, r, f, a1, a2, a3, a4: ops.catmix(x, r, f, a1, a2, a3, a4))


def _ssd_ins(tag, B, L, H, P, N, G):
    return lambda: [T(tag + "x", (B, L, H, P)), T(tag + "B", (B, L, G * N)), T(tag + "C", (B, L, G * N)), T(tag + "dt", (B, L, H), 2.0) - 3.0,
                    T(tag + "bias", (H,), 0.5), T(tag + "A", (H,), 1.0) + 1.0, 1 + 0.1 * T(tag + "D", (H,))]


def _ssd(B, L, H, P, N, G):
    return Case("ssd_reduce", (B, L, H, P, N, G), _ssd_ins(f"ssd{B}.{L}.{H}.", B, L, H, P, N, G), lambda *a: ops.ssd_reduce(*a, G), calls=2)


def _scan(B, L, H, N, G, chunk, reverse):
    return Case("ssd_scan", (B, L, H, N, G, chunk, int(reverse)), _ssd_ins(f"scan{B}.{L}.{H}.", B, L, H, 4, N, G),
                lambda *a: ops.ssd_scan(*a, G, chunk, reverse), calls=2)


def _dwconv(B, H, W, C, K, act, bias, dtype=F32):
    ins = lambda: [T(f"dw.x{H}.{W}.{C}", (B, H * W, C)).to(dtype), T(f"dw.w{C}.{K}", (C, 1, K, K), 0.5), T(f"dw.b{C}", (C,), 0.3) if bias else None]
    return Case("dwconv_bwd", (B, H, W, C, K, act, int(bias), "bf16" if dtype == BF16 else "f32"), ins, lambda x, w, b: ops.dwconv(x, w, b, H, W, act))


def _instnorm(B, HW, C, act):
    ins = lambda: [T(f"in.x{HW}.{C}", (B, HW, C), 2.0) + 3.0 * T(f"in.m{C}", (1, 1, C)), sc(0.9), sc(0.15)]
    return Case("instnorm", (B, HW, C, act), ins, lambda x, s, h: ops.instnorm(x, s, h, 1e-5, act), calls=2)


def _groupnorm(B, HW, C, G, act):
    ins = lambda: [T(f"gn.x{HW}.{C}", (B, HW, C), 2.0) + 3.0 * T(f"gn.m{C}", (1, 1, C)), 1 + 0.2 * T(f"gn.w{C}", (C,)), 0.1 * T(f"gn.b{C}", (C,)),
                   sc(0.9), sc(0.15)]
    return Case("groupnorm", (B, HW, C, G, act), ins, lambda x, w, b, s, h: ops.groupnorm(x, G, w, b, s, h, 1e-5, act), calls=2)


def _igate(shape, dtype=F32):
    ins = lambda: [T(f"ig.x{'.'.join(map(str, shape))}", shape, 2.0).to(dtype), sc(1.2), sc(0.15)]
    return Case("igate_bwd", shape + ("bf16" if dtype == BF16 else "f32",), ins, ops.igate)


def _igate_res(B, L, C, per_token):
    ins = lambda: [T(f"igr.x{B}.{L}.{C}", (B, L, C), 2.0), T(f"igr.r{B}.{L}.{C}", (B, L if per_token else 1, C)), sc(0.8), sc(1.2), sc(0.15)]
    return Case("igate_res_bwd", (B, L, C, per_token), ins, ops.igate_res)


def _skipgate(B, H, W, C):
    def ins():
        tag = f"sg{B}.{H}.{C}"
        shapes = [(C, 4, 1, 3), (C,), (C, 4, 3, 1), (C,), (C, 4, 3, 3), (C,), (C,), (C,), (C,), (C,)]
        p = [T(f"{tag}p{i}", s, 0.5 if len(s) > 1 else 0.3) for i, s in enumerate(shapes)]
        p[6], p[8] = 1 + p[6], 1 + p[8]
        p += [sc(v) for v in (1.3, 0.1, 0.8, -0.05, 0.33, 0.4, 0.27)] + [1 + 0.2 * T(tag + "g", (C,))]
        return [T(tag + "x", (B, H * W, C), 1.5)] + p
    return Case("skipgate_bwd", (B, H, W, C), ins, lambda x, *p: ops.skipgate(x, H, W, list(p)))


def _swish(n):
    return Case("swish_bwd", (n,), lambda: [T(f"sw.x{n}", (n,), 3.0), sc(1.3)], ops.swish)


def _bridge_pool(B, shapes):
    def f(*xs):
        al, att = ops.bridge_pool(list(xs))
        return (*al, att)
    return Case("bridge_pool", (B,) + tuple(v for s in shapes for v in s), lambda: [T(f"bp.x{i}.{L}.{C}", (B, L, C)) for i, (L, C) in enumerate(shapes)], f)


def _bridge_heads(B, Cs, S):
    n = len(Cs)
    ins = lambda: ([T(f"bh.a{B}.{S}", (B, 1, S)), sc(1.3), sc(0.1)] + [T(f"bh.w{i}.{c}.{S}", (c, S), 0.05) for i, c in enumerate(Cs)]
                   + [T(f"bh.b{i}.{c}", (c,), 0.1) for i, c in enumerate(Cs)])
    return Case("bridge_heads_bwd", (B, S) + tuple(Cs), ins, lambda a, e, t, *wb: tuple(ops.bridge_heads(a, e, t, list(wb[:n]), list(wb[n:]))))


def _colsum(rows, n):
    return Case("colsum", (rows, n), lambda: [T(f"cs.{rows}.{n}", (rows, n))], lambda t: ops.colsum(t), grad=False)


def _linear(M, K, N, bias, split_tn, fenced=False):
    """the short GEMMs: TN (the weight gradient) takes an ordinary workspace for its split-K partials; the split NT / NN launches of a shape
    take theirs from ops.SPLITWS (uncached slabs, tests/test_kernels_gpu.py) unless ADNM_SK_UC_SLABS=0 sends the fenced protocol through
    ops._ws as well (`fenced`: the wrapper zeroes that workspace, so only its guards and the result speak there)"""
    ins = lambda: [T(f"sk.x{M}.{K}", (M, K)), T(f"sk.w{N}.{K}", (N, K), 0.05), T(f"sk.b{N}", (N,)) if bias else None]
    nsplit = sum(lib.query("adnm_skgemm_ws_bytes", op, M, N, K) > 16 for op in (ops.SK_NT, ops.SK_NN))

    def plan():
        assert not ops.ts_ok_tn(M, N, K, torch.empty((1, 4), device=DEV)) and (lib.query("adnm_skgemm_ws_bytes", ops.SK_TN, M, N, K) > 16) == split_tn
        assert not fenced or nsplit > 0
    return Case("linear_skgemm" + ("_fenced" if fenced else ""), (M, K, N, int(bias)), ins, ops.linear, calls=1 + (nsplit if fenced else 0),
                env=(("ADNM_SK_UC_SLABS", "0"),) if fenced else (), plan=plan)


def _linear_ts(M, K, N, bias):
    """the tall-skinny weight gradient (adnm_tsgemm_tn): per-workgroup partial matrices + the shared fold.  It takes M >= ops.TS_MIN_ROWS token
    rows; the constant is lowered for the small cases (tools/kbench_ts.py lowers it through the environment before the import)"""
    ins = lambda: [T(f"ts.x{M}.{K}", (M, K)), T(f"ts.w{N}.{K}", (N, K), 0.3), T(f"ts.b{N}", (N,), 0.2) if bias else None]
    return Case("linear_tsgemm_tn", (M, K, N, int(bias)), ins, ops.linear, patch=((ops, "TS_MIN_ROWS", 64),),
                plan=lambda: (lambda x: ops.ts_ok_tn(M, N, K, x) or pytest.fail("not a tall-skinny shape"))(torch.empty((1, 4), device=DEV)))


def _conv3(B, H, W, K, N, act, bias, cl, split):
    def ins():
        w = T(f"c3.w{N}.{K}", (N, K, 3, 3), 0.2)
        if cl:   # (Cout, 3, 3, Cin) memory order behind the logical (Cout, Cin, 3, 3) shape
            w = w.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        return [T(f"c3.x{H}.{W}.{K}", (B, H * W, K)), w, T(f"c3.b{N}", (N,)) if bias else None]

    def f(x, w, b):
        if cl:   # .to(device) keeps the strides of a dense permuted tensor
            assert w.stride() == (9 * K, 1, 3 * K, K)
        return ops.conv3(x, w, b, H, W, act)

    def plan():
        assert (lib.query("adnm_conv3_ws_bytes", B, H, W, K, N) > 16, lib.query("adnm_conv3_ws_bytes", B, H, W, N, K) > 16) == split   # (forward, dgrad)
    return Case("conv3", (B, H, W, K, N, act, int(bias), int(cl)), ins, f, calls=3, plan=plan)


def _convt2x(B, H, W, C, cl):
    def ins():
        w = T(f"ct.w{C}", (C, C, 3, 3), 0.2)
        if cl:
            w = w.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        return [T(f"ct.x{H}.{W}.{C}", (B, H * W, C)), w, T(f"ct.b{C}", (C,))]
    return Case("convt2x", (B, H, W, C, int(cl)), ins, lambda x, w, b: ops.convt2x(x, w, b, H, W), calls=2)   # its TN GEMM and the bias colsum


def _adn_shapes(dm, di, gn, P):
    """shapes of the 15 reference-layout parameters of an ADN-SSD mixer in ABI order (include/adnm_hip.h: adnm_adnprep_fwd)"""
    nh, cx, qx, qbc = di // P, di + 2 * gn, di // 4, gn // 2
    chains = [qx, qbc, qx, qbc]
    return [(2 * di + 2 * gn + nh, dm), (cx // 2, 1, 3, 3)] + [(q, 1, 3, 1) for q in chains] + [(q, 1, 1, 3) for q in chains] + \
           [(di, 1, 3, 3), (di,), (di,), (dm, 2 * di), ()]


def _adn_prep(dims):
    ins = lambda: [T(f"ap.{'.'.join(map(str, dims))}.{k}", s, 0.5) for k, s in enumerate(_adn_shapes(*dims))]
    return Case("adn_prep_bwd", dims, ins, lambda *p: ops.adn_prep(*dims, list(p)))


def _adn_prep_multi(group):
    ins = lambda: [T(f"apm{i}.{'.'.join(map(str, d))}.{k}", s, 0.5) for i, d in enumerate(group) for k, s in enumerate(_adn_shapes(*d))]

    def f(*p):
        out = ops.AdnPrepMultiFn.apply(list(group), *p)
        return tuple(out[9 * i + j] for i in range(len(group)) for j in range(5))
    return Case("adn_prep_bwd_multi", (len(group),) + tuple(group[-1]), ins, f)


def _rainloss(n):
    tgt = lambda: T(f"rl.t{n}", (n,), 0.3).abs().to(DEV)
    return Case("rainloss", (n,), lambda: [T(f"rl.p{n}", (n,), 0.3).abs()], lambda p: ops.rainloss(p, tgt(), 0.57, 0.25, 0.0))


def _pool_counts(frames, H, W, pools):
    ins = lambda: [T(f"pc.t{frames}.{H}.{W}", (frames, H, W), 1.2), T(f"pc.p{frames}.{H}.{W}", (frames, H, W), 1.2)]
    return Case("pool_counts", (frames, H, W) + tuple(v for p in ops.pool_pairs(pools) for v in p), ins,
                lambda t, p: ops.pool_counts(t, p, [20, 30, 35, 40], 255.0, pools), grad=False)


ADN_BIG = (512, 1024, 16, 64)   # > 1024 x 256 items: the single launch's capped grid; > 512 blocks: the grouped launch's per-module cap
CASES = [
    # row kernels: kBlock / lanes_per_row(d) rows per workgroup (32 at d = 32, 4 from d = 256 on), at most kMaxPartBlocks = 1024 partial rows
    _rownorm(3, 32, True, True, True), _rownorm(1000, 32, False, False, True), _rownorm(5, 260, False, False, True), _rownorm(37, 48, True, True, False),
    _rownorm(32768, 32, True, False, True), _rownorm(32800, 32, False, True, True),
    _mixnorm(3, 32, True, True, True), _mixnorm(1000, 32, False, False, True), _mixnorm(131, 1024, True, True, False), _mixnorm(32800, 32, True, True, True),
    _lincomb(3, 32, 2, True), _lincomb(1000, 32, 1, True), _lincomb(7, 2048, 2, False), _lincomb(32800, 32, 3, True),
    # catmix: cdiv(M d / 4, 256) workgroups, at most 1024 (M d / 4 > 262144)
    _catmix(4, 64, True), _catmix(300, 64, False), _catmix(8192, 128, False), _catmix(8200, 128, True),
    # K1: [head statistics per (sample, token chunk) | B / C partials per head block (H P > 64) | ...]: one chunk, ragged chunks, 8 head blocks
    _ssd(3, 1, 4, 4, 8, 4), _ssd(1, 70, 12, 4, 16, 2), _ssd(2, 300, 16, 4, 16, 2), _ssd(2, 16, 512, 4, 16, 2), _ssd(1, 33, 24, 8, 8, 1),
    # K1b: L below, equal to and ragged against the chunk, both directions, N = 8 and 16
    _scan(1, 33, 2, 16, 2, 64, False), _scan(2, 64, 32, 8, 2, 64, True), _scan(2, 70, 8, 8, 2, 16, False), _scan(2, 70, 8, 8, 2, 16, True),
    _scan(1, 257, 4, 16, 1, 64, False),
    # depthwise conv backward + tap gradient: one workspace, sized for the larger of the fp32 / bf16 (8 channels per lane) / 5x5 column-walker
    # geometries; odd H / W, one partial row and many, both storage types
    _dwconv(1, 1, 1, 4, 3, SILU, True), _dwconv(1, 7, 9, 8, 3, NONE, True), _dwconv(2, 10, 14, 32, 5, NONE, False), _dwconv(1, 5, 3, 12, 5, GELU, True),
    _dwconv(1, 131, 130, 24, 3, NONE, True), _dwconv(3, 128, 129, 8, 3, GELU, False), _dwconv(2, 4, 4, 4096, 3, NONE, True),
    _dwconv(2, 16, 16, 32, 3, SILU, False, BF16), _dwconv(1, 9, 11, 16, 5, GELU, True, BF16), _dwconv(1, 131, 130, 24, 3, NONE, True, BF16),
    _dwconv(2, 10, 14, 32, 5, NONE, False, BF16),
    # InstanceNorm / GroupNorm: nchunk = cdiv(HW, 8 * 256 / cgb) pixel chunks, at most 128 (HW > 32768 at C = 32); gx > 1 channel blocks at C = 1024
    _instnorm(3, 77, 12, GELU), _instnorm(2, 300, 36, NONE), _instnorm(2, 1024, 64, GELU), _instnorm(2, 16, 1024, NONE), _instnorm(1, 33001, 32, NONE),
    _groupnorm(3, 77, 12, 3, GELU), _groupnorm(2, 300, 36, 1, NONE), _groupnorm(2, 1024, 64, 4, GELU), _groupnorm(2, 16, 1024, 32, NONE),
    _groupnorm(1, 33001, 32, 2, NONE),
    # gates: igate n / 4 / 256 + 1 workgroups, at most 512; igate_res B * cdiv(C / 4, 16); swish cdiv(n / 4, 1024), at most 1024
    _igate((100, 4)), _igate((3, 100, 64)), _igate((4 * 256 * 512 - 4,)), _igate((4 * 256 * 512 + 4,)), _igate((3, 100, 64), BF16),
    _igate_res(2, 77, 36, 0), _igate_res(4, 16, 1024, 0), _igate_res(1, 4096, 32, 0), _igate_res(2, 64, 16, 1), _igate_res(3, 5, 260, 1),
    _skipgate(3, 5, 5, 36), _skipgate(2, 4, 4, 256), _skipgate(2, 9, 7, 64), _skipgate(1, 40, 40, 256),
    _swish(400), _swish(20004), _swish(4 * 1024 * 1024), _swish(4 * 1024 * 1024 + 4),
    # bridge: 64 token slices per (sample, channel); heads: total / 512 rows per workgroup, a batch above 8 goes through in row chunks that
    # share the one workspace
    _bridge_pool(3, [(33, 8), (5, 4), (1, 12)]), _bridge_pool(2, [(700, 64)]), _bridge_pool(4, [(1024, 128), (256, 256), (64, 512), (4, 1024)]),
    _bridge_heads(7, [36, 20], 2144), _bridge_heads(2, [32, 64, 128, 128, 256, 512, 1024], 2144), _bridge_heads(19, [36, 20], 2144),
    _bridge_heads(16, [256, 512, 1024], 2144),
    # colsum: no bands below kColsumMinRows = 2048 rows, then rows / 256 bands, at most 256
    _colsum(2047, 32), _colsum(2048, 32), _colsum(5000, 257), _colsum(65535, 4), _colsum(65536 + 256, 32),
    # linear: (M, K, N).  TN unsplit / split; NT and NN split through the fenced protocol; the tall-skinny TN with 1, 17 and the capped 256 workgroups
    _linear(1024, 256, 1216, True, False), _linear(100, 48, 36, True, True), _linear(300, 20, 64, False, True), _linear(64, 2048, 1024, True, False),
    _linear(64, 4096, 1024, False, False, fenced=True), _linear(4, 2144, 256, True, False, fenced=True),
    _linear_ts(100, 32, 32, True), _linear_ts(4099, 48, 40, True), _linear_ts(65536 + 260, 32, 32, False),
    # conv3: deep maps split the reduction (partials + join), shallow ones do not — forward and input gradient each by its own channel counts
    # (the last argument); the weight gradient always takes partial rows
    _conv3(2, 4, 4, 256, 256, GELU, True, True, (True, True)), _conv3(2, 8, 8, 256, 64, NONE, True, True, (True, True)), _conv3(1, 4, 4, 64, 128, NONE, True, False, (True, True)),
    _conv3(2, 12, 12, 16, 24, GELU, True, False, (False, False)), _conv3(2, 7, 9, 8, 12, GELU, True, False, (False, False)), _conv3(1, 32, 32, 32, 200, NONE, True, True, (False, True)),
    # no bias, 9 N K between 8 MB / 16 and 8 MB / 16 - N floats: the launch once planned 16 partial rows where the query (rows with the bias
    # sums) sized 15, and refused the queried workspace
    _conv3(2, 32, 32, 140, 104, NONE, False, False, (True, True)),
    _convt2x(2, 4, 4, 64, True), _convt2x(2, 6, 10, 16, True), _convt2x(1, 16, 16, 32, False),
    # parameter prep: the single launch (grid capped at 1024) and the grouped one (512 per module, 8 modules per launch)
    _adn_prep((8, 8, 4, 4)), _adn_prep((36, 72, 20, 12)), _adn_prep(ADN_BIG),
    _adn_prep_multi([(8, 8, 4, 4), (20, 40, 12, 4)]), _adn_prep_multi([(8, 8, 4, 4)] * 8 + [(36, 72, 20, 12), ADN_BIG]),
    # loss: cdiv(n, 1024) workgroups, at most 1024
    _rainloss(100), _rainloss(5001), _rainloss(1024 * 1024), _rainloss(1024 * 1024 + 4),
    _pool_counts(6, 37, 53, ((4, 2), (16, 8), (3, 2), (1, 1))), _pool_counts(8, 64, 64, (4, 16)), _pool_counts(1, 16, 16, (16,)),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_workspace_contract(case, monkeypatch):
    for obj, name, value in case.patch:
        monkeypatch.setattr(obj, name, value)
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    if case.plan is not None:
        case.plan()
    check_contract(monkeypatch, case.op, case.shape, case.run, case.calls)


def test_case_ids_are_unique():
    assert len({c.id for c in CASES}) == len(CASES)


# ================================================================================================ 3. the split GEMM's fenced layout, called directly
def _poisoned(shape):
    t = torch.empty(shape, dtype=F32, device=DEV)
    bits(t).fill_(poison_bits(F32))
    return t


@pytest.mark.parametrize("op", ["nt", "nn"])
@pytest.mark.parametrize("M,K,N", [(64, 4096, 1024), (4, 2144, 256)])
def test_skgemm_fenced_workspace_called_directly(M, K, N, op, monkeypatch):
    """adnm_skgemm with slabs_uc = NULL and ws = [arrival counters, zeroed | slabs, poisoned] of exactly adnm_skgemm_ws_bytes between guards (the
    wrapper zeroes its whole fenced workspace, which would erase the poison): the result is bitwise ops.k_linear / k_linear_dx, the guards
    are intact, every counter is zero again (the header's promise); 4 bytes less are refused before anything is launched."""
    code = ops.SK_NT if op == "nt" else ops.SK_NN
    a = T(f"skd.a{op}{M}", (M, K if op == "nt" else N)).to(DEV)
    w = T(f"skd.w{N}.{K}", (N, K), 0.05).to(DEV)
    nb, cb = lib.query("adnm_skgemm_ws_bytes", code, M, N, K), lib.query("adnm_skgemm_counter_bytes", code, M, N, K)
    if nb <= 16:   # (4, 2144, 256) splits forward only: its input gradient takes no workspace
        assert op == "nn" and (M, K, N) == (4, 2144, 256)
        return
    assert 0 < cb < nb and cb % 256 == 0
    want = ops.k_linear(a, w, None) if op == "nt" else ops.k_linear_dx(a, w)
    stream = torch.cuda.current_stream().cuda_stream

    def call(ws, nbytes, c):
        return lib.load().adnm_skgemm(code, a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), 0, None, None, c.data_ptr(), c.stride(0), None,
                                      ws.data_ptr(), nbytes, None, 0, M, N, K, 0, None, stream)
    with guarded_workspaces(monkeypatch) as g:
        ws = g.alloc(nb, DEV)
        assert ws.numel() == nb and ws.data_ptr() % 256 == 0
        ws[:cb].zero_()
        c = _poisoned(tuple(want.shape))
        rc = call(ws, nb, c)
        assert rc == 0, lib.last_error()
        g.check()
        assert torch.equal(bits(c), bits(want)) and not bool(torch.isnan(c).any()), "the fenced protocol on a poisoned workspace differs from the wrapper's result"
        assert int(ws[:cb].view(torch.int32).abs().max()) == 0, "a split launch left an arrival counter behind"
        # 4 bytes short: refused by the library's own check, nothing written
        ws2 = g.alloc(nb, DEV)
        ws2[:cb].zero_()
        c2 = _poisoned(tuple(want.shape))
        rc = call(ws2, nb - 4, c2)
        torch.cuda.synchronize()
        assert rc != 0 and "workspace" in lib.last_error(), (rc, lib.last_error())
        assert bool((bits(c2) == poison_bits(F32)).all()), "a refused call wrote its output"
        assert bool((ws2[cb:].view(torch.int32) == poison_bits(F32)).all()), "a refused call wrote its workspace"
        g.check()


# ================================================================================================ 4. entry points that do not go through ops._ws
def _eval(alloc, t, p, thr, scale):
    """adnm_eval_counts / adnm_eval_ssim as GpuEvaluator.evaluate calls them, the workspaces from alloc(nbytes)"""
    B, Tn, H, W = t.shape
    stream = torch.cuda.current_stream().cuda_stream
    thr_c = (ctypes.c_float * len(thr))(*thr)
    out = torch.empty((B, Tn, 4 * len(thr) + 2), dtype=F32, device=DEV)
    nb = lib.query("adnm_eval_counts_ws_bytes", B * Tn, H * W, len(thr))
    ws = alloc(nb)
    lib.call("adnm_eval_counts", t.data_ptr(), p.data_ptr(), out.data_ptr(), thr_c, len(thr), scale, ws.data_ptr(), nb, B * Tn, H * W, stream)
    ssim = torch.empty((B, Tn), dtype=F32, device=DEV)
    nb2 = lib.query("adnm_eval_ssim_ws_bytes", B * Tn, H, W)
    ws2 = alloc(nb2)
    lib.call("adnm_eval_ssim", t.data_ptr(), p.data_ptr(), ssim.data_ptr(), scale, ws2.data_ptr(), nb2, B * Tn, H, W, stream)
    torch.cuda.synchronize()
    return [("counts", out), ("ssim", ssim)]


def _valid(alloc, pred, tgt, thr, scale, pools):
    """adnm_valid_accum / adnm_valid_ssim_accum / adnm_valid_pool_accum as Validator._launch calls them, twice (the block accumulates)"""
    B, Tn, H, W = pred.shape
    stream = torch.cuda.current_stream().cuda_stream
    thr_c = (ctypes.c_float * len(thr))(*thr)
    block = torch.zeros(lib.query("adnm_valid_block_bytes", Tn, len(thr)) // 8, dtype=torch.float64, device=DEV)
    table = torch.zeros(lib.query("adnm_valid_pool_block_bytes", Tn, len(thr), len(pools)) // 8, dtype=torch.float64, device=DEV)
    loss = torch.zeros((), dtype=F32, device=DEV)
    tab = ops.pool_table(pools)
    for _ in range(2):
        nb = lib.query("adnm_valid_accum_ws_bytes", B * Tn, Tn, H * W, len(thr))
        ws = alloc(nb)
        lib.call("adnm_valid_accum", pred.data_ptr(), tgt.data_ptr(), block.data_ptr(), loss.data_ptr(), thr_c, len(thr), scale, 0.57, 0.25, 0.0,
                 ws.data_ptr(), nb, B * Tn, Tn, H * W, stream)
        nb2 = lib.query("adnm_valid_ssim_accum_ws_bytes", B * Tn, Tn, H, W, len(thr))
        ws2 = alloc(nb2)
        lib.call("adnm_valid_ssim_accum", pred.data_ptr(), tgt.data_ptr(), block.data_ptr(), len(thr), scale, ws2.data_ptr(), nb2, B * Tn, Tn, H, W, stream)
        nb3 = lib.query("adnm_valid_pool_accum_ws_bytes", B * Tn, Tn, H, W, len(thr), tab, len(pools))
        assert nb3 > 0
        ws3 = alloc(nb3)
        lib.call("adnm_valid_pool_accum", pred.data_ptr(), Tn * H * W, H * W, tgt.data_ptr(), table.data_ptr(), thr_c, len(thr), scale, tab, len(pools),
                 ws3.data_ptr(), nb3, B * Tn, Tn, H, W, stream)
    torch.cuda.synchronize()
    return [("block", block), ("table", table), ("loss", loss)]


def _adamw(alloc):
    """adnm_adamw_step as tests/test_kernels_gpu.py::test_adamw_writes_the_shadows sets it up (no shadow), two steps"""
    n_t = [4096, 12, 70000, 4, 1024 * 33]
    offs, total = [], 0
    for k in n_t:
        offs.append(total)
        total += (k + 3) // 4 * 4
    g, p = T("aw.g", (total,), 0.01).to(DEV), T("aw.p", (total,), 0.3).to(DEV)
    m, v, state = torch.zeros(total, device=DEV), torch.zeros(total, device=DEV), torch.zeros(4, device=DEV)
    seg_end = torch.tensor([o // 4 for o in offs[1:]] + [total // 4], dtype=torch.int32, device=DEV)
    seg_rec = torch.tensor([0, -1, 2, -1, 4], dtype=torch.int32, device=DEV)
    nb = lib.query("adnm_adamw_ws_bytes")
    for _ in range(2):
        ws = alloc(nb)
        lib.call("adnm_adamw_step", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), total, state.data_ptr(), 1e-3, 0.9, 0.999, 1e-9, 1e-2, 0.05,
                 ws.data_ptr(), nb, None, 0, seg_end.data_ptr(), seg_rec.data_ptr(), 5, None, None, torch.cuda.current_stream().cuda_stream)
    # adnm_step_guard (the monitored step's norm + statistics pass) folds its partial norms through the same workspace
    stats = torch.zeros(9, dtype=torch.float64, device=DEV)   # (tests/test_step_guard_gpu.py: Bufs)
    ws = alloc(nb)
    lib.call("adnm_step_guard", g.data_ptr(), total, state.data_ptr(), 0.05, None, ws.data_ptr(), nb, stats.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [("p", p), ("m", m), ("v", v), ("state", state), ("stats", stats)]


def _fields(shape):
    name = "wsc.valid." + "x".join(map(str, shape))
    return recipe.tensor(name + ".pred", shape, scale=1.2).to(DEV), recipe.tensor(name + ".tgt", shape, scale=1.2).to(DEV)


DIRECT = {
    "eval-3x5x11x11": lambda al: _eval(al, *_fields((3, 5, 11, 11)), [20.0, 30.0, 35.0, 40.0], 255.0),          # hw = 121, one SSIM window
    "eval-2x3x17x19": lambda al: _eval(al, *_fields((2, 3, 17, 19)), [30.0], 255.0),                            # hw no multiple of 4
    "eval-2x20x64x64": lambda al: _eval(al, *_fields((2, 20, 64, 64)), [5.0, 10, 20, 30, 35, 40, 50, 70], 255.0),   # 16 SSIM tiles per frame
    "valid-3x5x11x11": lambda al: _valid(al, *_fields((3, 5, 11, 11)), [20.0, 30.0, 35.0, 40.0], 255.0, ((4, 2), (1, 1))),
    "valid-2x3x17x19": lambda al: _valid(al, *_fields((2, 3, 17, 19)), [30.0], 255.0, ((16, 8), (3, 2))),
    "valid-2x20x64x64": lambda al: _valid(al, *_fields((2, 20, 64, 64)), [20.0, 30.0, 35.0, 40.0], 255.0, ((4, 4), (16, 16))),
    "adamw": _adamw,
}


@pytest.mark.parametrize("name", list(DIRECT))
def test_direct_entry_points_keep_the_contract(name, monkeypatch):
    """the entry points whose callers allocate for themselves (GpuEvaluator, Validator, FlatTrainer): exact queried size, guards, poison, and a
    result bitwise that of the existing path (torch.empty of the queried size, at least 16 bytes)"""
    run = DIRECT[name]
    plain = run(lambda n: torch.empty(max(int(n), 16), dtype=torch.uint8, device=DEV))
    with guarded_workspaces(monkeypatch) as g:
        got = run(lambda n: g.alloc(n, DEV, caller=name))
        g.check()
    print(f"[ws-contract] {'direct:' + name:<47} bytes {','.join(str(r[2]) for r in g.records[:6]):<40} workspaces {g.calls:<4} guards intact")
    for (what, a), (_, b) in zip(plain, got):
        assert not bool(torch.isnan(b.float()).any()), f"{name}: {what} holds a NaN under a poisoned workspace"
        assert same_bits(a, b), f"{name}: {what} differs between a plain and a poisoned workspace"
    assert g.calls >= 2


# ================================================================================================ 5. undersized workspaces are refused
class _Launches:
    """with _Launches() as ev: ... -> ev.count = launches the library's opt-in profiler saw (include/adnm_hip.h, adnm_prof_*), by scope"""

    def _collect(self):
        buf = ctypes.create_string_buffer(1 << 20)
        lib.query("adnm_prof_collect", buf, len(buf))   # (collecting also clears the records)
        count = {}
        for line in buf.value.decode().splitlines():
            name, cnt = line.split("\t")[:2]
            count[name.split("@")[0]] = count.get(name.split("@")[0], 0) + int(cnt)
        return count

    def __enter__(self):
        torch.cuda.synchronize()
        self._collect()
        self.count = {}
        lib.query("adnm_prof_enable", 1)
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        lib.query("adnm_prof_enable", 0)
        self.count = self._collect()
        return False


def _fwd_only(case):
    """the forward itself takes the workspace: the call under test is the whole forward"""
    leaves = [None if t is None else t.to(DEV) for t in case.make()]
    return lambda: case.f(*leaves)


def _bwd_only(case, only=None):
    """the backward node takes it: the forward runs before the query is shortened.  only: the leaves that ask for a gradient (so that the
    node's first launch is the one with the workspace)"""
    leaves = [None if t is None else t.to(DEV).requires_grad_(t.is_floating_point() and (only is None or i in only)) for i, t in enumerate(case.make())]
    outs = case.f(*leaves)
    outs = [o for o in (outs if isinstance(outs, (tuple, list)) else (outs,)) if o is not None and o.requires_grad]
    cots = [torch.ones_like(o) for o in outs]
    torch.cuda.synchronize()
    return lambda: torch.autograd.backward(outs, cots)


# wrappers that hand the queried size straight through as ws_bytes, each at a shape whose workspace is above 16 bytes
SHORT = [
    (_rownorm(1000, 32, False, False, True), _bwd_only), (_mixnorm(1000, 32, False, False, True), _bwd_only), (_lincomb(1000, 32, 1, True), _bwd_only),
    (_catmix(300, 64, False), _bwd_only), (_ssd(1, 70, 12, 4, 16, 2), _fwd_only), (_ssd(1, 70, 12, 4, 16, 2), _bwd_only),
    (_scan(2, 70, 8, 8, 2, 16, False), _fwd_only), (_scan(2, 70, 8, 8, 2, 16, False), _bwd_only),
    (_dwconv(2, 10, 14, 32, 5, NONE, False), _bwd_only), (_dwconv(2, 16, 16, 32, 3, NONE, False, BF16), _bwd_only),
    (_instnorm(2, 300, 36, NONE), _fwd_only), (_instnorm(2, 300, 36, NONE), _bwd_only), (_groupnorm(2, 300, 36, 1, NONE), _fwd_only),
    (_groupnorm(2, 300, 36, 1, NONE), _bwd_only), (_igate((3, 100, 64)), _bwd_only), (_igate_res(2, 77, 36, 0), _bwd_only),
    (_skipgate(3, 5, 5, 36), _bwd_only), (_swish(20004), _bwd_only), (_bridge_pool(2, [(700, 64)]), _fwd_only), (_bridge_heads(7, [36, 20], 2144), _bwd_only),
    (_colsum(5000, 257), _fwd_only), (_linear(100, 48, 36, False, True), lambda c: _bwd_only(c, only=(1,))),
    (_linear_ts(4099, 48, 40, False), lambda c: _bwd_only(c, only=(1,))), (_conv3(2, 8, 8, 256, 64, NONE, False, True, (True, True)), _fwd_only),
    (_conv3(2, 8, 8, 256, 64, NONE, False, True, (True, True)), _bwd_only), (_conv3(2, 12, 12, 16, 24, NONE, False, False, (False, False)), lambda c: _bwd_only(c, only=(1,))),
    (_adn_prep((36, 72, 20, 12)), _bwd_only), (_adn_prep_multi([(8, 8, 4, 4), (20, 40, 12, 4)]), _bwd_only), (_rainloss(5001), _fwd_only),
    (_pool_counts(6, 37, 53, ((4, 2), (16, 8))), _fwd_only),
]


@pytest.mark.parametrize("case,stage", SHORT, ids=lambda v: v.id if isinstance(v, Case) else ("fwd" if v is _fwd_only else "bwd"))
def test_undersized_workspace_is_refused(case, stage, monkeypatch):
    """every *_ws_bytes query answers 4 bytes less than it should (where it asks for more than 16): the wrapper hands that on as ws_bytes,
    and the library's own check must refuse the call — RuntimeError with its workspace message — before it launches anything"""
    for obj, name, value in case.patch:
        monkeypatch.setattr(obj, name, value)
    fail = stage(case)
    real, shortened = lib.query, []

    def short_query(name, *args):
        v = real(name, *args)
        if name.endswith("_ws_bytes") and v > 16:
            shortened.append((name, v))
            return v - 4
        return v
    monkeypatch.setattr(lib, "query", short_query)
    with _Launches() as ev:
        with pytest.raises(RuntimeError, match="(?i)workspace"):
            fail()
    assert shortened, "no workspace query above 16 bytes: nothing was shortened"
    assert not ev.count, f"{case.id}: launched {ev.count} with a workspace 4 bytes short of {shortened}"


# ================================================================================================ 6. one pass over the whole model
def test_whole_model_under_guarded_workspaces(monkeypatch):
    """the 64 x 64 model, forward + loss + backward, eagerly: the plans only real layer shapes reach"""
    from models.ADNMUNet import create_ADNMUNet
    from models.loss import enRainfallLoss
    model = create_ADNMUNet(5, 20, 6, img_size=64)
    recipe.fill_parameters(model)
    model = model.to(DEV).train()
    frames = recipe.radar_batch(2, 25, 64, name="radar64").to(DEV)
    x, tgt = frames[:, :5], frames[:, 5:]
    loss_fn = enRainfallLoss(0.57, 0.25, gamma=0.0)

    def run():
        for p in model.parameters():
            p.grad = None
        out = model(x)
        loss = loss_fn(out, tgt)
        loss.backward()
        torch.cuda.synchronize()
        return [("out", out.detach()), ("loss", loss.detach())] + [(n, p.grad) for n, p in model.named_parameters() if p.grad is not None]
    g = check_contract(monkeypatch, "ADNMUNet-64", (2, 25, 64, 64), run, 100)
    callers = sorted({r[3].split(" ", 1)[1] for r in g.records})
    print(f"[ws-contract] ADNMUNet-64 callers: {callers}")
    assert g.calls >= 100
