"""The raw kernel entry points on the operands the fused nodes (ADNMixerFn, FeedForwardFn) hand them: column slices of wider buffers —
row stride larger than the width, a column offset, live neighbour columns.  For one entry point at one shape, every row operand and
every row output is an embedded view (tests/util.py: embed) with its own pads, and four things are asserted:
  1. layout invariance: the result equals, bit for bit, the same entry point on contiguous copies (a row stride changes addresses, not
     arithmetic; none of these kernels has a flat ld == C path, so no exception to this was needed);
  2. ground truth: the fp64 statement of the operation (as in test_kernels_gpu.py), rel-L2 1e-4 on fp32 outputs, 1e-3 on fp32
     gradients, 2e-2 for bf16 storage;
  3. containment: the pad columns of every output buffer still hold the poison, every input buffer is unchanged bit for bit
     (input pads hold NaN: a result that depends on a neighbour in any way is NaN);
  4. the stride reached the kernel: lib.call is recorded and the expected adnm_* entry point saw (pointer, ld) of the view, ld != width.
Column offsets and row strides are multiples of 8 elements, so every base pointer is 16-byte aligned for fp32 and bf16, as the
production nodes' are; misaligned / under-strided views are rejected by the entry points (the rejection tests at the end never launch)."""
import pytest
import torch
import torch.nn.functional as F

import adnm_oracle as O
from adnm_hip import ops, lib, recipe
from util import assert_close, embed, assert_pads_untouched, bits, poison_bits

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUT_TOL, GRAD_TOL, BF16_TOL = 1e-4, 1e-3, 2e-2
F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")


def T(name, shape, scale=1.0):
    return recipe.tensor(name, shape, scale)


def leaf(t):
    return t.clone().requires_grad_(True)


def rnd(t, dtype):
    """the values a `dtype` row tensor holds, as fp32 (the reference starts from what the kernel is given)"""
    return t.to(dtype).float()


def tols(dtype):
    return (OUT_TOL, GRAD_TOL) if dtype == F32 else (BF16_TOL, BF16_TOL)


@pytest.fixture
def calls(monkeypatch):
    """every lib.call made through adnm_hip.ops, as (entry point, args)"""
    rec, real = [], lib.call

    def spy(name, *args):
        rec.append((name, args))
        return real(name, *args)
    monkeypatch.setattr(lib, "call", spy)
    return rec


def assert_strided_call(rec, name, *views):
    """`name` was called with (data_ptr, row stride) of every view side by side in its arguments, the row stride not the width"""
    hits = [a for n, a in rec if n == name]
    assert hits, f"{name} was never called (got {sorted({n for n, _ in rec})})"
    for v in views:
        assert v.stride(0) != v.shape[1] and v.stride(1) == 1
        assert any(a[i] == v.data_ptr() and a[i + 1] == v.stride(0) for a in hits for i in range(len(a) - 1)), \
            f"{name} never saw the view (ptr, ld = {v.stride(0)}) of width {v.shape[1]}: a copy was made on the way"


def distinct(*views):
    """no two of these operands share a row stride: an entry point or kernel that indexes one with another's ld cannot pass"""
    lds = [v.stride(0) for v in views if v is not None]
    assert len(set(lds)) == len(lds), f"two operands share a row stride: {lds}"


class Views:
    """the embedded operands of one test: inputs (NaN pads, snapshot of every bit) and outputs (poison everywhere, payload included:
    an element the kernel fails to write stays a NaN)"""

    def __init__(self, dtype=F32):
        self.dtype, self.ins, self.outs = dtype, [], []

    def inp(self, t, left, right, name, dtype=None):
        buf, v = embed(t.to(DEV).to(dtype or self.dtype), left, right, poison="nan")
        self.ins.append((name, buf, bits(buf).clone()))
        return v

    def out(self, M, C, left, right, name, dtype=None):
        buf, v = embed(torch.zeros((M, C), dtype=dtype or self.dtype, device=DEV), left, right, poison="bits")
        bits(v).fill_(poison_bits(buf.dtype))
        self.outs.append((name, buf, left, C))
        return v

    def check(self):
        for name, buf, snap in self.ins:
            assert torch.equal(bits(buf.detach()), snap), f"input buffer {name} was written"
        for name, buf, left, C in self.outs:
            assert_pads_untouched(buf.detach(), left, C, name)


def same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(a, b), f"{what}: the strided result differs from the contiguous one"


# ------------------------------------------------------------------------------------------- row norms
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,d,mean,bias,affine,res", [(37, 48, True, True, False, False), (5, 260, False, False, True, True),
                                                      (777, 64, True, False, True, False)])
def test_rownorm_views(M, d, mean, bias, affine, res, dtype, calls):
    """forward into the left columns of a buffer whose next columns are live (cat[:, :di] beside wide[:, di:]); backward from the left
    slice of the gradient buffer (dcat[:, :di]) into a view, the residual gradient strided in one case"""
    eps = 1e-5 if mean else 1e-6
    otol, gtol = tols(dtype)
    tag = f"svrn{M}.{d}"
    x, cot, dres = rnd(T(tag + "x", (M, d), 2.0), dtype), rnd(T(tag + "c", (M, d)), dtype), rnd(T(tag + "r", (M, d)), dtype)
    w = 1 + 0.2 * T(tag + "w", (d,))
    b = 0.1 * T(tag + "b", (d,)) if bias else None
    sc, sh = (torch.tensor(1.3), torch.tensor(-0.2)) if affine else (None, None)
    # fp64 statement (test_rownorm)
    o = {k: (leaf(v.double()) if v is not None else None) for k, v in dict(x=x, w=w, b=b, sc=sc, sh=sh).items()}
    yo = O.layernorm(o["x"], o["w"], o["b"] if bias else 0.0, eps) if mean else O.rmsnorm(o["x"], o["w"], eps)
    if affine:
        yo = o["sc"] * yo + o["sh"]
    ((yo * cot.double()).sum() + ((o["x"] * dres.double()).sum() if res else 0)).backward()
    g = lambda t: t.to(DEV) if t is not None else None
    wg, bg, scg, shg = g(w), g(b), g(sc), g(sh)
    V = Views(dtype)
    xv, yv = V.inp(x, 8, 16, "x"), V.out(M, d, 0, 40, "y")
    y, mu, rstd = ops.k_rownorm_fwd(xv, wg, bg, scg, shg, eps, mean, out=yv)
    assert y is yv
    dyv, dxv = V.inp(cot, 0, 32, "dy"), V.out(M, d, 8, 8, "dx")
    drv = V.inp(dres, 24, 24, "dres") if res else None
    distinct(xv, yv, dyv, dxv, drv)
    dx, dw, db, dsc, dsh = ops.k_rownorm_bwd(dyv, xv, wg, bg, scg, mu, rstd, mean, bias, affine, dx_out=dxv, dres=drv, shift=shg)
    assert dx is dxv
    V.check()
    assert_strided_call(calls, "adnm_rownorm_fwd", xv, yv)
    assert_strided_call(calls, "adnm_rownorm_bwd", *([dyv, xv, dxv] + ([drv] if res else [])))
    # the same entry points on contiguous copies
    xc, dyc = xv.contiguous(), dyv.contiguous()
    y2, mu2, rstd2 = ops.k_rownorm_fwd(xc, wg, bg, scg, shg, eps, mean)
    dx2, dw2, db2, dsc2, dsh2 = ops.k_rownorm_bwd(dyc, xc, wg, bg, scg, mu2, rstd2, mean, bias, affine, dres=drv.contiguous() if res else None, shift=shg)
    same(yv.contiguous(), y2, "y"), same(rstd, rstd2, "rstd"), same(dxv.contiguous(), dx2, "dx"), same(dw, dw2, "dw")
    if mean:
        same(mu, mu2, "mu")
    if bias:
        same(db, db2, "db")
    if affine:
        same(dsc, dsc2, "dscale"), same(dsh, dsh2, "dshift")
    assert_close(yv.float(), yo, otol, "y")
    assert_close(dxv.float(), o["x"].grad, gtol, "dx")
    assert_close(dw, o["w"].grad, gtol, "dw")
    if bias:
        assert_close(db, o["b"].grad, gtol, "db")
    if affine:
        assert_close(dsc, o["sc"].grad, gtol, "dscale", atol=1e-4)
        assert_close(dsh, o["sh"].grad, gtol, "dshift", atol=1e-4)


# ------------------------------------------------------------------------------------------- SSD (K1)
@pytest.mark.parametrize("B,L,H,P,N,G,ln,dtype", [
    (1, 70, 12, 4, 16, 2, False, F32), (1, 70, 12, 4, 16, 2, False, BF16), (1, 33, 24, 8, 8, 1, False, F32), (3, 1, 4, 4, 8, 4, False, F32),
    (2, 300, 16, 4, 16, 2, True, F32), (2, 300, 16, 4, 16, 2, True, BF16)])
def test_ssd_reduce_views(B, L, H, P, N, G, ln, dtype, calls):
    """x | B | C as three adjacent slices of one buffer (xbc), dt_raw the right-hand columns of a second (proj[:, di + cx:]), y a view, the
    LayerNorm epilogue's output the left slice of a third (cat[:, :di]); backward: dx | dB | dC adjacent slices of a poisoned buffer laid
    out like dxbc, d dt_raw the right-hand columns of one laid out like dproj"""
    otol, gtol = tols(dtype)
    M, di, gn = B * L, H * P, G * N
    x, Bm, Cm = rnd(T("s.x", (B, L, H, P)), dtype), rnd(T("s.B", (B, L, gn)), dtype), rnd(T("s.C", (B, L, gn)), dtype)
    dt_raw, bias = rnd(T("s.dt", (B, L, H), 2.0) - 3.0, dtype), T("s.bias", (H,), 0.5)
    A_log, D = T("s.A", (H,), 1.0) + 1.0, 1 + 0.1 * T("s.D", (H,))
    cot = rnd(T("s.cot", (B, L, H, P)), dtype)
    ln_w, ln_b = 1 + 0.2 * T("s.lw", (di,)), 0.1 * T("s.lb", (di,))
    # fp64 statement (test_ssd_fwd_bwd)
    ins = [x, Bm, Cm, dt_raw, bias, A_log, D]
    o = [leaf(t.double()) for t in ins]
    yo, _ = O.ssd_reduce(o[0], F.softplus(o[3] + o[4]), torch.exp(o[5]), o[1], o[2], o[6], groups=G)
    (yo * cot.double()).sum().backward()
    V = Views(dtype)
    xbc = V.inp(torch.cat((x.reshape(M, di), Bm.reshape(M, gn), Cm.reshape(M, gn)), 1), 16, 8, "xbc")
    xv, bv, cv = xbc[:, :di], xbc[:, di:di + gn], xbc[:, di + gn:]
    tv = V.inp(dt_raw.reshape(M, H), 24, 0, "proj[dt]")
    yv = V.out(M, di, 8, 8, "y")
    par = [t.to(DEV) for t in (bias, A_log, D)]
    lnv = V.out(M, di, 0, 40, "cat[:, :di]") if ln else None
    res = ops.k_ssd_fwd(xv, bv, cv, tv, *par, B, L, H, P, N, G, y=yv, ln=(ln_w.to(DEV), ln_b.to(DEV), lnv, 1e-5) if ln else None)
    assert res[0] is yv
    kv = res[1]
    dyv = V.inp(cot.reshape(M, di), 8, 16, "dy")
    dxbc = V.out(M, di + 2 * gn, 8, 24, "dxbc")
    ddtv = V.out(M, H, 32, 0, "dproj[dt]")
    distinct(xbc, tv, yv, lnv, dyv, dxbc, ddtv)
    dbias, dA, dD = ops.k_ssd_bwd(dyv, xv, bv, cv, tv, *par, kv, dxbc[:, :di], dxbc[:, di:di + gn], dxbc[:, di + gn:], ddtv, B, L, H, P, N, G)
    V.check()
    assert_strided_call(calls, "adnm_ssd_reduce_fwd", *([xv, bv, cv, tv, yv] + ([lnv] if ln else [])))
    assert_strided_call(calls, "adnm_ssd_reduce_bwd", dyv, xv, bv, cv, tv, dxbc[:, :di], dxbc[:, di:di + gn], dxbc[:, di + gn:], ddtv)
    # contiguous copies
    c = [t.contiguous() for t in (xv, bv, cv, tv)]
    ln2 = torch.empty((M, di), dtype=dtype, device=DEV)
    res2 = ops.k_ssd_fwd(*c, *par, B, L, H, P, N, G, ln=(ln_w.to(DEV), ln_b.to(DEV), ln2, 1e-5) if ln else None)
    same(yv.contiguous(), res2[0], "y"), same(kv, res2[1], "kv")
    if ln:
        same(lnv.contiguous(), ln2, "LayerNorm(y)"), same(res[2], res2[2], "mu"), same(res[3], res2[3], "rstd")
    g2 = [torch.empty_like(t) for t in c]
    st2 = ops.k_ssd_bwd(dyv.contiguous(), *c, *par, res2[1], *g2, B, L, H, P, N, G)
    for name, a, b_ in zip(("dx", "dB", "dC", "ddt", "dbias", "dA_log", "dD"),
                           (dxbc[:, :di], dxbc[:, di:di + gn], dxbc[:, di + gn:], ddtv, dbias, dA, dD), g2 + list(st2)):
        same(a.contiguous(), b_, name)
    # ground truth
    assert_close(yv.float().view(B, L, H, P), yo, otol, "y")
    if ln:
        assert_close(lnv.float(), O.layernorm(yo.detach().reshape(M, di), ln_w.double(), ln_b.double(), 1e-5), otol, "LayerNorm(y)")
    got = (dxbc[:, :di].reshape(B, L, H, P), dxbc[:, di:di + gn].reshape(B, L, gn), dxbc[:, di + gn:].reshape(B, L, gn), ddtv.reshape(B, L, H), dbias, dA, dD)
    for name, a, b_ in zip(("dx", "dB", "dC", "ddt", "dbias", "dA_log", "dD"), got, o):
        assert_close(a.float(), b_.grad, gtol, name, atol=1e-6)


# ------------------------------------------------------------------------------------------- K1b chunked scan
@pytest.mark.parametrize("B,L,H,N,G,chunk", [(2, 70, 4, 8, 2, 16), (1, 33, 2, 16, 1, 8)])
def test_ssd_scan_interleaved_views(B, L, H, N, G, chunk, calls):
    """the form ADNMixerFn uses: the two scans (e = 0 forward in time, e = 1 backward) are interleaved head by head in one x / y / dt
    (head strides 2P / 2, pointers offset by e*P / e columns) and write one y and one set of gradient buffers.  Per half, the result is
    bitwise ops.ssd_scan on the de-interleaved contiguous operands, and the fp64 sequential recurrence is the ground truth."""
    P, M, gn = 4, B * L, G * N
    half = []
    for e in (0, 1):
        t = f"svsc{e}."
        half.append(dict(x=T(t + "x", (B, L, H, P)), Bm=T(t + "B", (B, L, gn)), Cm=T(t + "C", (B, L, gn)), dt=T(t + "dt", (B, L, H), 2.0) - 2.0,
                         bias=T(t + "bias", (H,), 0.5), A=T(t + "A", (H,), 1.0) + 1.0, D=1 + 0.1 * T(t + "D", (H,)), cot=T(t + "cot", (B, L, H, P))))
    il = lambda k, w: torch.stack((half[0][k].reshape(M, H, w), half[1][k].reshape(M, H, w)), 2).reshape(M, 2 * H * w)   # head 2j + e <- half e, head j
    di = 2 * H * P
    V = Views()
    xbc = V.inp(torch.cat((il("x", P), half[0]["Bm"].reshape(M, gn), half[1]["Bm"].reshape(M, gn), half[0]["Cm"].reshape(M, gn), half[1]["Cm"].reshape(M, gn)), 1),
                16, 8, "xbc")
    dtv = V.inp(il("dt", 1), 24, 0, "proj[dt]")
    par = [torch.stack((half[0][k], half[1][k]), 1).reshape(2 * H).to(DEV) for k in ("bias", "A", "D")]
    yv = V.out(M, di, 8, 16, "y")
    dyv = V.inp(il("cot", P), 8, 8, "dy")
    dxbc = V.out(M, di + 4 * gn, 24, 8, "dxbc")
    ddtv = V.out(M, 2 * H, 32, 0, "dproj[dt]")
    distinct(xbc, dtv, yv, dyv, dxbc, ddtv)
    poison = poison_bits(F32)
    S, stats = [], []
    for e in (0, 1):
        xe, be, ce = xbc[:, e * P:di], xbc[:, di + e * gn:di + (e + 1) * gn], xbc[:, di + 2 * gn + e * gn:di + 2 * gn + (e + 1) * gn]
        S.append(ops.k_ssd_scan_fwd(xe, 2 * P, be, ce, dtv[:, e:], 2, par[0][e:], par[1][e:], par[2][e:], 2, yv[:, e * P:], 2 * P, B, L, H, P, N, G,
                                    chunk, e == 1))
        if e == 0:   # the other half's columns of y are still untouched
            y3 = bits(yv).reshape(M, H, 2, P)
            assert bool((y3[:, :, 1] == poison).all()), "the first scan wrote columns of the second one's heads"
            assert not bool((y3[:, :, 0] == poison).any())
        assert_strided_call(calls, "adnm_ssd_scan_fwd", xe, be, ce, dtv[:, e:], yv[:, e * P:])
    for e in (0, 1):
        xe, be, ce = xbc[:, e * P:di], xbc[:, di + e * gn:di + (e + 1) * gn], xbc[:, di + 2 * gn + e * gn:di + 2 * gn + (e + 1) * gn]
        dbe, dce = dxbc[:, di + e * gn:di + (e + 1) * gn], dxbc[:, di + 2 * gn + e * gn:di + 2 * gn + (e + 1) * gn]
        stats.append(ops.k_ssd_scan_bwd(dyv[:, e * P:], 2 * P, xe, 2 * P, be, ce, dtv[:, e:], 2, par[0][e:], par[1][e:], par[2][e:], 2, S[e],
                                        dxbc[:, e * P:di], 2 * P, dbe, dce, ddtv[:, e:], 2, B, L, H, P, N, G, chunk, e == 1))
        if e == 0:
            g3 = bits(dxbc[:, :di]).reshape(M, H, 2, P)
            assert bool((g3[:, :, 1] == poison).all()) and bool((bits(ddtv).reshape(M, H, 2)[:, :, 1] == poison).all()), \
                "the first scan's backward wrote gradient columns of the second one's heads"
        assert_strided_call(calls, "adnm_ssd_scan_bwd", dyv[:, e * P:], xe, be, ce, dtv[:, e:], dxbc[:, e * P:di], dbe, dce, ddtv[:, e:])
    V.check()
    for e in (0, 1):
        h = half[e]
        ins = [h["x"], h["Bm"], h["Cm"], h["dt"], h["bias"], h["A"], h["D"]]
        got = (yv.reshape(M, H, 2, P)[:, :, e].reshape(B, L, H, P), dxbc[:, :di].reshape(M, H, 2, P)[:, :, e].reshape(B, L, H, P),
               dxbc[:, di + e * gn:di + (e + 1) * gn].reshape(B, L, gn), dxbc[:, di + 2 * gn + e * gn:di + 2 * gn + (e + 1) * gn].reshape(B, L, gn),
               ddtv.reshape(M, H, 2)[:, :, e].reshape(B, L, H), *stats[e])
        names = ("y", "dx", "dB", "dC", "ddt", "dbias", "dA_log", "dD")
        # bitwise: the stand-alone scan on the de-interleaved contiguous half
        g = [leaf(t.to(DEV)) for t in ins]
        yg = ops.ssd_scan(*g, G, chunk, e == 1)
        yg.backward(h["cot"].to(DEV))
        for name, a, b_ in zip(names, got, [yg.detach()] + [t.grad for t in g]):
            same(a.contiguous(), b_, f"half {e} {name}")
        # ground truth (test_ssd_scan_vs_sequential_oracle)
        o = [leaf(t.double()) for t in ins]
        flip = (lambda t: t.flip(1)) if e == 1 else (lambda t: t)
        yo = flip(O.ssd_chunk_scan(flip(o[0]), flip(F.softplus(o[3] + o[4])), -torch.exp(o[5]), flip(o[1]), flip(o[2]), o[6], G))
        (yo * h["cot"].double()).sum().backward()
        assert_close(got[0], yo, OUT_TOL, f"half {e} y")
        for name, a, b_ in zip(names[1:], got[1:], o):
            assert_close(a, b_.grad, GRAD_TOL, f"half {e} {name}", atol=1e-6)


# ------------------------------------------------------------------------------------------- depthwise conv
_ACTS = {lib.ACT_NONE: lambda t: t, lib.ACT_SILU: O.silu, lib.ACT_GELU: O.gelu}


@pytest.mark.parametrize("B,H,W,C,K,act,bias,chan_major,addend,dtype", [
    (1, 7, 9, 8, 3, lib.ACT_NONE, True, False, False, F32), (1, 7, 9, 8, 3, lib.ACT_NONE, True, True, False, BF16),
    (2, 10, 14, 32, 5, lib.ACT_NONE, False, True, True, F32), (2, 10, 14, 32, 5, lib.ACT_NONE, False, False, True, BF16),
    (1, 5, 3, 12, 5, lib.ACT_GELU, True, False, False, F32),
    (3, 33, 34, 24, 3, lib.ACT_SILU, False, True, False, F32), (3, 33, 34, 24, 3, lib.ACT_SILU, False, False, False, BF16)])
def test_dwconv_views(B, H, W, C, K, act, bias, chan_major, addend, dtype, calls):
    """x a left slice (proj[:, :di + cx]), y a right slice at an offset (wide[:, di:]), the addend strided where there is one; backward:
    dy a right slice (dwide[:, di:]), dx a left slice of another buffer (dproj[:, :di + cx]); the weight-gradient leaf reads the same views.
    (3, 33, 34, 24): the ragged strips of the column-walker weight gradient."""
    otol, gtol = tols(dtype)
    M = B * H * W
    x, w, cot = rnd(T("svdw.x", (B, H * W, C)), dtype), T("svdw.w", (C, 1, K, K), 0.5), rnd(T("svdw.c", (B, H * W, C)), dtype)
    b = T("svdw.b", (C,), 0.3) if bias else None
    add = rnd(T("svdw.a", (B, H * W, C)), dtype) if addend else None
    # fp64 statement (test_dwconv)
    xo, wo = leaf(x.double()), leaf(w.double())
    bo = leaf(b.double()) if bias else None
    yo = O.seq(_ACTS[act](F.conv2d(O.img(xo, H, W), wo, bo, padding=K // 2, groups=C)))
    if addend:
        yo = yo + add.double()
    (yo * cot.double()).sum().backward()
    wt = (w.reshape(C, K * K).contiguous() if chan_major else ops.tap_major(w)).to(DEV)
    bg = b.to(DEV) if bias else None
    V = Views(dtype)
    xv, yv = V.inp(x.reshape(M, C), 0, 24, "x"), V.out(M, C, 16, 0, "y")
    av = V.inp(add.reshape(M, C), 8, 32, "addend") if addend else None
    y = ops.k_dwconv_fwd(xv, wt, bg, B, H, W, C, K, act, y=yv, addend=av, chan_major=chan_major)
    assert y is yv
    dyv, dxv = V.inp(cot.reshape(M, C), 32, 0, "dy"), V.out(M, C, 0, 8, "dx")
    distinct(xv, yv, av, dyv, dxv)
    dx, dwt, db = ops.k_dwconv_bwd(dyv, xv, wt, bg, B, H, W, C, K, act, dx=dxv, want_bias=bias, chan_major=chan_major)
    assert dx is dxv
    V.check()
    assert_strided_call(calls, "adnm_dwconv_fwd", *([xv, yv] + ([av] if addend else [])))
    assert_strided_call(calls, "adnm_dwconv_bwd", dyv, xv, dxv)
    assert_strided_call(calls, "adnm_dwconv_wgrad", *([xv] + ([dyv] if act == lib.ACT_NONE else [])))   # (with an activation g is the dense dpre)
    xc, dyc = xv.contiguous(), dyv.contiguous()
    y2 = ops.k_dwconv_fwd(xc, wt, bg, B, H, W, C, K, act, addend=av.contiguous() if addend else None, chan_major=chan_major)
    dx2, dwt2, db2 = ops.k_dwconv_bwd(dyc, xc, wt, bg, B, H, W, C, K, act, want_bias=bias, chan_major=chan_major)
    same(yv.contiguous(), y2, "y"), same(dxv.contiguous(), dx2, "dx"), same(dwt, dwt2, "dw")
    assert_close(yv.float().view(B, H * W, C), yo, otol, "y")
    assert_close(dxv.float().view(B, H * W, C), xo.grad, gtol, "dx")
    assert_close(dwt if chan_major else dwt.t(), wo.grad.reshape(C, K * K), gtol, "dw")
    if bias:
        same(db, db2, "db")
        assert_close(db, bo.grad, gtol, "db")


# ------------------------------------------------------------------------------------------- FeedForward gate
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,Fh", [(301, 12), (64, 128)])
def test_gate_views(M, Fh, dtype, calls):
    otol, gtol = tols(dtype)
    h, cot = rnd(T(f"svg.h{M}", (M, 2 * Fh), 3.0), dtype), rnd(T(f"svg.c{M}", (M, Fh)), dtype)
    ho = leaf(h.double())
    yo = O.gelu(ho[:, :Fh]) * torch.sigmoid(ho[:, Fh:])
    (yo * cot.double()).sum().backward()
    V = Views(dtype)
    hv, dyv = V.inp(h, 8, 16, "h"), V.inp(cot, 16, 8, "dy")
    distinct(hv, dyv)
    y, dh = ops.k_gate_fwd(hv, Fh), ops.k_gate_bwd(dyv, hv, Fh)
    V.check()
    assert_strided_call(calls, "adnm_gate_fwd", hv)
    assert_strided_call(calls, "adnm_gate_bwd", dyv, hv)
    same(y, ops.k_gate_fwd(hv.contiguous(), Fh), "y"), same(dh, ops.k_gate_bwd(dyv.contiguous(), hv.contiguous(), Fh), "dh")
    assert_close(y.float(), yo, otol, "gate")
    assert_close(dh.float(), ho.grad, gtol, "dgate")


# ------------------------------------------------------------------------------------------- fused mixes (public functions)
def _leaf_view(V, t, left, right, name):
    """an embedded input view that is part of a leaf: the gradient of the view arrives in the leaf's .grad at the same columns"""
    v = V.inp(t, left, right, name)
    buf = V.ins[-1][1].requires_grad_(True)
    return buf, buf[:, left:left + t.shape[1]]


def _grad_of(buf, v, left):
    return buf.grad[:, left:left + v.shape[1]]


@pytest.mark.parametrize("M,C,K,use_gamma", [(333, 64, 3, True), (7, 2048, 2, False)])
def test_lincomb_views(M, C, K, use_gamma, calls):
    xs = [T(f"svlc.x{k}{M}", (M, C)) for k in range(K)]
    ss = [torch.tensor([0.7 + 0.3 * k]) for k in range(K)]
    ss[0] = None
    gamma = 1 + 0.2 * T("svlc.g", (C,)) if use_gamma else None
    cot = T(f"svlc.c{M}", (M, C))
    # fp64 statement (test_lincomb)
    xo = [leaf(x.double()) for x in xs]
    so = [leaf(s.double()) if s is not None else None for s in ss]
    go = leaf(gamma.double()) if use_gamma else None
    yo = sum((x if s is None else s * x) for x, s in zip(xo, so))
    yo = yo * go if use_gamma else yo
    (yo * cot.double()).sum().backward()
    pads = [(8, 16), (0, 8), (24, 16)]
    V = Views()
    lv = [_leaf_view(V, x, *pads[k], f"x{k}") for k, x in enumerate(xs)]
    cv = V.inp(cot, 16, 16, "dy")
    distinct(cv, *[v for _, v in lv])
    sg = [leaf(s.to(DEV)) if s is not None else None for s in ss]
    gg = leaf(gamma.to(DEV)) if use_gamma else None
    yg = ops.lincomb([v for _, v in lv], sg, gg)
    yg.backward(cv)
    V.check()
    assert_strided_call(calls, "adnm_lincomb_fwd", *[v for _, v in lv])
    assert_strided_call(calls, "adnm_lincomb_bwd", cv, *[v for _, v in lv])
    xc = [leaf(x.to(DEV)) for x in xs]
    sc = [leaf(s.to(DEV)) if s is not None else None for s in ss]
    gc = leaf(gamma.to(DEV)) if use_gamma else None
    yc = ops.lincomb(xc, sc, gc)
    yc.backward(cot.to(DEV))
    same(yg.detach(), yc.detach(), "y")
    assert_close(yg, yo, OUT_TOL, "y")
    for k in range(K):
        dxk = _grad_of(lv[k][0], lv[k][1], pads[k][0])
        same(dxk.contiguous(), xc[k].grad, f"dx{k}")
        assert_close(dxk, xo[k].grad, GRAD_TOL, f"dx{k}")
        if ss[k] is not None:
            same(sg[k].grad, sc[k].grad, f"ds{k}")
            assert_close(sg[k].grad, so[k].grad, GRAD_TOL, f"ds{k}", atol=1e-4)
    if use_gamma:
        same(gg.grad, gc.grad, "dgamma")
        assert_close(gg.grad, go.grad, GRAD_TOL, "dgamma", atol=1e-5)


def test_catmix_views(calls):
    M, d = 300, 64
    x, r, f = (T(f"svcm.{n}", (M, d)) for n in "xrf")
    cot = T("svcm.cot", (M, 2 * d))
    al = [torch.tensor(v) for v in (1.1, 0.9, 0.7, -0.4)]
    # fp64 statement (test_catmix)
    xo, ro, fo, ao = leaf(x.double()), leaf(r.double()), leaf(f.double()), [leaf(a.double()) for a in al]
    yo = torch.cat((ao[0] * xo, ao[1] * ro), -1) + torch.cat((ao[2] * fo, ao[3] * fo), -1)
    (yo * cot.double()).sum().backward()
    pads = [(8, 8), (0, 24), (16, 24)]
    V = Views()
    lv = [_leaf_view(V, t, *pads[k], n) for k, (t, n) in enumerate(zip((x, r, f), "xrf"))]
    cv = V.inp(cot, 8, 16, "dy")
    distinct(cv, *[v for _, v in lv])
    ag = [leaf(a.to(DEV)) for a in al]
    yg = ops.catmix(lv[0][1], lv[1][1], lv[2][1], *ag)
    yg.backward(cv)
    V.check()
    assert_strided_call(calls, "adnm_catmix_fwd", *[v for _, v in lv])
    assert_strided_call(calls, "adnm_catmix_bwd", cv, *[v for _, v in lv])
    lc, ac = [leaf(t.to(DEV)) for t in (x, r, f)], [leaf(a.to(DEV)) for a in al]
    yc = ops.catmix(*lc, *ac)
    yc.backward(cot.to(DEV))
    same(yg.detach(), yc.detach(), "y")
    assert_close(yg, yo, OUT_TOL, "catmix")
    for k, (n, o_) in enumerate(zip(("dx", "dr", "df"), (xo, ro, fo))):
        gk = _grad_of(lv[k][0], lv[k][1], pads[k][0])
        same(gk.contiguous(), lc[k].grad, n)
        assert_close(gk, o_.grad, GRAD_TOL, n)
    for i in range(4):
        same(ag[i].grad, ac[i].grad, f"da{i + 1}")
        assert_close(ag[i].grad, ao[i].grad, GRAD_TOL, f"da{i + 1}", atol=1e-5)


@pytest.mark.parametrize("M,d,mean,gamma,affine", [(131, 1024, True, True, True), (50, 512, False, False, True)])
def test_mixnorm_views(M, d, mean, gamma, affine, calls):
    eps = 1e-5
    x0, x1 = T(f"svmn.a{M}", (M, d), 2.0), T(f"svmn.b{M}", (M, d), 1.5)
    w, g = 1 + 0.2 * T(f"svmn.w{d}", (d,)), (1 + 0.3 * T(f"svmn.g{d}", (d,))) if gamma else None
    s0, s1 = torch.tensor([0.9]), torch.tensor([1.2])
    sc, sh = (torch.tensor(1.3), torch.tensor(-0.2)) if affine else (None, None)
    c1, c2 = T(f"svmn.c{M}", (M, d)), T(f"svmn.e{M}", (M, d))
    # fp64 statement (test_mixnorm)
    dbl = lambda t: leaf(t.double()) if t is not None else None
    po = [dbl(t) for t in (x0, x1, w, g, s0, s1, sc, sh)]
    xo = po[4] * po[0] + po[5] * po[1]
    if gamma:
        xo = xo * po[3]
    no = O.layernorm(xo, po[2], 0.0, eps) if mean else O.rmsnorm(xo, po[2], eps)
    if affine:
        no = po[6] * no + po[7]
    ((no * c1.double()).sum() + (xo * c2.double()).sum()).backward()
    V = Views()
    (b0, v0), (b1, v1) = _leaf_view(V, x0, 8, 8, "x0"), _leaf_view(V, x1, 0, 32, "x1")
    c1v, c2v = V.inp(c1, 16, 8, "d xn"), V.inp(c2, 24, 16, "d x")
    distinct(v0, v1, c1v, c2v)
    dev = lambda t: leaf(t.to(DEV)) if t is not None else None
    pg = [dev(t) for t in (w, g, s0, s1, sc, sh)]
    ng, xg = ops.mixnorm([v0, v1], [pg[2], pg[3]], pg[1], pg[0], None, pg[4], pg[5], eps, mean)
    torch.autograd.backward([ng, xg], [c1v, c2v])
    V.check()
    assert_strided_call(calls, "adnm_mixnorm_fwd", v0, v1)
    assert_strided_call(calls, "adnm_mixnorm_bwd", c1v, c2v, v0, v1)
    xc = [leaf(x0.to(DEV)), leaf(x1.to(DEV))]
    pc = [dev(t) for t in (w, g, s0, s1, sc, sh)]
    nc, xcm = ops.mixnorm(xc, [pc[2], pc[3]], pc[1], pc[0], None, pc[4], pc[5], eps, mean)
    torch.autograd.backward([nc, xcm], [c1.to(DEV), c2.to(DEV)])
    same(ng.detach(), nc.detach(), "xn"), same(xg.detach(), xcm.detach(), "x")
    assert_close(xg, xo, OUT_TOL, "x")
    assert_close(ng, no, OUT_TOL, "xn")
    got = [_grad_of(b0, v0, 8), _grad_of(b1, v1, 0)] + [p.grad if p is not None else None for p in pg]
    want = [xc[0].grad, xc[1].grad] + [p.grad if p is not None else None for p in pc]
    for name, a, c_, o_ in zip(("dx0", "dx1", "dw", "dgamma", "ds0", "ds1", "dscale", "dshift"), got, want, po):
        if a is not None:
            same(a.contiguous(), c_, name)
            assert_close(a, o_.grad, GRAD_TOL, name, atol=1e-4)


# ------------------------------------------------------------------------------------------- tall-skinny GEMMs
def _bf16_round(t):
    return t.to(BF16).to(t.dtype)


@pytest.fixture
def bf16_mfma():
    ops.set_mfma_precision("bf16")
    yield
    ops.set_mfma_precision("f32")


TS_SHAPES = [(4099, 32, 208), (4099, 128, 32), (333, 64, 20)]


def _ts_routes(M, K, N):
    """-> the output-gradient width of the input-gradient product.  The tall-skinny kernel takes every forward and weight-gradient shape
    here; as an input gradient it declines (333, 64, 20) (a reduction over 20 columns: not a multiple of 16), which then runs on the
    nearest width it accepts: the first 16 columns."""
    assert lib.query("adnm_tsgemm_supported", M, N, K) == 1 and lib.query("adnm_tsgemm_tn_supported", M, N, K) == 1, "the tall-skinny kernels are meant to take this shape"
    Nd = N if lib.query("adnm_tsgemm_supported", M, K, N) == 1 else N // 16 * 16
    assert lib.query("adnm_tsgemm_supported", M, K, Nd) == 1
    return Nd


@pytest.mark.parametrize("M,K,N", TS_SHAPES)
def test_tsgemm_views_f32(M, K, N, calls, monkeypatch):
    """k_linear / k_linear_dx / k_linear_dw as ADNMixerFn calls them on cat, dcat and dproj: strided input rows, out= a strided view, a
    strided second operand of the weight gradient; a ragged M reaches the tall-skinny kernels with the row threshold lowered"""
    monkeypatch.setattr(ops, "TS_MIN_ROWS", 1)
    Nd = _ts_routes(M, K, N)
    x, w, cot = T(f"svts.x{M}{K}", (M, K)), T(f"svts.w{N}{K}", (N, K), 0.3), T(f"svts.c{M}{N}", (M, N))
    wd, wdx = w.to(DEV), w[:Nd].to(DEV)
    V = Views()
    xv, yv = V.inp(x, 8, 24, "x"), V.out(M, N, 16, 8, "y")
    dyv, dxv = V.inp(cot, 0, 16, "dy"), V.out(M, K, 8, 8, "dx")
    dyd = dyv[:, :Nd]
    distinct(xv, yv, dyv, dxv)
    assert ops.k_linear(xv, wd, None, out=yv) is yv
    assert ops.k_linear_dx(dyd, wdx, out=dxv) is dxv
    dw, _ = ops.k_linear_dw(dyv, xv, False)
    V.check()
    nt = [a for n, a in calls if n == "adnm_tsgemm_nt"]
    assert len(nt) == 2 and [n for n, _ in calls if n == "adnm_skgemm"] == []
    assert_strided_call(calls, "adnm_tsgemm_nt", xv, yv, dyd, dxv)
    assert_strided_call(calls, "adnm_tsgemm_tn", dyv, xv)
    same(yv.contiguous(), ops.k_linear(xv.contiguous(), wd, None), "y")
    same(dxv.contiguous(), ops.k_linear_dx(dyd.contiguous(), wdx), "dx")
    same(dw, ops.k_linear_dw(dyv.contiguous(), xv.contiguous(), False)[0], "dw")
    assert_close(yv, x.double() @ w.double().t(), OUT_TOL, "y")
    assert_close(dxv, cot[:, :Nd].double() @ w[:Nd].double(), GRAD_TOL, "dx")
    assert_close(dw, cot.double().t() @ x.double(), GRAD_TOL, "dw")


@pytest.mark.parametrize("M,K,N", TS_SHAPES)
def test_tsgemm_views_bf16_rows(M, K, N, calls, monkeypatch, bf16_mfma):
    """bf16 token rows in and / or out (the wide internals of ADNMixerFn / FeedForwardFn at the full-resolution level), strided; the
    references of test_tsgemm_bf16_token_storage"""
    monkeypatch.setattr(ops, "TS_MIN_ROWS", 1)
    Nd = _ts_routes(M, K, N)
    x, w, cot = T(f"svtb.x{M}{K}", (M, K)), T(f"svtb.w{N}{K}", (N, K), 0.05), T(f"svtb.c{M}{N}", (M, N))
    wd, wdx, wr = w.to(DEV), w[:Nd].to(DEV), _bf16_round(w).double()
    V = Views()
    xb, cb = V.inp(x, 8, 24, "x bf16", BF16), V.inp(cot, 0, 16, "dy bf16", BF16)
    x32, c32 = V.inp(x, 16, 8, "x fp32"), V.inp(cot, 24, 8, "dy fp32")
    y32, y16 = V.out(M, N, 16, 8, "y fp32"), V.out(M, N, 8, 32, "y bf16", BF16)
    dx32 = V.out(M, K, 8, 8, "dx fp32")
    distinct(xb, cb, x32, c32, y32, y16, dx32)
    ops.k_linear(xb, wd, None, out=y32)       # bf16 rows in, fp32 out
    ops.k_linear(x32, wd, None, out=y16)      # fp32 rows in, bf16 out
    cbd = cb[:, :Nd]
    ops.k_linear_dx(cbd, wdx, out=dx32)       # bf16 gradient rows in
    dw, _ = ops.k_linear_dw(cb, xb, False)    # both operands bf16 rows
    dw2, _ = ops.k_linear_dw(c32, xb, False)  # fp32 gradient rows, bf16 activations
    V.check()
    assert [n for n, _ in calls if n == "adnm_skgemm"] == []
    assert_strided_call(calls, "adnm_tsgemm_nt", xb, y32, x32, y16, cbd, dx32)
    assert_strided_call(calls, "adnm_tsgemm_tn", cb, xb, c32)
    xbc, cbc = xb.contiguous(), cb.contiguous()
    same(y32.contiguous(), ops.k_linear(xbc, wd, None, out_dtype=F32), "bf16 in / fp32 out")
    same(y16.contiguous(), ops.k_linear(x32.contiguous(), wd, None, out_dtype=BF16), "fp32 in / bf16 out")
    same(dx32.contiguous(), ops.k_linear_dx(cbd.contiguous(), wdx, out_dtype=F32), "dx from bf16 rows")
    same(dw, ops.k_linear_dw(cbc, xbc, False)[0], "dw from bf16 rows")
    same(dw2, ops.k_linear_dw(c32.contiguous(), xbc, False)[0], "dw from fp32 x bf16 rows")
    assert_close(y32, xb.double().cpu() @ wr.t(), 2e-6, "bf16 in / fp32 out")
    assert_close(y16.double(), _bf16_round(x).double() @ wr.t(), 4e-3, "fp32 in / bf16 out (one rounding to bf16)")
    assert_close(dx32, cbd.double().cpu() @ wr[:Nd], 2e-6, "dx from bf16 rows")
    assert_close(dw, cb.double().cpu().t() @ xb.double().cpu(), 1e-5, "dw from bf16 rows")
    assert_close(dw2, cot.double().t() @ xb.double().cpu(), 1e-5, "dw from fp32 x bf16 rows")


# ------------------------------------------------------------------------------------------- Haar analysis, channel stride > 1
@pytest.mark.parametrize("B,H,W,C", [(1, 11, 13, 4), (2, 19, 23, 12)])
def test_haar_channel_stride_views(B, H, W, C, calls):
    """k_haar_dwt / k_wt_level read channel c at column c*cx of a row that is wider than C*cx (the LL band of the level above inside its
    (., 4C) sub-band tensor, here inside a wider buffer still): every other column is a NaN.  cx = 4: the entry points take cx in {1, 4}
    only.  Against the same entry point on the gathered contiguous input, and the fp64 butterfly / depthwise conv."""
    cx, K, M = 4, 3, B * H * W
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    x, taps = T(f"svh.x{H}", (M, C)), T(f"svh.t{H}", (K * K, 4 * C), 0.3)
    wide = torch.full((M, C * cx), NAN)
    wide[:, ::cx] = x
    V = Views()
    xv = V.inp(wide, 8, 12, "x")
    xc, td = x.to(DEV), taps.to(DEV)
    y = ops.k_haar_dwt(xv, B, H, W, C, cx)
    sub, tag = ops.k_wt_level(xv, B, H, W, C, cx, td, K)
    V.check()
    assert_strided_call(calls, "adnm_haar_dwt", xv)
    assert_strided_call(calls, "adnm_wt_level", xv)
    # (the reference launch is the cx = 1 instantiation of the same entry point on the gathered columns: the bitwise match also holds the
    # two template variants — scalar loads at a channel stride, 16-byte loads without — to one arithmetic)
    sub1, tag1 = ops.k_wt_level(xc, B, H, W, C, 1, td, K)
    same(y, ops.k_haar_dwt(xc, B, H, W, C, 1), "DWT"), same(sub, sub1, "sub"), same(tag, tag1, "tag")
    img = F.pad(O.img(x.double().view(B, H * W, C), H, W), (0, W % 2, 0, H % 2))
    so = O.haar_dwt(img).reshape(B, 4 * C, h2, w2)
    to = F.conv2d(so, taps.double().t().reshape(4 * C, 1, K, K), None, padding=K // 2, groups=4 * C)
    assert_close(y.view(B, h2 * w2, 4 * C), O.seq(so), OUT_TOL, "DWT")
    assert_close(sub.view(B, h2 * w2, 4 * C), O.seq(so), OUT_TOL, "sub")
    assert_close(tag.view(B, h2 * w2, 4 * C), O.seq(to), OUT_TOL, "tag")


# ------------------------------------------------------------------------------------------- dense 3x3 conv
def test_conv3_views(calls):
    """ops.conv3 keeps a token tensor whose rows are strided (x2.stride(0) goes to the kernels as ldin) and, without an activation, a
    strided incoming gradient (lddo of the input- and weight-gradient kernels)"""
    B, H, W, K, N = 2, 8, 8, 20, 20
    M = B * H * W
    x, w, cot, b = T("svc3.x", (B, H * W, K)), T("svc3.w", (N, K, 3, 3), 0.2), T("svc3.c", (B, H * W, N)), T("svc3.b", (N,))
    # fp64 statement (test_conv3)
    xo, wo, bo = leaf(x.double()), leaf(w.double()), leaf(b.double())
    yo = F.conv2d(xo.view(B, H, W, K).permute(0, 3, 1, 2), wo, bo, padding=1).permute(0, 2, 3, 1).reshape(B, H * W, N)
    (yo * cot.double()).sum().backward()
    V = Views()
    xbuf, xv = _leaf_view(V, x.reshape(M, K), 8, 12, "x")
    cv = V.inp(cot.reshape(M, N), 16, 12, "dy")
    distinct(xv, cv)
    wg, bg = leaf(w.to(DEV)), leaf(b.to(DEV))
    yg = ops.conv3(xv.unflatten(0, (B, H * W)), wg, bg, H, W, lib.ACT_NONE)
    yg.backward(cv.unflatten(0, (B, H * W)))
    V.check()
    assert_strided_call(calls, "adnm_conv3_fwd", xv)
    assert_strided_call(calls, "adnm_conv3_dgrad", cv)
    assert_strided_call(calls, "adnm_conv3_wgrad", cv, xv)
    xc, wc, bc = leaf(x.to(DEV)), leaf(w.to(DEV)), leaf(b.to(DEV))
    yc = ops.conv3(xc, wc, bc, H, W, lib.ACT_NONE)
    yc.backward(cot.to(DEV))
    dx = _grad_of(xbuf, xv, 8)
    same(yg.detach(), yc.detach(), "y"), same(dx.contiguous().view(B, H * W, K), xc.grad, "dx")
    same(wg.grad.contiguous(), wc.grad.contiguous(), "dw"), same(bg.grad, bc.grad, "db")
    assert_close(yg, yo, OUT_TOL, "y")
    assert_close(dx.view(B, H * W, K), xo.grad, GRAD_TOL, "dx")
    assert_close(wg.grad, wo.grad, GRAD_TOL, "dw")
    assert_close(bg.grad, bo.grad, GRAD_TOL, "db")


# ------------------------------------------------------------------------------------------- what the entry points refuse
# Every ADNM_REQUIRE tested here stands before the first launch of its entry point (it returns ADNM_EINVAL): nothing below reaches a
# kernel.  `off2`: a view 2 elements into a row — 8 bytes off for fp32, 4 for bf16: no vector access of 4 elements is aligned there.
def _off2(M, C, dtype=F32, ld=None):
    return torch.zeros((M, (ld or C + 8)), dtype=dtype, device=DEV)[:, 2:2 + C]


def _ok(M, C, dtype=F32):
    return torch.zeros((M, C + 8), dtype=dtype, device=DEV)[:, :C]


@pytest.fixture
def made(monkeypatch):
    """the names of the entry points called through lib.call, a refused call included"""
    names, real = [], lib.call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(lib, "call", spy)
    return names


@pytest.fixture
def no_launch(made):
    """The wrapper under test reached the library exactly once, with the call that was refused: it made no copy and no second call on the
    way.  That the refusal itself launches nothing is not observed here but read in the code: every ADNM_REQUIRE these tests name stands
    before the workspace check and before the first launch of its entry point, and returns ADNM_EINVAL."""
    yield made
    assert len(made) == 1, made


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("which", ["x", "y"])
def test_rownorm_fwd_rejects_misaligned(which, dtype, no_launch):
    M, d = 8, 16
    w = torch.ones(d, device=DEV)
    x, y = (_off2(M, d, dtype), _ok(M, d, dtype)) if which == "x" else (_ok(M, d, dtype), _off2(M, d, dtype))
    with pytest.raises(RuntimeError, match="rownorm_fwd: x and y must be aligned to 4 elements"):
        ops.k_rownorm_fwd(x, w, None, None, None, 1e-5, True, out=y)


@pytest.mark.parametrize("which", ["dy", "x", "dx", "dres"])
def test_rownorm_bwd_rejects_misaligned(which, no_launch):
    M, d = 8, 16
    w, mu, rstd = torch.ones(d, device=DEV), torch.zeros(M, device=DEV), torch.ones(M, device=DEV)
    v = {k: (_off2(M, d) if k == which else _ok(M, d)) for k in ("dy", "x", "dx", "dres")}
    with pytest.raises(RuntimeError, match="rownorm_bwd: dy, x, dx and the residual gradient must be aligned"):
        ops.k_rownorm_bwd(v["dy"], v["x"], w, None, None, mu, rstd, True, False, False, dx_out=v["dx"], dres=v["dres"])


def _ssd_operands(bad=None, dtype=F32):
    B, L, H, P, N, G = 1, 8, 4, 4, 8, 1
    M = B * L
    mk = lambda name, C: _off2(M, C, dtype) if name == bad else _ok(M, C, dtype)
    v = {n: mk(n, C) for n, C in (("x", H * P), ("Bm", G * N), ("Cm", G * N), ("dt", H), ("y", H * P), ("dy", H * P), ("dx", H * P), ("dBm", G * N),
                                  ("dCm", G * N), ("ddt", H))}
    par = [torch.zeros(H, device=DEV) for _ in range(3)]
    return v, par, (B, L, H, P, N, G)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("bad", ["x", "Bm", "Cm", "y"])
def test_ssd_reduce_fwd_rejects_misaligned(bad, dtype, no_launch):
    v, par, dims = _ssd_operands(bad, dtype)
    with pytest.raises(RuntimeError, match="ssd_reduce_fwd: x, B, C, y and the LayerNorm output must be aligned"):
        ops.k_ssd_fwd(v["x"], v["Bm"], v["Cm"], v["dt"], *par, *dims, y=v["y"])


def test_ssd_reduce_fwd_rejects_misaligned_layernorm_output(no_launch):
    B, L, H, P, N, G = 1, 8, 16, 4, 8, 1
    M = B * L
    par = [torch.zeros(H, device=DEV) for _ in range(3)]
    lw = torch.ones(H * P, device=DEV)
    with pytest.raises(RuntimeError, match="ssd_reduce_fwd: x, B, C, y and the LayerNorm output must be aligned"):
        ops.k_ssd_fwd(_ok(M, H * P), _ok(M, G * N), _ok(M, G * N), _ok(M, H), *par, B, L, H, P, N, G, y=_ok(M, H * P), ln=(lw, lw, _off2(M, H * P), 1e-5))


@pytest.mark.parametrize("bad", ["dy", "x", "Bm", "Cm", "dx", "dBm", "dCm"])
def test_ssd_reduce_bwd_rejects_misaligned(bad, no_launch):
    v, par, dims = _ssd_operands(bad)
    kv = torch.zeros((1, 4, 8, 4), device=DEV)
    with pytest.raises(RuntimeError, match="ssd_reduce_bwd: dy, x, B, C and their gradients must be aligned"):
        ops.k_ssd_bwd(v["dy"], v["x"], v["Bm"], v["Cm"], v["dt"], *par, kv, v["dx"], v["dBm"], v["dCm"], v["ddt"], *dims)


@pytest.mark.parametrize("bad", ["dt", "ddt"])
def test_ssd_reduce_bwd_rejects_short_dt_rows(bad, no_launch):
    """dt_raw / d dt_raw are read and written one element at a time: no alignment asked, but a row must hold its H columns"""
    v, par, dims = _ssd_operands()
    kv = torch.zeros((1, 4, 8, 4), device=DEV)
    v[bad] = torch.zeros((8, 4), device=DEV)[:, :2].as_strided((8, 4), (2, 1))   # row stride 2 < H = 4
    with pytest.raises(RuntimeError, match="ssd_reduce_bwd: dt row strides smaller than the rows they address"):
        ops.k_ssd_bwd(v["dy"], v["x"], v["Bm"], v["Cm"], v["dt"], *par, kv, v["dx"], v["dBm"], v["dCm"], v["ddt"], *dims)


def _scan_operands():
    B, L, H, P, N, G = 1, 8, 2, 4, 8, 1
    M = B * L
    v = {n: torch.zeros((M, C), device=DEV) for n, C in (("x", H * P), ("Bm", G * N), ("Cm", G * N), ("dt", H), ("y", H * P), ("dy", H * P),
                                                         ("dx", H * P), ("dBm", G * N), ("dCm", G * N), ("ddt", H))}
    par = [torch.zeros(H, device=DEV) for _ in range(3)]
    return v, par, (B, L, H, P, N, G, 4, False)


def _short(t, ld):
    """the same rows read with a row stride smaller than the row (never launched: the entry point refuses it)"""
    return t.as_strided(t.shape, (ld, 1))


@pytest.mark.parametrize("bad", ["x", "Bm", "Cm", "dt", "y", "xhs", "yhs", "dths"])
def test_ssd_scan_fwd_rejects_short_strides(bad, no_launch):
    v, par, dims = _scan_operands()
    hs = dict(xhs=4, yhs=4, dths=1)
    if bad in hs:
        hs[bad] = 0 if bad == "dths" else 2
        msg = "ssd_scan_fwd: head strides smaller than a head"
    else:
        v[bad] = _short(v[bad], v[bad].shape[1] - 1)
        msg = "ssd_scan_fwd: row strides smaller than the rows they address"
    with pytest.raises(RuntimeError, match=msg):
        ops.k_ssd_scan_fwd(v["x"], hs["xhs"], v["Bm"], v["Cm"], v["dt"], hs["dths"], *par, 1, v["y"], hs["yhs"], *dims)


@pytest.mark.parametrize("bad", ["dy", "x", "Bm", "Cm", "dt", "dx", "dBm", "dCm", "ddt", "dyhs", "xhs", "dxhs", "dths", "ddths"])
def test_ssd_scan_bwd_rejects_short_strides(bad, no_launch):
    v, par, dims = _scan_operands()
    hs = dict(dyhs=4, xhs=4, dxhs=4, dths=1, ddths=1)
    if bad in hs:
        hs[bad] = 0 if bad in ("dths", "ddths") else 2
        msg = "ssd_scan_bwd: head strides smaller than a head"
    else:
        v[bad] = _short(v[bad], v[bad].shape[1] - 1)
        msg = "ssd_scan_bwd: row strides smaller than the rows they address"
    S_in = torch.zeros((1, 2, 2, 4, 8), device=DEV)
    with pytest.raises(RuntimeError, match=msg):
        ops.k_ssd_scan_bwd(v["dy"], hs["dyhs"], v["x"], hs["xhs"], v["Bm"], v["Cm"], v["dt"], hs["dths"], *par, 1, S_in, v["dx"], hs["dxhs"], v["dBm"],
                           v["dCm"], v["ddt"], hs["ddths"], *dims)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_gate_rejects_misaligned(dtype, made):
    M, Fh = 8, 8
    st = torch.cuda.current_stream().cuda_stream
    dt = ops._dt(torch.zeros(0, dtype=dtype))
    h, hb, y, yb = _ok(M, 2 * Fh, dtype), _off2(M, 2 * Fh, dtype), _ok(M, Fh, dtype), _off2(M, Fh, dtype)
    dh, dhb = _ok(M, 2 * Fh, dtype), _off2(M, 2 * Fh, dtype)
    p = lambda t: (t.data_ptr(), t.stride(0))
    for hh, yy in ((hb, y), (h, yb)):
        with pytest.raises(RuntimeError, match="gate_fwd: h and y must be aligned to 4 elements"):
            lib.call("adnm_gate_fwd", *p(hh), *p(yy), M, Fh, dt, st)
    for gy, hh, gh in ((yb, h, dh), (y, hb, dh), (y, h, dhb)):
        with pytest.raises(RuntimeError, match="gate_bwd: dy, h and dh must be aligned to 4 elements"):
            lib.call("adnm_gate_bwd", *p(gy), *p(hh), *p(gh), M, Fh, dt, st)
    assert made == ["adnm_gate_fwd"] * 2 + ["adnm_gate_bwd"] * 3


def test_catmix_rejects_misaligned(made):
    M, d = 8, 8
    st = torch.cuda.current_stream().cuda_stream
    one = torch.ones((), device=DEV)
    good, bad, y = _ok(M, d), _off2(M, d), torch.zeros((M + 1, 2 * d), device=DEV)
    p = lambda t: (t.data_ptr(), t.stride(0)) if t is not None else (None, 0)
    al = (one.data_ptr(),) * 4
    for k in range(3):
        v = [bad if i == k else good for i in range(3)]
        with pytest.raises(RuntimeError, match="catmix_fwd: the operands must be aligned to 4 elements"):
            lib.call("adnm_catmix_fwd", *p(v[0]), *p(v[1]), *p(v[2]), *al, y.data_ptr(), M, d, lib.F32, st)
    with pytest.raises(RuntimeError, match="catmix_fwd: the output must be non-null and aligned to 4 elements"):
        lib.call("adnm_catmix_fwd", *p(good), *p(good), None, 0, *al, y.data_ptr() + 8, M, d, lib.F32, st)
    nb = lib.query("adnm_catmix_bwd_ws_bytes", M, d)
    ws, da, g = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV), torch.zeros(4, device=DEV), torch.zeros((M, d), device=DEV)
    dyok, dybad = _ok(M, 2 * d), _off2(M, 2 * d)
    for dy, grads in ((dybad, (g, g, g)), (dyok, (bad, g, g)), (dyok, (g, bad, g)), (dyok, (g, g, bad))):
        with pytest.raises(RuntimeError, match="catmix_bwd: dy and the gradients must be aligned to 4 elements"):
            lib.call("adnm_catmix_bwd", *p(dy), *p(good), *p(good), *p(good), *al, *[t.data_ptr() for t in grads], da.data_ptr(), ws.data_ptr(), nb,
                     M, d, lib.F32, st)
    assert made == ["adnm_catmix_fwd"] * 4 + ["adnm_catmix_bwd"] * 4


def test_lincomb_rejects_misaligned_and_ragged_gradient_strides(made):
    M, C = 8, 8
    st = torch.cuda.current_stream().cuda_stream
    good, bad = _ok(M, C), _off2(M, C)
    p = lambda t: (t.data_ptr(), t.stride(0))
    for k in range(3):
        v = [bad if i == k else good for i in range(3)]
        with pytest.raises(RuntimeError, match="lincomb_fwd: the operands must be aligned to 4 elements"):
            lib.call("adnm_lincomb_fwd", *p(v[0]), *p(v[1]), *p(v[2]), None, None, None, None, *p(good), M, C, lib.F32, st)
    with pytest.raises(RuntimeError, match="lincomb_fwd: the output must be aligned to 4 elements"):
        lib.call("adnm_lincomb_fwd", *p(good), None, 0, None, 0, None, None, None, None, *p(bad), M, C, lib.F32, st)
    nb = lib.query("adnm_lincomb_bwd_ws_bytes", M, C)
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
    bwd = lambda dy, dxs: lib.call("adnm_lincomb_bwd", *p(dy), *p(good), *p(good), *p(good), None, None, None, None, *dxs[0], *dxs[1], *dxs[2],
                                   None, None, None, None, ws.data_ptr(), nb, M, C, lib.F32, st)
    with pytest.raises(RuntimeError, match="lincomb_bwd: the operands must be aligned"):
        lib.call("adnm_lincomb_bwd", *p(good), *p(bad), *p(good), *p(good), None, None, None, None, *p(good), *p(good), *p(good),
                 None, None, None, None, ws.data_ptr(), nb, M, C, lib.F32, st)
    for k in range(3):   # a gradient row stride that is no multiple of 4: rows 1, 2, 3 would be misaligned
        dxs = [(good.data_ptr(), C + 2) if i == k else p(good) for i in range(3)]
        with pytest.raises(RuntimeError, match="lincomb_bwd: gradient row strides must be >= C and multiples of 4"):
            bwd(good, dxs)
    for dy, k in ((bad, -1), (good, 0), (good, 1), (good, 2)):
        dxs = [p(bad) if i == k else p(good) for i in range(3)]
        with pytest.raises(RuntimeError, match="lincomb_bwd: dy and the gradients must be aligned to 4 elements"):
            bwd(dy, dxs)
    assert made == ["adnm_lincomb_fwd"] * 4 + ["adnm_lincomb_bwd"] * 8


def test_mixnorm_rejects_misaligned(made):
    M, d = 8, 8
    st = torch.cuda.current_stream().cuda_stream
    good, bad = _ok(M, d), _off2(M, d)
    w, rstd = torch.ones(d, device=DEV), torch.ones(M, device=DEV)
    p = lambda t: (t.data_ptr(), t.stride(0)) if t is not None else (None, 0)
    fwd = lambda x0, x1, ym, yn: lib.call("adnm_mixnorm_fwd", *p(x0), *p(x1), None, None, None, w.data_ptr(), None, None, None, *p(ym), *p(yn),
                                          None, rstd.data_ptr(), M, d, 1e-5, 0, st)
    for x0, x1 in ((bad, good), (good, bad)):
        with pytest.raises(RuntimeError, match="mixnorm_fwd: the operands must be 16-byte aligned"):
            fwd(x0, x1, good, good)
    for ym, yn in ((bad, good), (good, bad)):
        with pytest.raises(RuntimeError, match="mixnorm_fwd: the outputs must be 16-byte aligned"):
            fwd(good, good, ym, yn)
    nb = lib.query("adnm_mixnorm_bwd_ws_bytes", M, d)
    ws, dw = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV), torch.zeros(d, device=DEV)
    bwd = lambda dyn, dres, x0, dx0, dx1: lib.call("adnm_mixnorm_bwd", *p(dyn), *p(dres), *p(x0), *p(good), None, None, None, w.data_ptr(), None, None,
                                                   None, rstd.data_ptr(), *p(dx0), *p(dx1), None, None, None, dw.data_ptr(), None, None, None,
                                                   ws.data_ptr(), nb, M, d, 0, st)
    with pytest.raises(RuntimeError, match="mixnorm_bwd: the operands must be 16-byte aligned"):
        bwd(good, None, bad, good, good)
    for a in ((bad, None, good, good, good), (good, bad, good, good, good), (good, None, good, bad, good), (good, None, good, good, bad)):
        with pytest.raises(RuntimeError, match="mixnorm_bwd: the gradients must be 16-byte aligned"):
            bwd(*a)
    assert made == ["adnm_mixnorm_fwd"] * 4 + ["adnm_mixnorm_bwd"] * 5
