"""The output contract of the kernels: a launch writes EVERY element of every output, saved statistic, intermediate and gradient buffer it is
handed, whatever the memory held before; and a step, a graph replay or a scored batch does not depend on the one before it.

Nearly every such buffer is torch.empty from the caching allocator — in this suite usually the block the same op freed a moment ago, holding
last call's right numbers — FlatTrainer's flat gradient buffer is zeroed once and then written in place step after step, and the captured
graphs keep their intermediates at fixed addresses.  An element a grid, a tail or an early exit skips is invisible to a test that pins values.

1. Every op runs three times on the same inputs: as the suite runs it, and under util.poisoned_outputs with pattern 0 and pattern 1, where
   torch.empty / torch.empty_like of the wrapper modules return memory filled with a payload NaN (0x5A.. / 0xA5.. bytes for integer types).
   Every returned output and gradient must be the first run's BIT FOR BIT and free of NaN, and no allocation may keep an element that holds
   pattern 0 in run 0 and pattern 1 in run 1 (util.unwritten) unless its (site, role) is on ALLOW below.  The kernels are specified bitwise
   reproducible and without float atomics, and the other test files pin the first run to the fp64 oracle: there is no tolerance in this file.
2. FlatTrainer: the gradient slices (and the accumulator of accum_steps = 2) filled with the payload NaN before a step give the bits of a
   step from zeros, no payload is left, and the alignment padding between the slices (summed into the norm) is still zero.
3. A step after any predecessor — none, another batch three times as bright, itself — gives the same loss, gradient and parameters, eagerly
   and through the captured graphs in f32, bf16 and fp8; Validator and Forecaster after other batches and a reset give what a first batch gives.

Shapes: the cases of tests/test_workspace_contract_gpu.py (the smallest that reach each plan, ragged tails included), and for the ops that
take no workspace the smallest with a ragged tail in the loops of their launch code (noted at the table).  Every case prints one line
`[out-contract] op shape allocations sites verdict` (profiles/output_contract.txt is that output of one run).

A finding is one of three: the kernel must write the element (fix the grid or the tail); the kernel accumulates by contract (the host
allocates zeros at that site); the element is never read by any kernel or torch op (an ALLOW entry with its reason).

Found by this file and fixed with it (all three were buffers the host allocated and nothing ever read — the third kind — and each was
removed instead of being put on the allow-list):
  * k_rownorm_fwd handed RMSNorm (mean=False) a one-element `mu` that neither rownorm kernel reads or writes, and saved it for backward;
    it is None now, as in mixnorm.
  * Conv3Fn / ConvT2xFn asked the gradient registry for a weight gradient in the channels-last order they write, got a fresh NCHW tensor
    for a weight no trainer had registered, dropped it unwritten and allocated a second one; GradRegistry.take allocates fresh memory in
    the layout it was asked for.
  * ResidentDataset made its pinned order / words images as torch.empty(N).pin_memory(): a pageable tensor nobody wrote, copied into the
    pinned one; they are allocated pinned.
On the allow-list: the one element behind the storage-less handle of a projection the mixer prep writes only as its narrow copy.
No kernel was found to skip an element of an output, a gradient slice or a graph intermediate at these shapes."""
import pytest
import torch

from adnm_hip import lib, ops, recipe
from test_workspace_contract_gpu import CASES, Case, same_bits
from util import bits, pattern_mask, poison_bits, poisoned_outputs, unwritten

pytestmark = pytest.mark.gpu
DEV = "cuda"
NONE, SILU, GELU = lib.ACT_NONE, lib.ACT_SILU, lib.ACT_GELU
F32, BF16 = torch.float32, torch.bfloat16

# {(caller site, buffer role): reason}.  Only for elements that no kernel and no torch op ever reads; never a returned output, a returned
# gradient or a saved-for-backward statistic.  test_every_allow_list_entry_was_hit fails on an entry no case reaches.
ALLOW = {
    ("ops.py <lambda>", "handle"): "AdnPrepMultiFn's storage-less (N, K) handle of a matrix written only as its bf16 / e4m3 copy: one element expanded to "
                                   "carry shape and autograd edge; the GEMMs read the narrow copy, no kernel or torch op reads or writes the element",
}
_HIT, _RAN = set(), set()


def T(name, shape, scale=1.0):
    return recipe.tensor("outc." + name, shape, scale)


def check_outputs(monkeypatch, op, shape, run):
    """run() -> [(name, tensor)] three times: plain, under pattern 0, under pattern 1; prints the record line"""
    plain = run()
    recs, got = [], []
    for pattern in (0, 1):
        with poisoned_outputs(monkeypatch, pattern) as p:
            got.append(run())
        recs.append(p.records)
    torch.cuda.synchronize()
    found = unwritten(recs[0], recs[1])
    for key in found:
        if key in ALLOW:
            _HIT.add(key)
    bad = {k: v for k, v in found.items() if k not in ALLOW}
    diffs = []
    for g in got:
        assert [n for n, _ in plain] == [n for n, _ in g]
        for (name, a), (_, b) in zip(plain, g):
            if b.is_floating_point() and bool(torch.isnan(b.float()).any()):
                diffs.append(f"{name} holds a NaN")
            elif not same_bits(a, b):
                diffs.append(f"{name} differs from the plain run")
    sites = sorted({r[1] for r in recs[0]})
    verdict = "all written" if not (bad or diffs) else "UNWRITTEN" if bad else "DIFFERS"
    print(f"[out-contract] {op:<22} {'x'.join(str(s) for s in shape):<30} allocations {len(recs[0]):<5} sites {len(sites):<4} {verdict}"
          + (f"   allowed {sorted(k for k in found if k in ALLOW)}" if len(found) > len(bad) else ""))
    _RAN.add((op, tuple(shape)))
    lines = [f"{site} [{where}] `{role}`: {n} elements no kernel wrote, the first at flat index {first}" for (site, role), (n, where, first) in bad.items()]
    assert not lines and not diffs, f"{op} {shape}: " + "; ".join(lines + sorted(set(diffs)))
    return recs[0]


# ================================================================================================ the cases the workspace table lacks
class Run:
    """a case that is not one op on leaves: run() -> [(name, tensor)] made by make() once"""

    def __init__(self, op, shape, make, prec=None, patch=()):
        self.op, self.shape, self._make, self.prec, self.patch, self._run = op, shape, make, prec, patch, None
        self.id = f"{op}-{'x'.join(str(s) for s in shape)}"
        self.env, self.plan = (), None

    def run(self):
        if self._run is None:
            self._run = self._make()
        out = self._run()
        torch.cuda.synchronize()
        return out


def _prec(case, prec, patch=()):
    case.prec, case.patch = prec, tuple(case.patch) + tuple(patch)
    case.id += "-" + prec
    case.shape = tuple(case.shape) + (prec,)
    return case


def _act(n, code):
    return Case("act", (n, "gelu" if code == GELU else "silu"), lambda: [T(f"act.x{n}", (n,), 3.0)], lambda x: ops.act(x, code))


def _gate(M, F2, dtype):
    return Case("gate", (M, F2, "bf16" if dtype == BF16 else "f32"), lambda: [T(f"gate.h{M}.{F2}", (M, F2), 3.0).to(dtype)], ops.gate)


def _emul(M, C):
    """column slices of wider matrices, as Vssd's gate form passes them (tests/test_kernels_gpu.py::test_emul_column_slices)"""
    return Case("emul", (M, C), lambda: [T(f"em.a{M}", (M, 28), 2.0), T(f"em.b{M}", (M, 20), 0.5)], lambda a, b: ops.emul(a[:, :C], b[:, 8:8 + C]))


def _chanpad(B, L, Cin, Cout):
    return Case("chanpad", (B, L, Cin, Cout), lambda: [T(f"cp.x{L}.{Cin}", (B, L, Cin))], lambda x: ops.chanpad(x, Cout))


def _maxpool(B, H, W, C, kh, kw, stride, tap=False):
    return Case("maxpool" + ("_tap" if tap else ""), (B, H, W, C, kh, kw, stride), lambda: [T(f"mp.x{H}.{W}.{C}", (B, H * W, C))],
                lambda x: ops.maxpool(x, H, W, kh, kw, stride, tap=tap))


def _pyramid(H, W, levels):
    shapes, (h, w) = [], (H, W)
    for _ in range(levels):
        shapes.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return shapes


def _haar(B, H, W, C, levels):
    shapes = _pyramid(H, W, levels)

    def ins():
        bands = [T(f"hs.{i}.{H}", (B * ((h + 1) // 2) * ((w + 1) // 2), 4 * C)) for i, (h, w) in enumerate(shapes)]
        return [T(f"hs.x{H}", (B * H * W, C)), T(f"hs.a{H}", (B * H * W, C)), T(f"hs.b{H}", (B * H * W, C))] + bands

    def f(x, a, b, *bands):
        dwt = ops.k_haar_dwt(x, B, H, W, C)
        h2, w2 = (H + 1) // 2, (W + 1) // 2
        return (dwt, ops.k_haar_dwt(dwt, B, h2, w2, C, 4), ops.k_haar_idwt(dwt, None, B, H, W, C),
                ops.k_haar_idwt(bands[0], None, B, H, W, C, y_add=(a, b)), ops.k_haar_synthesis(list(bands), shapes, B, C, y_add=(a, b)),
                ops.k_haar_synthesis(list(bands), shapes, B, C))
    return Case("haar", (B, H, W, C, levels), ins, f, grad=False)


def _wtconv(B, H, W, C, K, levels, bias):
    ins = lambda: ([T(f"wt.x{H}.{C}", (B, H * W, C)), T(f"wt.bw{C}.{K}", (K * K, C), 0.3), T(f"wt.bb{C}", (C,), 0.2) if bias else None]
                   + [T(f"wt.l{i}.{C}.{K}", (K * K, 4 * C), 0.3) for i in range(levels)])
    return Case("wtconv", (B, H, W, C, K, levels, int(bias)), ins, lambda x, bw, bb, *lw: ops.wtconv(x, H, W, K, bw, bb, list(lw), tap=True))


def _ssd_bf16(B, L, H, P, N, G):
    """the bf16 storage of tests/test_kernels_gpu.py::test_bf16_storage_paths (forward; bf16 rows in, bf16 rows out)"""
    tag = f"ssdb{L}."
    ins = lambda: [T(tag + "x", (B, L, H, P)).to(BF16), T(tag + "B", (B, L, G * N)).to(BF16), T(tag + "C", (B, L, G * N)).to(BF16),
                   (T(tag + "dt", (B, L, H)) - 3).to(BF16), torch.zeros(H), torch.ones(H), torch.ones(H)]
    return Case("ssd_reduce_bf16", (B, L, H, P, N, G), ins, lambda *a: ops.ssd_reduce(*a, G), grad=False)


def _conv1d3(B, n):
    return Case("conv1d3", (B, n), lambda: [T(f"c1.x{n}", (B, 1, n)), torch.tensor([[[0.3, -0.8, 0.5]]]), torch.tensor([0.1])], ops.conv1d3)


def _attn4(B, L, heads):
    return Case("attn4", (B, L, heads), lambda: [T(f"at.q{L}.{heads}", (B, L, 12 * heads), 1.5)], lambda q: ops.attn4(q, heads, 0.5))


def _feedforward(B, H, W, d, bias):
    def ins():
        b = [T("ff.bi", (4 * d,), 0.2), T("ff.bd", (4 * d,), 0.2), T("ff.bo", (d,), 0.2)] if bias else [None, None, None]
        return [T("ff.x", (B, H * W, d)), T("ff.wi", (4 * d, d), 0.3), b[0], T("ff.dw", (4 * d, 1, 3, 3), 0.5), b[1], T("ff.wo", (d, 2 * d), 0.3), b[2]]
    return Case("feedforward", (B, H, W, d, int(bias)), ins, lambda *a: ops.feedforward(*a, H, W))


def _linear(M, K, N, prec):
    """ops.linear in the bf16 and fp8 modes; fp8 with explicit scales (a power of two each: any scale is a valid one, values beyond fmax
    saturate), written for the leaves of each run"""
    def f(x, w, b):
        if prec == "fp8":
            ops.QUANT.set(x.device, w.data_ptr(), "linear_fwd", 64.0, 1024.0)
            ops.QUANT.set(x.device, w.data_ptr(), "linear_dgrad", 4096.0, 1024.0)
        return ops.linear(x, w, b)
    c = Case("linear", (M, K, N), lambda: [T(f"lp.x{M}.{K}", (M, K)), T(f"lp.w{N}.{K}", (N, K), 0.05), T(f"lp.b{N}", (N,))], f)
    return _prec(c, prec, patch=((ops, "TS_MIN_ROWS", 64),) if M == 4099 else ())


def _conv3(B, H, W, K, N, prec):
    def f(x, w, b):
        if prec == "fp8":
            ops.QUANT.set(x.device, w.data_ptr(), "conv3_fwd", 64.0, 256.0)
            ops.QUANT.set(x.device, w.data_ptr(), "conv3_dgrad", 4096.0, 256.0)
        return ops.conv3(x, w, b, H, W, GELU)
    c = Case("conv3", (B, H, W, K, N), lambda: [T(f"c3.x{H}.{W}.{K}", (B, H * W, K)), T(f"c3.w{N}.{K}", (N, K, 3, 3), 0.2), T(f"c3.b{N}", (N,))], f)
    return _prec(c, prec)


def _convt2x(B, H, W, C, cl):
    def ins():
        w = T(f"ct.w{C}", (C, C, 3, 3), 0.2)
        if cl:
            w = w.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        return [T(f"ct.x{H}.{W}.{C}", (B, H * W, C)), w, T(f"ct.b{C}", (C,))]
    return Case("convt2x", (B, H, W, C, int(cl)), ins, lambda x, w, b: ops.convt2x(x, w, b, H, W))


def _module_run(mods_fn, inputs_fn, forward):
    """modules made and filled once; run(): forward(mods, *leaves) -> outputs; cotangents from recipe.tensor; outputs, input and parameter gradients"""
    def make():
        mods = mods_fn()
        net = torch.nn.ModuleList(mods)
        recipe.fill_parameters(net)
        net.to(DEV).train()
        ins = [t.to(DEV) for t in inputs_fn()]

        def run():
            net.zero_grad(set_to_none=True)
            leaves = [t.clone().requires_grad_(True) for t in ins]
            outs = forward(mods, *leaves)
            outs = list(outs) if isinstance(outs, (tuple, list)) else [outs]
            torch.autograd.backward(outs, [T(f"mod.cot{i}.{'.'.join(map(str, o.shape))}", tuple(o.shape)).to(DEV) for i, o in enumerate(outs)])
            return ([(f"out{i}", o.detach()) for i, o in enumerate(outs)] + [(f"din{i}", l.grad) for i, l in enumerate(leaves)]
                    + [(k, p.grad) for k, p in net.named_parameters() if p.grad is not None])
        return run
    return make


def _adn_mixer(B, H, W, d, prec=None):
    from models.ADNssd import Mamba2
    return Run("adn_mixer", (B, H, W, d) + ((prec,) if prec else ()), prec=prec, make=_module_run(lambda: [Mamba2(d_model=d, headdim=4)], lambda: [T(f"adn.u{H}.{W}", (B, H * W, d))],
                                                      lambda mods, u: mods[0](u, H, W)))


def _vssd_mixer(B, H, W, d):
    from models.Vssd import Mamba2
    return Run("vssd_mixer", (B, H, W, d), _module_run(lambda: [Mamba2(d_model=d, headdim=4)], lambda: [T(f"vssd.u{H}.{W}", (B, H * W, d))],
                                                       lambda mods, u: mods[0](u, H, W)))


def _prep_group(B, H, W, d, prec=None):
    """two mixers and two WTConv2d behind ONE grouped parameter prep per kind (tests/test_paramprep_gpu.py::test_prep_group_matches_per_module)"""
    from models.ADNssd import Mamba2
    from models.WTConv2d import WTConv2d

    def forward(mods, u):
        ops.prep_group(torch.nn.ModuleList(mods))
        for m in mods:
            u = m(u, H, W) if isinstance(m, Mamba2) else m.forward_tokens(u, H, W)
        return u
    return Run("prep_group_chain", (B, H, W, d) + ((prec,) if prec else ()), prec=prec,
               make=_module_run(lambda: [Mamba2(d_model=d, headdim=4), WTConv2d(d, d, 5, 1, True, wt_levels=2), Mamba2(d_model=d, headdim=4),
                                    WTConv2d(d, d, 3, 1, False, wt_levels=1)], lambda: [T(f"pg.u{H}.{W}", (B, H * W, d))], forward))


def _e2d(instance_norm, prec):
    """the grouped EncoderToDecoder node at the shapes of tests/test_e2d_group_gpu.py::test_node_equals_three_module_calls"""
    def make():
        import test_e2d_group_gpu as E
        mods, xs, gates, cots = E._chains([256, 256, 512], [2, 4, 3], instance_norm)

        def run():
            outs, dxs, dgs, grads = E._run(mods, xs, gates, cots, True, False)
            return ([(f"out{i}", o.detach()) for i, o in enumerate(outs)] + [(f"dx{i}", g) for i, g in enumerate(dxs)] + [(f"dres{i}", g) for i, g in enumerate(dgs)]
                    + [(k, g) for k, g in sorted(grads.items()) if g is not None])
        return run
    return Run("e2d_group", (256, 256, 512, "in" if instance_norm else "gn4", prec), make, prec=prec)


def _cast(n):
    """adnm_cast_f32_bf16 / adnm_cast_bf16_f32 as FlatTrainer._cast calls them (csrc/optim.hip: 8 elements per lane, 256 lanes, at most 4096
    workgroups, then a grid stride): a tail alone, two workgroups with a tail, past the cap; the destinations come from the poisoned allocator"""
    def make():
        src = T(f"cast.{min(n, 4099)}", (min(n, 4099),), 2.0).to(DEV).repeat(-(-n // min(n, 4099)))[:n].contiguous()
        st = lambda: torch.cuda.current_stream().cuda_stream

        def run():
            wire = ops.torch.empty(n, dtype=BF16, device=DEV)
            lib.call("adnm_cast_f32_bf16", src.data_ptr(), wire.data_ptr(), n, 1.0, st())
            back = ops.torch.empty(n, dtype=F32, device=DEV)
            lib.call("adnm_cast_bf16_f32", wire.data_ptr(), back.data_ptr(), n, 0.5, st())
            return [("wire", wire), ("back", back)]
        return run
    return Run("cast", (n,), make)


EXTRA = [
    # act / emul / chanpad: one float4 (or element) per lane over a capped grid stride (csrc/activation.hip, elementwise.hip: grid_for), act with
    # a scalar tail of n % 4 elements written by workgroup 0: one lane's worth, two workgroups, many; 1031 has the tail
    _act(4, GELU), _act(1028, SILU), _act(1031, GELU), _act(20004, GELU), _act(20004, SILU),
    _gate(100, 72, F32), _gate(1000, 256, F32), _gate(100, 72, BF16), _gate(1000, 256, BF16),
    _emul(301, 12), _chanpad(2, 77, 12, 16), _chanpad(2, 77, 16, 12),
    # pools: odd maps (a window cut by the border), the overlapping 3 x 3 / 1 form, and the tap variant that returns the input's alias
    _maxpool(2, 9, 7, 8, 2, 2, 2), _maxpool(1, 5, 6, 12, 3, 3, 1), _maxpool(2, 9, 7, 8, 2, 2, 2, tap=True),
    # the Haar pair, the three-level synthesis cascade and its addends on odd maps (every level ragged), and WTConv2d's node on them: the
    # fused level kernels (K = 3, 5) with and without bias
    _haar(1, 37, 51, 8, 3), _haar(2, 19, 23, 12, 2), _wtconv(1, 11, 13, 4, 3, 3, True), _wtconv(1, 20, 28, 8, 5, 2, False),
    _ssd_bf16(2, 70, 16, 4, 16, 2),
    # conv1d3 is one workgroup that walks B rows of n: n no multiple of its lanes; attn4 has cdiv(L, 64) query tiles per (sample, head)
    _conv1d3(3, 1001), _conv1d3(4, 2144), _attn4(1, 100, 3), _attn4(2, 64, 64),
    _feedforward(1, 9, 13, 16, True), _feedforward(1, 9, 13, 16, False),
    _adn_mixer(1, 3, 5, 32), _adn_mixer(2, 6, 10, 64), _adn_mixer(2, 6, 10, 64, "bf16"), _vssd_mixer(1, 3, 5, 32), _prep_group(2, 5, 7, 32),
    _prep_group(2, 5, 7, 64, "bf16"),   # in_proj / out_proj above 8192 elements: written only as their bf16 copies (the allow-list's handle)
    # the narrow-operand GEMMs and convs: a split weight gradient, the tall-skinny kernels (TS_MIN_ROWS lowered as in the workspace table)
    _linear(300, 20, 64, "bf16"), _linear(4099, 48, 40, "bf16"), _linear(300, 20, 64, "fp8"), _linear(4099, 48, 40, "fp8"),
    _conv3(1, 7, 9, 8, 6, "f32"), _conv3(1, 7, 9, 8, 6, "fp8"), _convt2x(2, 6, 10, 16, False), _convt2x(2, 6, 10, 16, True),
    _e2d(True, "f32"), _e2d(False, "bf16"),
    _cast(5), _cast(2051), _cast(8 * 256 * 4096 + 8 + 3),
]


class _Mode:
    """the GEMM precision of a case, and a fresh quantisation table around an fp8 one"""

    def __init__(self, prec):
        self.prec = prec

    def __enter__(self):
        if self.prec is not None:
            ops.QUANT.reset()
            ops.set_mfma_precision(self.prec)
            self.rows, ops.QUANT.max_rows = ops.QUANT.max_rows, 1 << 30

    def __exit__(self, *exc):
        if self.prec is not None:
            ops.QUANT.max_rows = self.rows
            ops.set_mfma_precision("f32")
            ops.QUANT.reset()
        return False


def _check_case(case, monkeypatch):
    for obj, name, value in case.patch:
        monkeypatch.setattr(obj, name, value)
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    if case.plan is not None:
        case.plan()
    with _Mode(getattr(case, "prec", None)):
        check_outputs(monkeypatch, case.op, case.shape, case.run)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_workspace_table_cases_write_their_outputs(case, monkeypatch):
    _check_case(case, monkeypatch)


@pytest.mark.parametrize("case", EXTRA, ids=lambda c: c.id)
def test_other_ops_write_their_outputs(case, monkeypatch):
    _check_case(case, monkeypatch)


def test_case_ids_are_unique():
    assert len({c.id for c in EXTRA}) == len(EXTRA)


# ================================================================================================ scoring, rendering and feed ops (no gradient)
def _pair(frames, H, W, tag):
    shape = (frames, H, W)
    return recipe.tensor(f"outc.{tag}.t", shape, 1.2).abs().to(DEV), recipe.tensor(f"outc.{tag}.p", shape, 1.2).abs().to(DEV)


def _blobs(frames, H, W, tag):
    """smooth fields with echoes that move: block matching, labelling and the spectra have something to find"""
    return recipe.radar_batch(1, 2 * frames, max(H, W), name="outc." + tag)[0, :, 0, :H, :W].mul(255.0 / 70.0).contiguous().to(DEV).view(2, frames, H, W)


THR = [20.0, 30.0, 35.0, 40.0]


def _fss(frames, H, W):
    t, p = _pair(frames, H, W, "fss")
    return lambda: [("sums", ops.fss_sums(t, p, THR, 255.0, (1, 5, 17)))]


def _trec(n, H, W, block, radius):
    prev, last = _blobs(n, H, W, "trec")

    def run():
        m, c = ops.trec_motion(prev, last, 255.0, block, radius, 4, return_costs=True)
        u, m2 = ops.trec_flow(prev, last, 255.0, block, radius, 4, return_motion=True)
        return [("motion", m), ("costs", c), ("advect", ops.advect(last, m, block, 3)), ("flow", u), ("motion2", m2), ("flow_only", ops.trec_flow(prev, last, 255.0, block, radius, 4)),
                ("field", ops.flow_field(u, block, H, W)), ("advect_flow", ops.advect_flow(last, u, block, 3)),
                ("extrapolate", ops.extrapolate(torch.stack((prev, last), 1), 2, 255.0, block, radius))]
    return run


def _spectrum(frames, H, W):
    t, p = _pair(frames, H, W, "spec")
    return lambda: [("spectrum", ops.power_spectrum(t, p, 255.0))]


def _joint(frames, H, W, scale):
    t, p = _pair(frames, H, W, "joint")
    return lambda: [("joint", ops.joint_histogram(t, p, scale))]


def _objects(frames, H, W):
    t, p = _blobs(frames, H, W, "obj")
    return lambda: [("stats", ops.object_stats(t, p, [10.0, 20.0], 255.0)), ("stats3", ops.object_stats(t, p, [10.0], 255.0, min_area=3)),
                    ("labels", ops.label_objects(t, 10.0, 255.0)), ("labels3", ops.label_objects(p, 10.0, 255.0, min_area=3))]


def _render(B, Tn, H, W):
    import numpy as np
    pred = recipe.tensor("outc.render", (B, Tn, H, W), 0.4).abs().to(DEV)
    rgba = (np.arange(4 * 5, dtype=np.int64).reshape(5, 4) * 37 % 256).astype(np.uint8)
    rgba[1] = (0x5A, 0xA5, 0x5A, 0xA5)   # colours that ARE the two byte patterns: a written byte may hold either
    tables = ops.render_tables([0.0, 10.0, 20.0, 35.0, 50.0, 256.0], rgba)

    def run():
        f, s = ops.forecast_render_tables(pred, tables, 255.0, 1, 2, 3)
        f0, s0 = ops.forecast_render_tables(pred, tables, 0.0, 0, 1, 0)
        return [("fields", f), ("strip", s), ("bins", f0), ("strip0", s0)]
    return run


def _evaluator(B, Tn, H, W):
    from adnm_hip.evaluator import GpuEvaluator
    t, p = (v.view(B, Tn, H, W) for v in _pair(B * Tn, H, W, "eval"))

    def run():
        ev = GpuEvaluator(Tn, 255.0, THR)
        ev.evaluate(t, p)
        return [("counts", ev._tables[0][0])] + ([("ssim", ev._ssim[0][0])] if ev._ssim[0][0] is not None else [])
    return run


def _ingest(B, Tn, H0, W0, size):
    from adnm_hip import dataio
    raw = (recipe.tensor("outc.ingest", (B, Tn, H0, W0)).abs() * 255).to(torch.uint8).to(DEV)
    return lambda: [("frames", dataio.ingest(raw, size))]


def _feed(side, crop, augment):
    """ResidentDataset.fetch(): an odd side; a crop whose column offset is 1 (mod 4) on some samples (shift draws every offset over two
    epochs of 6 samples of a 9-column span) and the transpose bit (asserted on the epoch's words)"""
    from adnm_hip.dataio import TRANSPOSE, Augment, ResidentDataset, unpack_word
    frames = recipe.radar_batch(6, 7, side, name="outc.feed")

    def run():
        feed = ResidentDataset.from_frames(frames, 2, 3, DEV, generator=torch.Generator().manual_seed(5), crop=crop,
                                           augment=Augment(seed=3) if augment else None)
        out = []
        for epoch in range(2):
            feed.begin_epoch()
            if augment:
                words = [unpack_word(int(w)) for w in feed.words.words]
                out.append((f"words{epoch}", feed.words.words.clone()))
                run.ox1 |= any(ox % 4 == 1 for _, _, ox in words)
                run.transposed |= any(code & TRANSPOSE for code, _, _ in words)
            for i in range(len(feed)):
                x, tgt = feed.fetch()
                out += [(f"x{epoch}.{i}", x), (f"tgt{epoch}.{i}", tgt)]
        return out
    run.ox1 = run.transposed = False
    return run


ONESHOT = {
    "fss_sums-6x37x53": lambda: _fss(6, 37, 53),
    "trec+advect+flow-3x37x53-b8r2": lambda: _trec(3, 37, 53, 8, 2),        # ragged last block row and column
    "trec+advect+flow-2x16x24-b8r2": lambda: _trec(2, 16, 24, 8, 2),        # whole blocks only
    "power_spectrum-3x8x8": lambda: _spectrum(3, 8, 8), "power_spectrum-2x16x8": lambda: _spectrum(2, 16, 8),
    "joint_histogram-3x37x53-L2": lambda: _joint(3, 37, 53, 1.0), "joint_histogram-3x37x53-L91": lambda: _joint(3, 37, 53, 90.0),
    "objects-2x1x1": lambda: _objects(2, 1, 1), "objects-2x9x7": lambda: _objects(2, 9, 7), "objects-2x33x31": lambda: _objects(2, 33, 31),
    "forecast_render-2x5x9x7": lambda: _render(2, 5, 9, 7), "forecast_render-1x4x37x53": lambda: _render(1, 4, 37, 53),
    "evaluator-2x3x17x19": lambda: _evaluator(2, 3, 17, 19), "evaluator-3x5x9x9": lambda: _evaluator(3, 5, 9, 9),   # 9 x 9: no SSIM window
    "ingest-2x3x37x53->32": lambda: _ingest(2, 3, 37, 53, 32), "ingest-1x2x64x64->33": lambda: _ingest(1, 2, 64, 64, 33),
    "feed-37-plain": lambda: _feed(37, None, False), "feed-37-crop28-aug": lambda: _feed(37, (28, 28), True),
}


@pytest.mark.parametrize("name", list(ONESHOT))
def test_one_shot_ops_write_their_outputs(name, monkeypatch):
    run = ONESHOT[name]()

    def synced():
        out = run()
        torch.cuda.synchronize()
        return out
    op, shape = name.split("-", 1)
    check_outputs(monkeypatch, op, tuple(shape.split("x")), synced)
    if name == "feed-37-crop28-aug":
        assert run.ox1 and run.transposed, "the draw holds no column offset of 1 (mod 4) or no transpose: pick another seed"


# ================================================================================================ one pass over the whole model
def _model(salt=0):
    from models.ADNMUNet import create_ADNMUNet
    m = create_ADNMUNet(5, 20, 6, img_size=64)
    recipe.fill_parameters(m, salt=salt)
    return m.to(DEV).train()


@pytest.mark.parametrize("prec", ["f32", "bf16", "fp8"])
def test_whole_model_writes_its_outputs(prec, monkeypatch):
    """the 64 x 64 model, forward + loss + backward, eagerly: the shapes and the strided views only real layers reach; in bf16 and fp8 the
    narrow operands and the bf16 storage of the wide intermediates (fp8: scales from one calibration pass, then fixed)"""
    from models.loss import enRainfallLoss
    model = _model()
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
    with _Mode(prec):
        ops.QUANT.max_rows = 8192   # (the model's own rule: bf16 operands above 8192 token rows)
        if prec == "fp8":
            ops.fp8_calibrate(x.device, run)
        recs = check_outputs(monkeypatch, "ADNMUNet-64", (2, 25, 64, 64, prec), run)
    sites = sorted({r[1] for r in recs})
    print(f"[out-contract] ADNMUNet-64 {prec} sites: {sites}")
    assert len(recs) >= 300 and len(sites) >= 20, (len(recs), len(sites))


# ================================================================================================ FlatTrainer: gradient slices and replay order
def _trainer(model, **kw):
    from adnm_hip.trainer import FlatTrainer
    from models.loss import enRainfallLoss
    return FlatTrainer(model, enRainfallLoss(0.57, 0.25, gamma=0.0), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, max_norm=0.025, **kw)


_data = {}


def _batches():
    """A, and B: other frames, three times as bright, so that every intermediate differs"""
    if "A" not in _data:
        for name, gain in (("A", 1.0), ("B", 3.0)):
            f = (recipe.radar_batch(2, 25, 64, name="outc.trainer." + name) * gain).to(DEV)
            _data[name] = (f[:, :5].contiguous(), f[:, 5:].contiguous())
    return _data["A"], _data["B"]


def _u8(t):
    return t.detach().contiguous().view(torch.uint8).clone() if t.dim() else t.detach().reshape(1).view(torch.uint8).clone()


class _Precision:
    def __init__(self, prec):
        self.prec = prec

    def __enter__(self):
        ops.set_mfma_precision(self.prec)
        ops.QUANT.reset()

    def __exit__(self, *exc):
        ops.set_mfma_precision("f32")
        ops.QUANT.reset()
        return False


class _Rig:
    """a prepared trainer, the state after prepare() and the ways back to it"""

    def __init__(self, tr, A):
        tr.prepare(*A)
        self.tr, self.sd, self.p0 = tr, tr.state_dict(), tr.flat_p.clone()
        pad = torch.ones(tr.n, dtype=torch.bool, device=DEV)
        for o, p in zip(tr.offs, tr.used):
            pad[o:o + p.numel()] = False
        self.pad = pad
        assert int(pad.sum()) > 0, "the flat layout of this model has no padding: the padding check is vacuous"

    def restore(self, sd=None):
        self.tr.flat_p.copy_(self.p0)               # the parameters are model.state_dict()'s business: first, then the trainer's state
        self.tr.load_state_dict(sd or self.sd)

    def poison_grads(self, acc=False):
        for g in self.tr.g_views:                   # every element of every slice; the padding between them stays as it is
            bits(g).fill_(poison_bits(F32))
        planted = int(pattern_mask(self.tr.flat_g, 0).sum())
        assert planted == self.tr.n - int(self.pad.sum()) and float(self.tr.flat_g[self.pad].abs().max()) == 0.0, "the poison did not reach the slices"
        if acc:
            bits(self.tr._accumulator()).fill_(poison_bits(F32))

    def read(self, loss):
        torch.cuda.synchronize()
        return {"loss": _u8(loss), "flat_g": _u8(self.tr.flat_g), "flat_p": _u8(self.tr.flat_p)}

    def step(self, batch, poison=False):
        if poison:
            self.poison_grads()
        return self.read(self.tr.step(*batch))

    def cycle(self, batches, poison=False):
        """one accumulation cycle: the micro-steps' losses, flat_g and flat_p after the optimiser step"""
        losses = []
        for i, b in enumerate(batches):
            if poison:
                self.poison_grads(acc=i == 0)
            losses.append(_u8(self.tr.step(*b)))
        out = self.read(losses[-1])
        out["loss"] = torch.cat(losses)
        return out

    def assert_clean(self, what):
        g = self.tr.flat_g
        assert not bool(pattern_mask(g, 0).any()), f"{what}: {int(pattern_mask(g, 0).sum())} elements of flat_g still hold the payload: no kernel wrote them"
        assert not bool(torch.isnan(g).any()), f"{what}: flat_g holds a NaN"
        assert float(g[self.pad].abs().max()) == 0.0, f"{what}: the alignment padding of flat_g is no longer zero (it is summed into the norm)"


def _same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs ({int((a[k] != b[k]).sum())} of {a[k].numel()} bytes)"


def _record(op, shape, detail, verdict="same bits"):
    print(f"[out-contract] {op:<22} {shape:<30} {detail}   {verdict}")


def _grad_slices(rig, what, mode, prec):
    A, B = _batches()
    rig.restore()
    want = rig.step(A)
    rig.restore()
    got = rig.step(A, poison=True)
    rig.assert_clean(f"{what}: a step on poisoned gradient slices")
    _same(want, got, f"{what}: a step on poisoned gradient slices against a step on clean ones")
    _record("flat_g", f"{mode}-{prec}", f"slices {len(rig.tr.g_views)} elements {rig.tr.n} padding {int(rig.pad.sum())}")
    # accum_steps = 2: the accumulator is never zeroed, so the first micro-step must overwrite it
    rig.restore()
    rig.tr.accum_steps = 2
    try:
        sd2 = rig.tr.state_dict()
        want = rig.cycle([A, B])
        rig.restore(sd2)
        got = rig.cycle([A, B], poison=True)
        rig.assert_clean(f"{what}: an accumulation cycle on poisoned slices and a poisoned accumulator")
        for lo, hi in rig.tr.buckets:   # (the padding between two buckets belongs to no pass: nothing reads it)
            assert not bool(pattern_mask(rig.tr._accumulator()[lo:hi], 0).any()), f"{what}: the accumulator still holds the payload in bucket {lo}:{hi}"
        _same(want, got, f"{what}: an accumulation cycle on poisoned buffers against a clean one")
        _record("flat_g accum_steps=2", f"{mode}-{prec}", f"slices {len(rig.tr.g_views)} elements {rig.tr.n} accumulator poisoned")
    finally:
        rig.tr.accum_steps = 1
        rig.restore()


def _replay_order(rig, what, mode, prec):
    A, B = _batches()
    runs = {}
    for name, before in (("first", None), ("after B", B), ("after A", A)):
        rig.restore()
        if before is not None:
            rig.step(before)
            rig.restore()
        runs[name] = rig.step(A)
    _same(runs["first"], runs["after B"], f"{what}: step(A) after step(B)")
    _same(runs["first"], runs["after A"], f"{what}: step(A) after step(A)")
    _record("replay order", f"{mode}-{prec}", "predecessors none / step(B) / step(A)")


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_eager_step_overwrites_the_gradient_slices(prec):
    with _Precision(prec):
        tr = _trainer(_model(), use_graph=False)
        try:
            rig = _Rig(tr, _batches()[0])
            _replay_order(rig, f"eager {prec}", "eager", prec)
            _grad_slices(rig, f"eager {prec}", "eager", prec)
        finally:
            tr.close()


@pytest.mark.parametrize("mode", ["graph", "graph-2stage"])
@pytest.mark.parametrize("prec", ["f32", "bf16", "fp8"])
def test_graph_replay_overwrites_and_forgets(prec, mode):
    """one capture per precision and mode serves both checks: the gradient slices (f32, bf16) and the order of the replays (all three)"""
    kw = dict(overlap=True, nstages=2) if mode == "graph-2stage" else {}
    with _Precision(prec):
        tr = _trainer(_model(), use_graph=True, **kw)
        try:
            rig = _Rig(tr, _batches()[0])
            assert tr.graph is not None and tr.staged == (mode == "graph-2stage")
            _replay_order(rig, f"{mode} {prec}", mode, prec)   # first: its run without predecessor follows the capture's own batch
            if prec != "fp8":
                _grad_slices(rig, f"{mode} {prec}", mode, prec)
        finally:
            tr.close()


# ================================================================================================ Validator and Forecaster after other batches
class _Drift(torch.nn.Module):
    """a stand-in forecast (tests/test_objects_gpu.py): the last input frame, moved and weakened with every lead"""
    T = 4

    def forward(self, x):
        last = x[:, -1, 0].float()
        return torch.stack([torch.roll(last, t + 1, dims=-1) * (1.0 - 0.15 * t) for t in range(self.T)], dim=1)


def _val_batches():
    out = []
    for name, gain in (("A", 1.0), ("B", 3.0), ("C", 0.5)):
        f = (recipe.radar_batch(2, 9, 32, name="outc.valid." + name) * gain * (255.0 / 70.0)).clamp(0, 1).to(DEV)
        out.append((f[:, :5].contiguous(), f[:, 5:].contiguous()))
    return out


def test_validator_does_not_depend_on_the_batches_before():
    from adnm_hip.validate import Validator
    from models.loss import RainfallLoss
    A, B, C = _val_batches()

    def make():
        return Validator(_Drift(), RainfallLoss(), 4, 90.0, THR, pools=((4, 2), (16, 8)), fss=(1, 5), persistence=True, advection=(8, 2), advection_flow=True,
                         spectrum=True, joint=True, objects=True)

    def read(val, out):
        torch.cuda.synchronize()
        return {"block": _u8(val._block), "out": _u8(out), "advected": _u8(val.advected(A[0])), "flow": _u8(val.flow(A[0])), "loss": _u8(val.last_loss),
                "done": repr(val.done(per_lead=True))}
    first = make()
    try:
        want = read(first, first.step(*A))
    finally:
        first.close()
    val = make()
    try:
        val.step(*B)
        val.step(*C)
        val.done(reset=True)
        got = read(val, val.step(*A))
        val.reset()
        again = read(val, val.step(*A))
    finally:
        val.close()
    for name, r in (("two other batches and a reset", got), ("itself and a reset", again)):
        assert r.pop("done") == want["done"], f"Validator.done() after {name} differs from a first batch's"
        _same({k: v for k, v in want.items() if k != "done"}, r, f"Validator after {name}")
    _record("Validator order", "2x4x32x32", f"block {want['block'].numel() // 8} doubles, predecessors none / B, C / A")


def test_forecaster_does_not_depend_on_the_batches_before():
    from adnm_hip.forecast import Forecaster, Palette
    import numpy as np
    A, B, C = _val_batches()
    rgba = (np.arange(4 * 5, dtype=np.int64).reshape(5, 4) * 37 % 256).astype(np.uint8)
    pal = Palette([0.0, 10.0, 20.0, 35.0, 50.0, 256.0], rgba)

    def read(res):
        torch.cuda.synchronize()
        return {"pred": _u8(res.pred), "fields": _u8(res.fields), "strip": _u8(res.strip)}
    first = Forecaster(_Drift(), pal, pixel_scale=255.0, frame_start=1, frame_step=2, gap=3)
    try:
        want = read(first(A[0]))
    finally:
        first.close()
    fc = Forecaster(_Drift(), pal, pixel_scale=255.0, frame_start=1, frame_step=2, gap=3)
    try:
        fc(B[0]), fc(C[0])
        got = read(fc(A[0]))
        again = read(fc(A[0]))
    finally:
        fc.close()
    _same(want, got, "Forecaster after two other batches")
    _same(want, again, "Forecaster after itself")
    _record("Forecaster order", "2x4x32x32", f"strip {tuple(first.render(A[1]).strip.shape)}, predecessors none / B, C / A")


# ================================================================================================ the allow-list is alive
def test_every_allow_list_entry_was_hit():
    """a stale entry fails: every (site, role) on the list must have been reached by one of the cases above (checked when they all ran)"""
    every = {(c.op, tuple(c.shape)) for c in CASES + EXTRA} | {("ADNMUNet-64", (2, 25, 64, 64, prec)) for prec in ("f32", "bf16", "fp8")}
    if not every <= _RAN:
        return   # a selection of the file ran: nothing to say about the list
    stale = sorted(set(ALLOW) - _HIT)
    assert not stale, f"allow-list entries that no case hit: {stale}"
    assert all(isinstance(r, str) and r for r in ALLOW.values()), "every allow-list entry carries its reason"
