"""The launch group (include/adnm_hip.h: adnm_group_*; ops.GROUP) and the grouped EncoderToDecoder node (ops.e2d_group): a bracket gives
bit for bit what the same calls give as separate launches, and the node what separate EncoderToDecoder.forward calls give."""
import ctypes

import pytest
import torch

from adnm_hip import lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (M, N, K) of Y[M,N] = X[M,K] W[N,K]^T.  Two LDS-tiled problems whose plans split the reduction (distinct counters and slabs inside one
# merged launch), an unsplit ragged one on the same kernel, and a split one on the register-streaming kernel (a launch of its own)
NT_SHAPES = [(16, 512, 2048), (64, 4096, 1024), (100, 72, 36), (64, 512, 2048)]
# (M, N, K) of dX[M,K] = dY[M,N] W[N,K].  Two split problems of one register-streaming instantiation, a split LDS-tiled one (the other kernel)
# and an unsplit ragged one
NN_SHAPES = [(64, 2048, 512), (64, 2048, 1024), (256, 1024, 2048), (100, 72, 36)]


@pytest.fixture(params=["f32", "bf16"])
def prec(request):
    ops.set_mfma_precision(request.param)
    yield request.param
    ops.set_mfma_precision("f32")


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


def _counters_idle():
    torch.cuda.synchronize()
    for regs in ops.SPLITWS._streams.values():
        for reg in regs:
            assert int(reg.counters.abs().max()) == 0, "a split launch left an arrival counter behind"


@pytest.mark.parametrize("op", ["nt", "nn"])
def test_bracket_equals_separate_gemm_launches(op, prec):
    shapes = NT_SHAPES if op == "nt" else NN_SHAPES
    code = ops.SK_NT if op == "nt" else ops.SK_NN
    split = [lib.query("adnm_skgemm_ws_bytes", code, M, N, K) > 16 for M, N, K in shapes]
    assert sum(split) >= 2 and not all(split), split
    a = [_rand((M, K if op == "nt" else N), 10 + i) for i, (M, N, K) in enumerate(shapes)]
    w = [_rand((N, K), 20 + i, 0.05) for i, (M, N, K) in enumerate(shapes)]
    bias = [_rand((N,), 30 + i) if op == "nt" and i % 2 == 0 else None for i, (M, N, K) in enumerate(shapes)]
    run = (lambda i: ops.k_linear(a[i], w[i], bias[i])) if op == "nt" else (lambda i: ops.k_linear_dx(a[i], w[i]))
    want = [run(i) for i in range(len(shapes))]
    scope = "skgemm_nt" if op == "nt" else "skgemm_nn"
    for again in range(2):   # back to back: a stale counter or a shared workspace would show in the second round
        with _Events() as ev:
            with ops.GROUP:
                got = [run(i) for i in range(len(shapes))]
                assert lib.query("adnm_group_pending") == len(shapes)
        assert lib.query("adnm_group_pending") == 0
        # one event per launch: fewer launches than problems = a merge took place; more than one = a problem whose plan selects the other
        # kernel went out in a launch of its own
        print(f"{op} {prec}: {ev.count.get(scope)} launches for {len(shapes)} problems")
        assert 2 <= ev.count.get(scope, 0) < len(shapes), ev.count
        for i, (g, r) in enumerate(zip(got, want)):
            assert torch.equal(g, r), f"{op} problem {i} {shapes[i]} (round {again}): max |diff| {float((g - r).abs().max())}"
    _counters_idle()
    again = [run(i) for i in range(len(shapes))]   # plain launches behind a bracket: the region is as they expect it
    assert all(torch.equal(g, r) for g, r in zip(again, want))


def test_more_problems_than_one_launch_holds(prec):
    """ten problems of one instantiation: a launch holds eight, the rest follow in a second one"""
    M, N, K = 100, 72, 36
    a = [_rand((M, K), 50 + i) for i in range(10)]
    w = [_rand((N, K), 70 + i, 0.05) for i in range(10)]
    want = [ops.k_linear(a[i], w[i], None) for i in range(10)]
    with _Events() as ev:
        with ops.GROUP:
            got = [ops.k_linear(a[i], w[i], None) for i in range(10)]
    assert ev.count.get("skgemm_nt") == 2, ev.count
    assert all(torch.equal(g, r) for g, r in zip(got, want))


def test_exception_inside_a_bracket_leaves_nothing_recorded():
    M, N, K = 64, 512, 2048
    a, w = _rand((M, K), 1), _rand((N, K), 2, 0.05)
    want = ops.k_linear(a, w, None)
    with pytest.raises(KeyError):
        with ops.GROUP:
            ops.k_linear(a, w, None)
            assert lib.query("adnm_group_pending") == 1
            raise KeyError("inside the bracket")
    assert lib.query("adnm_group_pending") == 0 and not ops.GROUP.open
    assert torch.equal(ops.k_linear(a, w, None), want)
    with ops.GROUP:
        got = ops.k_linear(a, w, None)
    assert torch.equal(got, want)
    _counters_idle()


def test_trailing_copy_is_refused_inside_a_bracket():
    a, w = _rand((64, 256), 3), _rand((128, 256), 4, 0.05)
    out = torch.empty((64, 130), device=DEV)[:, 1:129]   # a view the kernel cannot write (misaligned): k_linear would copy into it
    with pytest.raises(AssertionError, match="trailing copy"):
        with ops.GROUP:
            ops.k_linear(a, w, None, out=out)
    assert not ops.GROUP.open


# ---- stencil and gate kinds: B = 2; maps 2x2, 4x4 and 3x3 (a window cut by the border); channels 256, 256, 512
KIND_SHAPES = [(2, 2, 256), (2, 4, 256), (2, 3, 512)]   # (B, H = W, C)


STORAGE = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])   # token storage: both forms of every kernel


@STORAGE
@pytest.mark.parametrize("act", [lib.ACT_NONE, lib.ACT_GELU], ids=["none", "gelu"])
def test_bracket_equals_separate_stencil_launches(act, dtype):
    x = [_rand((B * h * h, C), 400 + i).to(dtype) for i, (B, h, C) in enumerate(KIND_SHAPES)]
    dy = [_rand((B * h * h, C), 410 + i).to(dtype) for i, (B, h, C) in enumerate(KIND_SHAPES)]
    wt = [_rand((C, 9), 420 + i, 0.3) for i, (B, h, C) in enumerate(KIND_SHAPES)]
    bias = [_rand((C,), 430 + i) for i, (B, h, C) in enumerate(KIND_SHAPES)]
    fwd = lambda i: ops.k_dwconv_fwd(x[i], wt[i], bias[i], KIND_SHAPES[i][0], KIND_SHAPES[i][1], KIND_SHAPES[i][1], KIND_SHAPES[i][2], 3, act, chan_major=True)
    args = lambda i: (dy[i], x[i], wt[i], bias[i], KIND_SHAPES[i][0], KIND_SHAPES[i][1], KIND_SHAPES[i][1], KIND_SHAPES[i][2], 3, act)
    want_y = [fwd(i) for i in range(3)]
    want_g = [ops.k_dwconv_bwd(*args(i), want_bias=True, chan_major=True) for i in range(3)]
    for again in range(2):
        with _Events() as ev:
            with ops.GROUP:
                got_y = [fwd(i) for i in range(3)]
                assert lib.query("adnm_group_pending") == 3
            with ops.GROUP:
                states = [ops.k_dwconv_bwd_dx(*args(i), want_bias=True, chan_major=True) for i in range(3)]
                assert lib.query("adnm_group_pending") == (6 if act != lib.ACT_NONE else 3)   # dpre, then the input gradient that reads it
        # three problems of one instantiation per step = one launch: the forward, (dpre,) the input gradient
        assert ev.count.get("dwconv_k3") == (3 if act != lib.ACT_NONE else 2), ev.count
        assert got_y[0].dtype == dtype and states[0]["dx"].dtype == dtype
        got_g = [ops.k_dwconv_bwd_w(s) for s in states]
        for i in range(3):
            assert torch.equal(got_y[i], want_y[i]), f"forward {KIND_SHAPES[i]} (round {again})"
            for name, g, r in zip(("dx", "dw", "db"), got_g[i], want_g[i]):
                assert torch.equal(g, r), f"{name} {KIND_SHAPES[i]} (round {again})"


def test_weight_gradient_is_refused_inside_a_bracket():
    """adnm_dwconv_bwd with a weight-gradient destination would read a dpre that is only recorded: a host refusal, before any launch"""
    B, h, C = KIND_SHAPES[0]
    x, dy, wt = _rand((B * h * h, C), 1), _rand((B * h * h, C), 2), _rand((C, 9), 3)
    dx, dwt, ws = torch.empty_like(x), torch.empty_like(wt), torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="inside a launch group"):
        with ops.GROUP:
            lib.call("adnm_dwconv_bwd", dy.data_ptr(), C, x.data_ptr(), C, wt.data_ptr(), None, None, dx.data_ptr(), C, dwt.data_ptr(), None,
                     ws.data_ptr(), ws.numel(), B, h, h, C, 3, 3, lib.ACT_NONE, 1, lib.F32, None)
    assert lib.query("adnm_group_pending") == 0 and not ops.GROUP.open


@STORAGE
def test_bracket_equals_separate_gate_launches(dtype):
    h = [_rand((B * s * s, 2 * C), 500 + i).to(dtype) for i, (B, s, C) in enumerate(KIND_SHAPES)]
    dy = [_rand((B * s * s, C), 510 + i).to(dtype) for i, (B, s, C) in enumerate(KIND_SHAPES)]
    want_y = [ops.k_gate_fwd(h[i], KIND_SHAPES[i][2]) for i in range(3)]
    want_d = [ops.k_gate_bwd(dy[i], h[i], KIND_SHAPES[i][2]) for i in range(3)]
    for again in range(2):
        with _Events() as ev:
            with ops.GROUP:
                got_y = [ops.k_gate_fwd(h[i], KIND_SHAPES[i][2]) for i in range(3)]
                got_d = [ops.k_gate_bwd(dy[i], h[i], KIND_SHAPES[i][2]) for i in range(3)]
                assert lib.query("adnm_group_pending") == 6
        assert ev.count.get("gate_fwd") == 1 and ev.count.get("gate_bwd") == 1, ev.count   # three problems each, one launch each
        assert got_y[0].dtype == dtype and got_d[0].dtype == dtype
        for i in range(3):
            assert torch.equal(got_y[i], want_y[i]) and torch.equal(got_d[i], want_d[i]), f"gate {KIND_SHAPES[i]} (round {again})"


@STORAGE
@pytest.mark.parametrize("act", [lib.ACT_NONE, lib.ACT_GELU], ids=["none", "gelu"])
def test_bracket_equals_separate_instnorm_launches(act, dtype):
    """stats then apply are two dependent launches of one call: position 0 of every problem goes before position 1 of any; without a bound
    fold queue the scalar gradients' folds are recorded behind both"""
    x = [_rand((B, s * s, C), 600 + i).to(dtype) for i, (B, s, C) in enumerate(KIND_SHAPES)]
    dy = [_rand((B, s * s, C), 610 + i).to(dtype) for i, (B, s, C) in enumerate(KIND_SHAPES)]
    scale, shift = _rand((), 620) + 1.5, _rand((), 621)
    fwd = lambda i: ops.k_instnorm_fwd(x[i], scale, shift, KIND_SHAPES[i][0], KIND_SHAPES[i][1] ** 2, KIND_SHAPES[i][2], 1e-5, act)
    want = [fwd(i) for i in range(3)]
    bwd = lambda i: ops.k_instnorm_bwd(dy[i], x[i], scale, shift, want[i][1], want[i][2], KIND_SHAPES[i][0], KIND_SHAPES[i][1] ** 2, KIND_SHAPES[i][2], act)
    want_g = [bwd(i) for i in range(3)]
    for again in range(2):
        with _Events() as ev:
            with ops.GROUP:
                got = [fwd(i) for i in range(3)]
                assert lib.query("adnm_group_pending") == 6
            with ops.GROUP:
                got_g = [bwd(i) for i in range(3)]
                assert lib.query("adnm_group_pending") == 9   # stats, apply and the recorded fold of each problem
        for scope in ("instnorm_stats", "instnorm_apply", "instnorm_bwd_stats", "instnorm_bwd_apply"):
            assert ev.count.get(scope) == 1, ev.count   # three problems, one launch
        assert got[0][0].dtype == dtype and got_g[0][0].dtype == dtype
        for i in range(3):
            for name, g, r in zip(("y", "mu", "rstd"), got[i], want[i]):
                assert torch.equal(g, r), f"{name} {KIND_SHAPES[i]} (round {again})"
            for name, g, r in zip(("dx", "dscale", "dshift"), got_g[i], want_g[i]):
                assert torch.equal(g, r), f"{name} {KIND_SHAPES[i]} (round {again})"


@pytest.mark.parametrize("per_token", [False, True], ids=["gate_b1c", "gate_blc"])
def test_bracket_equals_separate_igate_res_launches(per_token):
    def run(grouped):
        xs = [_rand((B, s * s, C), 700 + i).requires_grad_(True) for i, (B, s, C) in enumerate(KIND_SHAPES)]
        rs = [_rand((B, s * s if per_token else 1, C), 710 + i).requires_grad_(True) for i, (B, s, C) in enumerate(KIND_SHAPES)]
        ps = [[(_rand((), 720 + 3 * i + k) + 1.0).requires_grad_(True) for k in range(3)] for i in range(3)]
        ctx = [ops._SubCtx(5) for _ in range(3)]
        cots = [_rand(tuple(x.shape), 730 + i) for i, x in enumerate(xs)]
        with torch.no_grad():
            if grouped:
                with ops.GROUP:
                    ys = [ops.IGateResFn.forward(ctx[i], xs[i], rs[i], *ps[i]) for i in range(3)]
                with ops.GROUP:
                    gs = [ops.IGateResFn.backward(ctx[i], cots[i]) for i in range(3)]
            else:
                ys = [ops.IGateResFn.forward(ctx[i], xs[i], rs[i], *ps[i]) for i in range(3)]
                gs = [ops.IGateResFn.backward(ctx[i], cots[i]) for i in range(3)]
        torch.cuda.synchronize()
        return ys, gs
    want_y, want_g = run(False)
    for again in range(2):
        got_y, got_g = run(True)
        for i in range(3):
            assert torch.equal(got_y[i], want_y[i]), f"y {KIND_SHAPES[i]} (round {again})"
            for name, g, r in zip(("dx", "dres", "dgama", "denhance", "dthreshold"), got_g[i], want_g[i]):
                assert torch.equal(g, r), f"{name} {KIND_SHAPES[i]} (round {again})"


# ---- the node against separate EncoderToDecoder.forward calls
def _chains(dims, maps, instance_norm, B=2):
    from models.model_untils import EncoderToDecoder
    torch.manual_seed(1234)
    mods = [EncoderToDecoder(embed_dim=c, InstanceNorm=instance_norm).to(DEV) for c in dims]
    for m in mods:   # away from the initial values (gamma = 1, scale = 1, shift = 0 ...): every parameter gradient is a real number
        for p in m.parameters():
            p.data.add_(0.05 * torch.randn_like(p))
    xs = [_rand((B, h * h, c), 100 + i) for i, (c, h) in enumerate(zip(dims, maps))]
    gates = [_rand((B, 1, c), 200 + i) for i, c in enumerate(dims)]
    cots = [_rand((B, h * h, c), 300 + i) for i, (c, h) in enumerate(zip(dims, maps))]
    return mods, xs, gates, cots


def _run(mods, xs, gates, cots, grouped, queues):
    for m in mods:
        m.zero_grad(set_to_none=True)
    xs = [x.clone().requires_grad_(True) for x in xs]
    gates = [g.clone().requires_grad_(True) for g in gates]
    dev = torch.device(DEV, torch.cuda.current_device())
    with ops.FOLDS.active(dev, on=queues):
        outs = ops.e2d_group(xs, gates, mods) if grouped else [m(x=x, res=g) for m, x, g in zip(mods, xs, gates)]
        torch.autograd.backward(outs, cots)
    torch.cuda.synchronize()
    grads = {f"{i}.{k}": p.grad for i, m in enumerate(mods) for k, p in m.named_parameters()}
    return outs, [x.grad for x in xs], [g.grad for g in gates], grads


@pytest.mark.parametrize("queues", [False, True], ids=["immediate", "queued"])
@pytest.mark.parametrize("instance_norm", [True, False], ids=["instnorm", "groupnorm4"])
def test_node_equals_three_module_calls(instance_norm, queues, prec):
    # B = 2; maps 2x2, 4x4 and 3x3 (a window cut by the border); C / 4 divisible by 64 (the skip backward)
    mods, xs, gates, cots = _chains([256, 256, 512], [2, 4, 3], instance_norm)
    ro, rdx, rdg, rg = _run(mods, xs, gates, cots, False, queues)
    go, gdx, gdg, gg = _run(mods, xs, gates, cots, True, queues)
    for i in range(3):
        assert torch.equal(go[i], ro[i]), f"output {i}"
        assert torch.equal(gdx[i], rdx[i]), f"d x {i}"
        assert torch.equal(gdg[i], rdg[i]), f"d res {i}"
    assert set(gg) == set(rg)
    used = 0
    for k in rg:
        assert (gg[k] is None) == (rg[k] is None), k
        if rg[k] is not None:
            used += 1
            assert torch.equal(gg[k], rg[k]), f"d {k}: max |diff| {float((gg[k] - rg[k]).abs().max())}"
    assert used >= 3 * 35, used   # the 37 tensors of group_args() less the affine pair an InstanceNorm does not have
    _counters_idle()


def test_node_equals_seven_forward_only_chains(prec):
    """compute_dead_branches=True: seven chains, forward only (the dead ones never get a gradient)"""
    mods, xs, gates, _ = _chains([256, 256, 512, 128, 64, 32, 16], [2, 4, 3, 2, 4, 3, 2], True)
    with torch.no_grad():
        want = [m(x=x, res=g) for m, x, g in zip(mods, xs, gates)]
        got = ops.e2d_group(xs, gates, mods)
    assert len(got) == 7 and all(torch.equal(g, r) for g, r in zip(got, want))
