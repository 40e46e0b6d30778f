"""The five skip-gate kernels (csrc/skipgate.hip) inside a launch group (ops.GROUP): several problems in one bracket give, bit for bit, what
the same calls give outside a bracket, in one launch per kernel and direction (two when there are more problems than a launch holds), and
ops.e2d_group runs the skip step of its chains that way."""
import ctypes

import pytest
import torch

from adnm_hip import lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_SCOPES = ("skip_pool_fwd", "skip_branch_fwd")
BWD_SCOPES = ("skip_branch_bwd", "skip_conv_bwd", "skip_pool_bwd")
GRAD_NAMES = ["w13", "b13", "w31", "b31", "w33", "b33", "ffd13.w", "ffd13.b", "ffd33.w", "ffd33.b", "enh13", "thr13", "enh33", "thr33",
              "alpha1", "alpha2", "alpha3", "gamma"]

# (B, H, W, C): a wide map; a channel count that is no multiple of 16 conv groups on an odd map; waves that straddle pixel slices
THREE = [(2, 4, 4, 256), (3, 5, 5, 36), (2, 9, 7, 64)]
# more than one pixel slice in the weight-gradient pass (partial rows + skip_wgrad_fold) beside a problem that writes the gradient directly
WGRAD_SLICES = [(1, 40, 40, 256), (2, 4, 4, 256)]
NINE = [(1, 4, 4, 64)] * 9   # more than a launch holds (8): two launches per position


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


def _problem(i, B, H, W, C):
    """-> (x, cotangent, the 18 parameters in adnm_skipgate_fwd's order), every problem with values of its own"""
    s = 1000 * (i + 1)
    shapes = [(C, 4, 1, 3), (C,), (C, 4, 3, 1), (C,), (C, 4, 3, 3), (C,), (C,), (C,), (C,), (C,)]
    params = [_rand(sh, s + 10 + k, 0.5 if len(sh) > 1 else 0.3) for k, sh in enumerate(shapes)]
    params[6], params[8] = 1 + params[6], 1 + params[8]
    params += [torch.tensor(v + 0.01 * i, device=DEV) for v in (1.3, 0.1, 0.8, -0.05, 0.33, 0.4, 0.27)] + [1 + 0.2 * _rand((C,), s + 40)]
    return _rand((B, H * W, C), s + 1, 1.5), _rand((B, H * W, C), s + 2), params


def _run(shapes, probs, grouped, queues, events=None):
    """forward and backward of every problem through SkipGateFn's own code -> (outs, [(dx, 18 parameter gradients)])"""
    n = len(shapes)
    ctx = [ops._SubCtx(21) for _ in range(n)]
    fwd = lambda i: ops.SkipGateFn.forward(ctx[i], probs[i][0], shapes[i][1], shapes[i][2], *probs[i][2])
    bwd = lambda i: ops.SkipGateFn.backward(ctx[i], probs[i][1])
    dev = torch.device(DEV, torch.cuda.current_device())
    with torch.no_grad(), ops.FOLDS.active(dev, on=queues):
        if grouped:
            with _Events() as ev_f:
                with ops.GROUP:
                    outs = [fwd(i) for i in range(n)]
                    assert lib.query("adnm_group_pending") == 2 * n   # pools and branches of every problem, nothing launched yet
            with _Events() as ev_b:
                with ops.GROUP:
                    gs = [bwd(i) for i in range(n)]
                    assert lib.query("adnm_group_pending") >= 3 * n
            assert lib.query("adnm_group_pending") == 0
            if events is not None:
                events.append((ev_f.count, ev_b.count))
        else:
            outs = [fwd(i) for i in range(n)]
            gs = [bwd(i) for i in range(n)]
    torch.cuda.synchronize()
    return outs, [(g[0], list(g[3:21])) for g in gs]


def _compare(shapes, got, want, what):
    for i, shape in enumerate(shapes):
        assert torch.equal(got[0][i], want[0][i]), f"{what}: out of problem {i} {shape}"
        assert torch.equal(got[1][i][0], want[1][i][0]), f"{what}: dx of problem {i} {shape}"
        assert len(got[1][i][1]) == 18
        for name, g, r in zip(GRAD_NAMES, got[1][i][1], want[1][i][1]):
            assert g.shape == r.shape and torch.equal(g, r), f"{what}: d{name} of problem {i} {shape}: max |diff| {float((g - r).abs().max())}"


@pytest.fixture(scope="module")
def separate():
    """the reference of every set of problems, computed once: the same calls outside a bracket (folds immediate)"""
    memo = {}

    def get(shapes):
        key = tuple(shapes)
        if key not in memo:
            probs = [_problem(i, *s) for i, s in enumerate(shapes)]
            memo[key] = (probs, _run(shapes, probs, False, False))
        return memo[key]
    return get


@pytest.mark.parametrize("queues", [False, True], ids=["immediate", "queued"])
def test_three_problems_in_one_bracket(separate, queues):
    """forward and backward, with the fold and leaf queues bound (the folds wait there) and without (recorded behind the producers)"""
    probs, want = separate(THREE)
    for again in range(2):   # back to back: a temporary shared between two problems of a launch would show in the second round
        events = []
        got = _run(THREE, probs, True, queues, events)
        _compare(THREE, got, want, f"round {again}")
        ev_f, ev_b = events[0]
        for scope in FWD_SCOPES:
            assert ev_f.get(scope) == 1, ev_f   # three problems, one launch
        for scope in BWD_SCOPES:
            assert ev_b.get(scope) == 1, ev_b


def test_partial_rows_beside_a_direct_weight_gradient(separate):
    probs, want = separate(WGRAD_SLICES)
    with _Events() as ev:   # launched alone, exactly one of the two problems folds partial weight rows
        _compare(WGRAD_SLICES, _run(WGRAD_SLICES, probs, False, False), want, "separate again")
    assert ev.count.get("skip_wgrad_fold") == 1, ev.count
    events = []
    got = _run(WGRAD_SLICES, probs, True, False, events)
    _compare(WGRAD_SLICES, got, want, "wgrad slices")
    assert all(events[0][1].get(scope) == 1 for scope in BWD_SCOPES), events[0][1]


def test_nine_problems_take_two_launches(separate):
    probs, want = separate(NINE)
    events = []
    got = _run(NINE, probs, True, False, events)
    _compare(NINE, got, want, "nine problems")
    ev_f, ev_b = events[0]
    for scope in FWD_SCOPES:
        assert ev_f.get(scope) == 2, ev_f   # eight problems, then the ninth
    for scope in BWD_SCOPES:
        assert ev_b.get(scope) == 2, ev_b


def test_a_bracket_that_raises_launches_nothing(separate):
    probs, want = separate(THREE)
    ctx = [ops._SubCtx(21) for _ in THREE]
    with _Events() as ev:
        with pytest.raises(KeyError):
            with torch.no_grad(), ops.GROUP:
                for i, (B, H, W, C) in enumerate(THREE):
                    ops.SkipGateFn.forward(ctx[i], probs[i][0], H, W, *probs[i][2])
                assert lib.query("adnm_group_pending") == 6
                raise KeyError("inside the bracket")
        assert lib.query("adnm_group_pending") == 0 and not ops.GROUP.open
    assert not any(k.startswith("skip_") for k in ev.count), ev.count
    _compare(THREE, _run(THREE, probs, True, False), want, "behind the cleared bracket")


# ---- the node: three small InstanceNorm chains, the skip step of all three in one bracket
@pytest.fixture(params=["f32", "bf16"])
def prec(request):
    ops.set_mfma_precision(request.param)
    yield request.param
    ops.set_mfma_precision("f32")


def _node_run(mods, xs, gates, cots, grouped):
    for m in mods:
        m.zero_grad(set_to_none=True)
    xs = [x.clone().requires_grad_(True) for x in xs]
    gates = [g.clone().requires_grad_(True) for g in gates]
    with _Events() as ev:
        outs = ops.e2d_group(xs, gates, mods) if grouped else [m(x=x, res=g) for m, x, g in zip(mods, xs, gates)]
        torch.autograd.backward(outs, cots)
    grads = {f"{i}.{k}": p.grad for i, m in enumerate(mods) for k, p in m.named_parameters()}
    return outs, [x.grad for x in xs], [g.grad for g in gates], grads, ev.count


def test_node_runs_the_skip_kernels_once_per_direction(prec):
    from models.model_untils import EncoderToDecoder
    dims, maps, B = [256, 256, 512], [2, 4, 3], 2
    torch.manual_seed(1234)
    mods = [EncoderToDecoder(embed_dim=c, InstanceNorm=True).to(DEV) for c in dims]
    for m in mods:   # away from the initial values: every parameter gradient is a real number
        for p in m.parameters():
            p.data.add_(0.05 * torch.randn_like(p))
    xs = [_rand((B, h * h, c), 100 + i) for i, (c, h) in enumerate(zip(dims, maps))]
    gates = [_rand((B, 1, c), 200 + i) for i, c in enumerate(dims)]
    cots = [_rand((B, h * h, c), 300 + i) for i, (c, h) in enumerate(zip(dims, maps))]
    ro, rdx, rdg, rg, rcount = _node_run(mods, xs, gates, cots, False)
    go, gdx, gdg, gg, gcount = _node_run(mods, xs, gates, cots, True)
    for scope in FWD_SCOPES + BWD_SCOPES:
        assert rcount.get(scope) == 3 and gcount.get(scope) == 1, (scope, rcount.get(scope), gcount.get(scope))
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
    assert used >= 3 * 35, used
