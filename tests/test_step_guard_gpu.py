"""The monitored training step on the GPU (FlatTrainer(monitor=True); adnm_step_guard, adnm_adamw_step_guarded,
adnm_quant_update_guarded, adnm_loss_stat): train.py:136-153 with the per-step .item() reads replaced by device-resident statistics,
and the step a mixed-precision trainer skips — one whose gradient is not finite.  The guarded sequence against adnm_adamw_step bit for
bit when the gradient is finite; nothing but the counters moves when it is not; the trainer against a twin without the monitor."""
import numpy as np
import pytest
import torch

from adnm_hip import lib, ops, recipe
from adnm_hip.trainer import FlatTrainer

pytestmark = pytest.mark.gpu
DEV = "cuda"

NEW_ENTRY_POINTS = ("adnm_step_guard", "adnm_adamw_step_guarded", "adnm_quant_update_guarded", "adnm_loss_stat")
# one partial float4 trip; a few workgroups (257 quads: the second segment starts inside a wave); 262 145 quads = 1025 workgroups of the
# AdamW launch and 129 contiguous ranges of the segmented one.  BIG: one quad more than a full pass of the AdamW grid (4096 x 256 lanes),
# so that lane 0 alone makes a second grid-stride trip
SIZES = [4, 1028, 1048580]
BIG = 4 * 4096 * 256 + 4
KINDS = ["none", "bf16", "bf16_seg", "fp8"]
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-9, wd=1e-2, max_norm=0.5)
HEADROOM = 2.0
# what the GEMMs of a recording step would have left in the call-site record (row 2) and the optimiser pass before it in the weight
# records (rows 0, 1): [scale_a, scale_b, amax_a, amax_b, fmax_a, fmax_b, record, -]
TABLE = [[1.0, 0.5, 0.0, 2.0, 0.0, 448.0, 1.0, 0.0], [1.0, 2.0, 0.0, 0.75, 0.0, 448.0, 1.0, 0.0], [1.0, 1.0, 3.0, 2.0, 448.0, 448.0, 1.0, 0.0]]

_base = {}


def _vals(name, n, **kw):
    """the first n of one recipe stream per name, made once at the largest size"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _base:
        _base[key] = recipe.tensor("guard." + name, (BIG,), **kw).to(DEV)
    return _base[key][:n].clone()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Bufs:
    """flat p / m / v / state (+ shadow, segment tables, quantisation table) of one optimiser, and both ways to step it"""

    def __init__(self, n, kind):
        self.n, self.kind = n, kind
        self.p, self.m, self.v = _vals("p", n), _vals("m", n, scale=0.1), _vals("v", n, scale=0.01, positive=True)
        self.state = torch.zeros(4, device=DEV)
        self.ws = torch.empty(int(lib.query("adnm_adamw_ws_bytes")), dtype=torch.uint8, device=DEV)
        self.stats = torch.zeros(9, dtype=torch.float64, device=DEV)
        self.shadow = self.seg_end = self.seg_rec = self.tab = self.qstate = None
        n4 = n // 4
        if kind != "none":
            self.shadow = torch.zeros(n, dtype=torch.uint8 if kind == "fp8" else torch.bfloat16, device=DEV)
        if kind in ("bf16_seg", "fp8"):
            cut = 1 if n4 == 1 else (100 if n4 < 1000 else 100001)   # two segments; the cut is no multiple of the wave
            self.seg_end = torch.tensor([cut, n4], dtype=torch.int32, device=DEV)
            self.seg_rec = torch.tensor([0, 1] if kind == "fp8" else [-1, -1], dtype=torch.int32, device=DEV)
        if kind == "fp8":
            self.tab = torch.tensor(TABLE, dtype=torch.float32, device=DEV)
            self.qstate = torch.tensor([0.0, 2.0], device=DEV)   # period 2: steps 1 and 3 of a run end a recording step

    def clone(self):
        c = Bufs.__new__(Bufs)
        c.__dict__ = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in self.__dict__.items()}
        return c

    def _shadow_args(self):
        if self.kind == "none":
            return (None, 0, None, None, 0, None)
        seg = (self.seg_end.data_ptr(), self.seg_rec.data_ptr(), 2) if self.seg_end is not None else (None, None, 0)
        return (self.shadow.data_ptr(), 2 if self.kind == "fp8" else 1) + seg + (self.tab.data_ptr() if self.tab is not None else None,)

    def _hyper_args(self):
        h = HYPER
        return (h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["max_norm"])

    def plain_step(self, g):
        """what FlatTrainer(monitor=False) launches: (fp8: table update,) adnm_adamw_step"""
        if self.tab is not None:
            lib.call("adnm_quant_update", self.tab.data_ptr(), self.tab.shape[0], self.qstate.data_ptr(), HEADROOM, _stream())
        lib.call("adnm_adamw_step", self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n, self.state.data_ptr(),
                 *self._hyper_args(), self.ws.data_ptr(), self.ws.numel(), *self._shadow_args(), None, _stream())

    def guarded_step(self, g):
        """the guarded sequence: guard + statistics -> (fp8: guarded table update) -> guarded optimiser"""
        lib.call("adnm_step_guard", g.data_ptr(), self.n, self.state.data_ptr(), HYPER["max_norm"], None, self.ws.data_ptr(), self.ws.numel(),
                 self.stats.data_ptr(), _stream())
        if self.tab is not None:
            lib.call("adnm_quant_update_guarded", self.tab.data_ptr(), self.tab.shape[0], self.qstate.data_ptr(), HEADROOM, self.stats.data_ptr(),
                     _stream())
        lib.call("adnm_adamw_step_guarded", self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.n, self.state.data_ptr(),
                 *self._hyper_args(), *self._shadow_args(), None, self.stats.data_ptr(), _stream())

    def named(self):
        return [(k, getattr(self, k)) for k in ("p", "m", "v", "state", "shadow", "tab", "qstate") if getattr(self, k) is not None]

    def skip_flag(self):
        return int(self.stats.view(torch.int32)[16])


def _same_bits(a, b):
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))   # (NaN-safe, and +0 / -0 differ)


def _assert_same(x, y, what):
    for (name, a), (_, b) in zip(x.named(), y.named()):
        assert _same_bits(a, b), f"{what}: {name} differs"


def _ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


# (the second grid pass exists only in the interleaved AdamW kernel; the segmented one splits the buffer into contiguous ranges)
@pytest.mark.parametrize("n,kind", [(n, k) for n in SIZES for k in KINDS] + [(BIG, "none"), (BIG, "bf16")])
def test_guarded_sequence_is_bitwise_adamw_step_on_finite_gradients(n, kind):
    ref = Bufs(n, kind)
    mine = ref.clone()
    norms = []
    for i in range(3):
        g = _vals(f"g{i}", n, scale=0.5 ** i)
        ref.plain_step(g)
        mine.guarded_step(g.clone())
        _assert_same(ref, mine, f"step {i + 1}")
        assert mine.skip_flag() == 0
        norms.append(float(ref.state[1].sqrt()))
    if kind == "fp8":
        assert not torch.equal(ref.tab[:, 1], torch.tensor(TABLE, device=DEV)[:, 1]), "the table never made a new scale: the fp8 case checks nothing"
    if kind == "bf16":
        assert torch.equal(mine.shadow, mine.p.to(torch.bfloat16))
    st = mine.stats.tolist()
    assert st[0] == 3 and st[1] == 0 and st[6] == 0 and st[7] == 0
    # the norms are fp32 values (torch's sqrt and the kernel's may differ in the last place), summed in fp64
    assert abs(st[2] - sum(norms)) <= sum(_ulp32(x) for x in norms) and abs(st[3] - max(norms)) <= _ulp32(max(norms))
    assert abs(st[4] - norms[-1]) <= _ulp32(norms[-1])
    assert st[5] == sum(x > np.float32(HYPER["max_norm"]) for x in norms)


def test_second_grid_pass_is_not_skipped_by_mistake():
    """BIG has exactly one quad beyond the grid's first pass: it must have been updated (the case above would pass if BOTH sides forgot it)"""
    b = Bufs(BIG, "none")
    p0 = b.p.clone()
    b.guarded_step(_vals("g0", BIG))
    assert not torch.equal(b.p[-4:], p0[-4:]) and not torch.equal(b.p[:4], p0[:4])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_poisoned_gradient_changes_nothing_but_the_counters(n, kind):
    start = Bufs(n, kind)
    start.plain_step(_vals("g0", n))   # one ordinary step first: non-trivial state floats, a written shadow
    if kind == "fp8":   # ... and the table as a RECORDING step leaves it: maxima collected, flags set, the counter on a multiple of the period
        start.tab.copy_(torch.tensor(TABLE, device=DEV))
        start.tab[:, 0:2] = torch.tensor([[1.0, 4.0], [1.0, 8.0], [2.0, 3.0]], device=DEV)
        start.qstate[0] = 2.0
    g1 = _vals("g1", n)
    want = start.clone()
    want.plain_step(g1)                # the first clean step of an untouched copy
    places = [0, n - 1] + ([n // 2] if n == SIZES[-1] else [])
    for bad in (float("inf"), float("-inf"), float("nan")):
        for at in places:
            b = start.clone()
            g = g1.clone()
            g[at] = bad
            b.guarded_step(g)
            what = f"{bad} at {at}"
            for (name, a), (_, a0) in zip(b.named(), start.named()):
                if name == "tab":   # only the call-site record's maxima are gone
                    exp = a0.clone()
                    exp[2, 2:4] = 0.0
                    a0 = exp
                assert _same_bits(a, a0), f"{what}: the skipped step changed {name}"
            st = b.stats.tolist()
            assert st[0] == 0 and st[1] == 1 and st[2] == 0 and st[3] == 0 and st[5] == 0, (what, st)
            assert not np.isfinite(st[4]) and b.skip_flag() == 1, (what, st)
            if b.tab is not None:
                b.tab[2, 2:4] = start.tab[2, 2:4]   # the repeated step's GEMMs collect their maxima again
            b.guarded_step(g1.clone())
            _assert_same(b, want, f"{what}: the clean step after the skip")
            st = b.stats.tolist()
            assert st[0] == 1 and st[1] == 1 and b.skip_flag() == 0, (what, st)
            assert abs(st[4] - float(want.state[1].sqrt())) <= _ulp32(st[4]), (what, st)


def test_overflowing_sum_of_squares_counts_as_non_finite():
    """finite values whose squares overflow fp32: no norm can be formed, the step is skipped (include/adnm_hip.h says so)"""
    b = Bufs(1028, "none")
    before = b.clone()
    g = torch.full((1028,), 1e20, device=DEV)
    b.guarded_step(g)
    _assert_same(b, before, "overflowing norm")
    assert b.stats.tolist()[:2] == [0.0, 1.0]


def test_guard_reads_max_norm_from_hyper_and_loss_stat_sorts_its_input():
    n = 1028
    b = Bufs(n, "none")
    g = _vals("g0", n)
    norm = float(g.double().pow(2).sum().sqrt())
    for hyper_max, clipped in ((norm * 1.5, 0), (norm * 0.5, 1), (0.0, 0)):
        b.stats.zero_()
        hyper = torch.tensor([1e-3, hyper_max], dtype=torch.float32, device=DEV)
        # by-value max_norm says the opposite: the device-resident one must win
        lib.call("adnm_step_guard", g.data_ptr(), n, b.state.data_ptr(), norm * 0.5 if not clipped else norm * 1.5, hyper.data_ptr(),
                 b.ws.data_ptr(), b.ws.numel(), b.stats.data_ptr(), _stream())
        assert b.stats.tolist()[5] == clipped, hyper_max
    b.stats.zero_()
    losses = [0.25, float("inf"), 1.5, float("nan"), float("-inf"), 3.0]
    held = [torch.tensor(v, device=DEV) for v in losses]
    for v in held:
        lib.call("adnm_loss_stat", v.data_ptr(), b.stats.data_ptr(), _stream())
    st = b.stats.tolist()
    assert st[6] == 4.75 and st[7] == 3 and st[:6] == [0.0] * 6


# ---------------------------------------------------------------------------------------------------------------- the trainer
def _unet64():
    from models.ADNMUNet import create_ADNMUNet
    model = create_ADNMUNet(5, 20, 6, img_size=64)
    recipe.fill_parameters(model)
    return model.to(DEV).train()


def _trainer(**kw):
    from models.loss import enRainfallLoss
    kw.setdefault("max_norm", 0.025)
    return FlatTrainer(_unet64(), enRainfallLoss(0.57, 0.25, gamma=0.0), lr=1e-3, betas=(0.9, 0.999), eps=1e-9, weight_decay=1e-2, use_graph=True, **kw)


def _batches(k, name):
    frames = recipe.radar_batch(k, 25, 64, name=name).to(DEV)
    return [(frames[i:i + 1, :5].contiguous(), frames[i:i + 1, 5:].contiguous()) for i in range(k)]


def _poisoned(x):
    """a single inf pixel in the middle input frame: the first convolution spreads it, the norms behind it turn it into NaN, and it
    reaches the gradient of every parameter"""
    x = x.clone()
    x[0, 2, 0, 31, 17] = float("inf")
    return x


def _snapshot(tr):
    """everything an optimiser step writes"""
    out = {"flat_p": tr.flat_p.clone(), "exp_avg": tr.exp_avg.clone(), "exp_avg_sq": tr.exp_avg_sq.clone(), "state": tr.state.clone()}
    if tr.shadow is not None:
        out["shadow"] = tr.shadow.clone()
    if tr.fp8:
        out["qtab"], out["qstate"] = ops.QUANT.snapshot(tr.flat_p.device)
    return out


def _assert_snap(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert _same_bits(a[k], b[k]), f"{what}: {k} differs"


def _twin_and_skip(prec, monkeypatch, tail):
    """the body of the two tests below.  tail: overlap=True — the backward cut into stage graphs and the guarded sequence captured and
    replayed as the TAIL GRAPH (hyper-parameters from device memory); else one graph and the guarded sequence launched eagerly.
    (a) three steps with the monitor leave every optimiser tensor bitwise what the twin without it holds; (b) a fourth step on an
    input with one inf pixel (frame 2, pixel (31, 17): the gradient it leaves is not finite — the test asserts the skip) changes none
    of them and counts one skip; a fifth, clean step equals the twin's fourth.  fp8: a calibration period of 2 instead of 16, so that
    the steps of this test — the skipped one too — are recording steps and make new scales."""
    monkeypatch.setattr(ops.QUANT, "period", 2)
    (x, t), (x4, t4) = _batches(2, "guard.twin")
    ops.set_mfma_precision(prec)
    try:
        ops.QUANT.reset()
        twin = _trainer(overlap=tail)
        try:
            for _ in range(3):
                twin.step(x, t)
            assert (twin.tail is not None) == tail
            after3 = _snapshot(twin)
            twin.step(x4, t4)
            after4 = _snapshot(twin)
            assert twin._stats is None
        finally:
            twin.close()
        del twin
        ops.QUANT.reset()
        tr = _trainer(monitor=True, overlap=tail)
        try:
            tr.prepare(x, t)
            assert (tr.tail is not None) == tail and tr.staged == tail
            # the tail's warm-up ran the guard and one optimiser pass for real: prepare() puts the block back with the optimiser state
            assert not tr._stats.view(torch.int32).any() and not tr.state.any() and not tr.exp_avg.any(), "prepare() left a trace"
            for _ in range(3):
                tr.step(x, t)
            assert tr.shadow_mode == {"f32": 0, "bf16": 1, "fp8": 2}[prec] and tr.graph is not None
            _assert_snap(_snapshot(tr), after3, "three monitored steps")
            tr.step(_poisoned(x4), t4)
            got = _snapshot(tr)
            assert not torch.isfinite(tr.flat_g).all(), "the poisoned input left the gradient finite: choose another pixel"
            if prec == "fp8":
                # the skipped step was a recording one (flags set by step 3); the maxima its GEMMs collected are gone — the call-site
                # records are what step 3 left, with zero maxima — and the weight records keep the max |w| step 3's optimiser pass gathered
                nrec = len(ops.QUANT.dump(x.device))
                tab = got["qtab"][:nrec]
                sites = tab[:, 4] > 0
                assert bool(sites.any()) and bool((~sites).any()) and bool((tab[:, 6] == 1).all())
                assert bool((tab[sites][:, 2:4] == 0).all()) and bool((tab[~sites][:, 3] > 0).any())
            _assert_snap(got, after3, "the skipped step")
            st = tr.stats()
            assert st["skipped"] == 1 and st["steps"] == 3 and not np.isfinite(st["last_norm"]), st
            tr.step(x4, t4)
            _assert_snap(_snapshot(tr), after4, "the clean step after the skip")
            st = tr.stats()
            assert st["skipped"] == 1 and st["steps"] == 4 and abs(st["last_norm"] - float(tr.grad_norm())) <= _ulp32(st["last_norm"]), st
        finally:
            tr.close()
        assert tr._stats is None
    finally:
        ops.set_mfma_precision("f32")
        ops.QUANT.reset()


@pytest.mark.parametrize("prec", ["f32", "bf16", "fp8"])
def test_monitored_trainer_equals_its_twin_and_skips_a_poisoned_step(prec, monkeypatch):
    """one forward / backward graph, the guarded sequence launched eagerly behind it (what one GPU runs by default)"""
    _twin_and_skip(prec, monkeypatch, tail=False)


@pytest.mark.parametrize("prec", ["f32", "bf16", "fp8"])
def test_monitored_tail_graph_equals_its_twin_and_skips_a_poisoned_step(prec, monkeypatch):
    """the same through the captured tail graph: guard, guarded table update and guarded AdamW replayed, the skip decided and obeyed
    where the host cannot intervene"""
    _twin_and_skip(prec, monkeypatch, tail=True)


def _stats_vs_twin(tail):
    """five clean steps on five batches.  max_norm: the midpoint between the 2nd and 3rd largest norms of a first twin run; the
    reference is a second twin WITH that threshold (the threshold moves the trajectory), read with .item() after every step.
    tail: the staged form with the captured tail graph.  The monitored trainer is then built and captured with max_norm = 0.025, below
    every norm of the run, and the threshold is assigned AFTER prepare(): the guard's clip count is right only if the replayed
    guard reads hyper[1] from device memory, as the AdamW kernels do."""
    data = _batches(5, "guard.stats")

    def twin_run(max_norm):
        tw = _trainer(max_norm=max_norm, overlap=tail)
        try:
            norms, losses = [], []
            for x, t in data:
                losses.append(tw.step(x, t).item())
                norms.append(tw.grad_norm().item())
            return norms, losses
        finally:
            tw.close()
    first, _ = twin_run(0.025)
    top = sorted(first, reverse=True)
    mid = 0.5 * (top[1] + top[2])
    norms, losses = twin_run(mid)
    print(f"norms of the first twin {first}; threshold {mid}; norms of the reference twin {norms}; losses {losses}")
    mid32 = float(np.float32(mid))
    assert all(abs(v - mid32) > 1e-3 * mid32 for v in norms), "a norm sits on the threshold: choose other batches"
    tr = _trainer(max_norm=0.025 if tail else mid, monitor=True, overlap=tail)
    try:
        tr.prepare(*data[0])
        assert (tr.tail is not None) == tail
        assert tr._stats is not None and not tr._stats.view(torch.int32).any(), "prepare() alone must leave the block zero"
        if tail:
            assert all(v > 0.025 * 1.001 for v in norms), "the captured threshold must differ from the assigned one in its clip count"
            tr.max_norm = mid
        assert tr.stats()["steps"] == 0
        for x, t in data:
            tr.step(x, t)
        st = tr.stats()
        print(st)
        assert st["steps"] == 5 and st["skipped"] == 0 and st["loss_nonfinite"] == 0
        want_clips = sum(v > mid32 for v in norms)
        assert 0 < want_clips < 5 and st["clip_count"] == want_clips and st["clip_rate"] == want_clips / 5
        assert abs(st["norm_sum"] - sum(norms)) <= 1e-6 * sum(norms)
        assert abs(st["loss_sum"] - sum(losses)) <= 1e-6 * abs(sum(losses))
        assert st["norm_mean"] == st["norm_sum"] / 5
        assert abs(st["norm_max"] - max(norms)) <= _ulp32(max(norms))
        assert abs(st["last_norm"] - norms[-1]) <= _ulp32(norms[-1])
        assert tr.stats(reset=True) == st
        zero = tr.stats()
        assert all(v == 0 for v in zero.values()), zero
        tr.step(*data[0])
        tr.reset_stats()
        assert not tr._stats.view(torch.int32).any()
    finally:
        tr.close()


def test_statistics_agree_with_per_step_item_reads():
    _stats_vs_twin(tail=False)


def test_statistics_through_the_tail_graph_follow_the_device_resident_threshold():
    _stats_vs_twin(tail=True)


def test_accumulation_skips_the_whole_cycle():
    """accum_steps=2: a poisoned SECOND micro-batch reaches the guard through the accumulator; the cycle is skipped, ends like any
    other, and the next clean cycle is the twin's, bit for bit"""
    data = _batches(4, "guard.accum")
    twin = _trainer(accum_steps=2)
    try:
        losses = [float(twin.step(x, t)) for x, t in data]
        want = _snapshot(twin)
    finally:
        twin.close()
    tr = _trainer(accum_steps=2, monitor=True)
    try:
        tr.step(*data[0])
        tr.step(*data[1])
        before = _snapshot(tr)
        tr.step(*data[2])
        assert tr.micro_step == 1
        bad = float(tr.step(_poisoned(data[3][0]), data[3][1]))
        assert tr.micro_step == 0
        _assert_snap(_snapshot(tr), before, "the skipped cycle")
        st = tr.stats()
        assert st["steps"] == 1 and st["skipped"] == 1, st
        tr.step(*data[2])
        tr.step(*data[3])
        assert tr.micro_step == 0
        _assert_snap(_snapshot(tr), want, "the clean cycle after the skipped one")
        st = tr.stats()
        finite = [losses[0], losses[1], losses[2], losses[2], losses[3]] + ([bad] if np.isfinite(bad) else [])
        print(f"loss of the poisoned micro-batch: {bad}; {st}")
        assert st["steps"] == 2 and st["skipped"] == 1 and st["loss_nonfinite"] == (0 if np.isfinite(bad) else 1), st
        assert abs(st["loss_sum"] - sum(finite)) <= 1e-6 * abs(sum(finite)), (st, finite)
    finally:
        tr.close()


def test_nothing_new_when_the_monitor_is_off(monkeypatch):
    called = []
    real = lib.call

    def spy(name, *a):
        called.append(name)
        return real(name, *a)
    monkeypatch.setattr(lib, "call", spy)
    (x, t), = _batches(1, "guard.off")
    tr = _trainer()
    try:
        tr.step(x, t)
        tr.step(x, t)
        assert "adnm_adamw_step" in called, "the spy saw nothing"
        assert not set(called) & set(NEW_ENTRY_POINTS), set(called) & set(NEW_ENTRY_POINTS)
        assert tr._stats is None and tr.monitor is False
        with pytest.raises(RuntimeError, match="monitor=False"):
            tr.stats()
        with pytest.raises(RuntimeError, match="monitor=False"):
            tr.reset_stats()
    finally:
        tr.close()
