"""Host-side logic that needs no GPU: the trainer's ownership / error path, the gradient-destination registry's
finaliser safety, the supervised multi-rank launcher of bench.py, RadarIngest's slot bookkeeping."""
import gc
import os
import subprocess
import sys
import time

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Toy(nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.a, self.b = nn.Linear(8, 16), nn.Linear(16, 4)

    def forward(self, x):
        return self.b(torch.tanh(self.a(x)))


def test_prepare_exception_path_restores_state():
    """An exception inside prepare() (here: a loss function that raises on the second call, i.e. after the dry run) must leave the
    collector enabled, no graph objects behind and the trainer reusable; close() is idempotent and drops the registration."""
    from adnm_hip import ops
    from adnm_hip.trainer import FlatTrainer
    calls = [0]

    def loss_fn(o, t):
        calls[0] += 1
        if calls[0] == 2:
            raise ValueError("boom")
        return (o - t).pow(2).mean()

    model = _Toy()
    tr = FlatTrainer(model, loss_fn, use_graph=False, fused=False)
    x, t = torch.randn(5, 8), torch.randn(5, 4)
    assert gc.isenabled()
    tr.prepare(x, t)            # first call of loss_fn: fine
    with pytest.raises(ValueError):
        tr.step(x, t)           # second call raises inside the eager step
    assert gc.isenabled()
    tr2 = FlatTrainer(_Toy(), loss_fn, use_graph=False, fused=False)
    calls[0] = 1
    with pytest.raises(ValueError):
        tr2.prepare(x, t)       # raises inside prepare's dry run
    assert gc.isenabled() and tr2.graph is None and tr2.graph2 is None and tr2.static_loss is None
    assert tr2.tail is None and tr2.sx is None and tr2.st is None
    calls[0] = 10
    tr2.prepare(x, t)           # and the same object can be prepared again
    tr2.step(x, t)
    owner = id(tr2)
    tr2.close()
    tr2.close()
    ops.GRADS.reset_claims(owner)   # drains the finaliser queue
    assert owner not in ops.GRADS._claimed and not any(o == owner for o, _ in ops.GRADS._dst.values())


def test_side_stream_keyword_is_accepted_false_and_refused_true():
    """The side-stream lane for weight gradients is gone (DESIGN.md keeps the measurements): callers that still pass side_stream=False
    construct as before, side_stream=True is refused at construction with a message that names the removal, and ops no longer has the lane's singleton."""
    from adnm_hip import ops
    from adnm_hip.trainer import FlatTrainer
    loss_fn = lambda o, t: (o - t).pow(2).mean()
    tr = FlatTrainer(_Toy(), loss_fn, use_graph=False, fused=False, side_stream=False)
    assert not hasattr(tr, "side_stream")
    with pytest.raises(ValueError, match="removed"):
        FlatTrainer(_Toy(), loss_fn, use_graph=False, fused=False, side_stream=True)
    assert not hasattr(ops, "SIDE")


def test_grad_registry_drop_is_lock_free_and_reentrant():
    """drop() is what a finaliser calls: it must not take the registry lock (the cyclic collector can run while register() / take()
    hold it on the same thread)."""
    from adnm_hip.ops import GradRegistry
    reg = GradRegistry()
    g = torch.zeros(4)
    reg.register(1, {g.data_ptr(): g})
    with reg._lock:            # as if the collector fired inside take()
        reg.drop(1)            # must return at once
        with reg._lock:        # and the lock is re-entrant for the same thread
            pass
    t = reg.take(g.data_ptr(), (4,), g.device)
    assert t.data_ptr() != g.data_ptr()   # owner 1 was forgotten before the lookup
    # a slice whose layout differs from what the caller writes is refused WITHOUT being claimed
    w = torch.zeros(2, 3, 3, 5).permute(0, 3, 1, 2)   # (2, 5, 3, 3) logical, channels-last memory
    reg.register(2, {w.data_ptr(): w})
    got = reg.take(w.data_ptr(), (2, 5, 3, 3), w.device, strides=(45, 9, 3, 1))
    assert got.data_ptr() != w.data_ptr() and w.data_ptr() not in reg.born_in_place(2)
    got = reg.take(w.data_ptr(), (2, 5, 3, 3), w.device, strides=tuple(w.stride()))
    assert got.data_ptr() == w.data_ptr() and w.data_ptr() in reg.born_in_place(2)


def test_grad_registry_hands_out_dense_slices_under_another_shape():
    """A (4d, d, 1, 1) conv weight whose gradient a GEMM writes as (4d, d): the same dense memory, so the claim succeeds with the slice
    viewed the caller's way (and is recorded: the trainer's gather then skips the copy); a non-dense layout is still refused."""
    from adnm_hip.ops import GradRegistry
    reg = GradRegistry()
    g = torch.zeros(8, 4, 1, 1)
    reg.register(7, {g.data_ptr(): g})
    t = reg.take(g.data_ptr(), (8, 4), g.device)
    assert t.shape == (8, 4) and t.data_ptr() == g.data_ptr() and g.data_ptr() in reg.born_in_place(7)
    h = torch.zeros(6, 5)[:, :4]   # not dense
    reg.register(8, {h.data_ptr(): h})
    u = reg.take(h.data_ptr(), (24,), h.device)
    assert u.data_ptr() != h.data_ptr() and h.data_ptr() not in reg.born_in_place(8)
    k = torch.zeros(8, 4)
    reg.register(9, {k.data_ptr(): k})
    v = reg.take(k.data_ptr(), (4, 8), k.device, strides=(1, 4))   # the caller would write a transposed layout: refused
    assert v.data_ptr() != k.data_ptr() and k.data_ptr() not in reg.born_in_place(9)


def test_bench_multi_rank_launcher_reports_a_dead_rank():
    """`python bench.py --gpus 2` on a box without GPUs: both ranks exit at once ("needs a GPU"); the parent must notice, stop the
    job and exit non-zero within seconds instead of waiting for a rendezvous that never happens."""
    env = dict(os.environ, ADNM_BENCH_TIMEOUT="120")
    env.pop("WORLD_SIZE", None)
    if torch.cuda.is_available():
        pytest.skip("needs a box without a GPU (on a GPU box the 2-rank job would really start)")
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "exited with status" in r.stderr and "needs a GPU" in r.stderr
    assert time.time() - t0 < 240


def test_radar_ingest_slot_bookkeeping():
    """submit, submit, take, take works; a third submit without a take raises (no staging buffer is overwritten under a copy)."""
    from adnm_hip import dataio
    ing = dataio.RadarIngest.__new__(dataio.RadarIngest)   # the bookkeeping alone: no pinned memory / device here
    ing._pending, ing._slot = [], 0
    ing._pending.append(0), ing._pending.append(1)
    with pytest.raises(RuntimeError):
        dataio.RadarIngest.submit(ing, None)
    assert ing._pending.pop(0) == 0 and ing._pending.pop(0) == 1


def test_bench_stdout_line_is_small_and_parses():
    """the driver parses ONE stdout line; it must stay under 4 kB however many kernels the profile holds.
    Canned profile = round 3's per-(kernel, shape) table (profiles/r03_kernel_shapes_bf16.tsv)."""
    import json
    import bench
    prof = {}
    with open(os.path.join(ROOT, "profiles", "r03_kernel_shapes_bf16.tsv")) as f:
        next(f)
        for row in f:
            key, n, avg_us, ms, _ = row.rstrip("\n").split("\t")
            n = max(1, round(float(n)))
            prof[key] = {"launches": 3 * n, "ms": 3 * float(ms), "bytes": 3 * n * float(key.split("@")[1])}
    assert len(prof) > 100
    pmc = {"kernels": {k.split("@")[0]: {"hbm_bytes_per_step": 1.5e8, "launches_per_step": 1} for k in prof}}
    kernels, families, roofline = bench.summarise(prof, 3, pmc, "canned " + "x" * 200, 8.5e-3, 11.0)
    assert roofline["kernel"] in kernels and roofline["traffic"] is not None and 0 < roofline["frac"] < 1
    res = {"metric": "sequences/sec training ADNM-UNet 5->20x128x128", "value": 468.4, "unit": "sequences/s", "n_gpus": 1, "steps": 20, "warmup": 10,
           "ms_per_step": 8.54, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "dtype_detail": "d" * 300,
           "data": "synthetic", "config": {"workload": "w" * 250, "per_gpu_batch": 4, "protocol": "p" * 150},
           "windows_ms_per_step": [8.5] * 5, "roofline": roofline,
           "cpu_baseline": {"value": 3.7, "unit": "sequences/s", "cores": 16, "kind": "port", "sample": "s" * 200}}
    line = bench.stdout_line(res, families, "bench_tables.json")
    assert "\n" not in line and len(line) < 4096
    back = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype", "config", "roofline", "cpu_baseline"):
        assert k in back
    assert back["roofline"]["frac"] == roofline["frac"] and 1 <= len(back["families_top"]) <= 8
    assert "kernels" not in back and "families" not in back
    # a pathological record still comes out under the cap (families dropped from the tail) ...
    fat = dict(res, dtype_detail="d" * 1500)
    assert len(bench.stdout_line(fat, families, "t.json")) < 4096
    # ... and one that cannot fit raises instead of printing a line the driver will not parse
    with pytest.raises(RuntimeError):
        bench.stdout_line(dict(res, dtype_detail="d" * 5000), families, "t.json")


def test_bench_times_exactly_the_steps_asked_for():
    """--steps K is the number of timed steps in all: the windows add up to K, at most 5 of them, lengths within one step.  The
    side files of --full's measurements are refused without it."""
    import bench
    for k in range(1, 60):
        sizes = bench.window_sizes(k)
        assert sum(sizes) == k and len(sizes) == min(5, k) and max(sizes) - min(sizes) <= 1
    assert bench.parse(["--steps", "7"]).dump_json is None
    assert bench.parse(["--full"]).dump_json == os.path.join(ROOT, "bench_tables.json")
    assert bench.parse(["--full", "--dump-prof", "p.tsv"]).dump_prof == "p.tsv"
    for bad in (["--steps", "0"], ["--dump-prof", "p.tsv"], ["--dump-json", "t.json"]):
        with pytest.raises(SystemExit):
            bench.parse(bad)


def test_bench_dump_outputs_is_a_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: loss and gradient norm as float64, the parameters as float32 in named order — all of them while they fit,
    else the same sorted sample of distinct elements on every run — and never more than 64 MB in all."""
    import numpy as np
    import bench
    assert 4 * bench.OUT_SAMPLE + 16 <= 64 << 20
    params = [torch.arange(300.0).view(3, 100), torch.arange(300.0, 305.0)]
    shapes = bench.write_outputs(str(tmp_path / "all"), torch.tensor(0.25), torch.tensor(3.0), params)
    assert shapes == {"loss": [1], "grad_norm": [1], "params": [305]}
    p = np.load(tmp_path / "all" / "params.npy")
    assert p.dtype == np.float32 and (p == np.arange(305)).all()
    assert np.load(tmp_path / "all" / "loss.npy").dtype == np.float64 and float(np.load(tmp_path / "all" / "grad_norm.npy")[0]) == 3.0
    monkeypatch.setattr(bench, "OUT_SAMPLE", 50)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.write_outputs(a, 0.25, 3.0, params)
    bench.write_outputs(b, 0.25, 3.0, params)
    sa, sb = np.load(os.path.join(a, "params.npy")), np.load(os.path.join(b, "params.npy"))
    assert sa.shape == (50,) and (sa == sb).all() and (np.diff(sa) > 0).all() and sa.max() < 305


def test_flat_trainer_refuses_unclaimed_and_doubly_claimed_parameters():
    """a parameter that receives a gradient but is named by no stage (it would never be trained, only decayed), or by two
    stages, is an error, not a silent layout decision."""
    from adnm_hip.trainer import FlatTrainer

    class M(nn.Module):
        def __init__(self, stages):
            super().__init__()
            torch.manual_seed(0)
            self.a, self.b = nn.Linear(4, 4), nn.Linear(4, 2)
            self.extra = nn.Parameter(torch.ones(()))
            self._stages = stages

        def forward(self, x):
            return self.b(torch.tanh(self.a(x))) * self.extra

        def forward_stages(self):
            s0 = lambda x: (torch.tanh(self.a(x)),)
            s1 = lambda h: (self.b(h) * self.extra,)
            return [(s0, self._stages[0](self)), (s1, self._stages[1](self))]

    x, t = torch.randn(3, 4), torch.randn(3, 2)
    loss = lambda o, tt: (o - tt).pow(2).mean()
    tr = FlatTrainer(M((lambda m: [m.a], lambda m: [m.b])), loss, use_graph=False, fused=False, overlap=True)
    with pytest.raises(RuntimeError, match="belong to no stage.*extra"):
        tr.prepare(x, t)
    tr = FlatTrainer(M((lambda m: [m.a, m.b], lambda m: [m.b])), loss, use_graph=False, fused=False, overlap=True)
    with pytest.raises(RuntimeError, match="more than one stage"):
        tr.prepare(x, t)


def test_shadow_staleness_rule_on_cpu_tensors(monkeypatch):
    """ops.ShadowSet / ShadowRegistry on CPU tensors (pointer arithmetic and version counters; the device rewrite is replaced by a
    recorder): after a write torch performs on a re-homed parameter — an in-place op, load_state_dict, a write through the flat buffer —
    lookup() rewrites the shadow before it hands it out, and only then.  A write through p.data is invisible (refresh_shadows())."""
    from adnm_hip import ops
    m = nn.Sequential(nn.Linear(8, 16), nn.Linear(16, 4))
    params = list(m.parameters())
    offs, n = [], 0
    for p in params:
        offs.append(n)
        n += (p.numel() + 3) // 4 * 4
    flat = torch.zeros(n)
    for p, o in zip(params, offs):   # re-homed as FlatTrainer._flatten does
        view = flat[o:o + p.numel()].view_as(p)
        view.copy_(p.data)
        p.data = view
    shadow = torch.zeros(n, dtype=torch.bfloat16)
    s = ops.ShadowSet(flat, shadow, 1, offs, [-1] * len(params), params)
    writes = []

    def write(collect_only=False):
        writes.append(collect_only)
        shadow.copy_(flat.to(torch.bfloat16))
        s.mark_current()
        s.valid = True
    monkeypatch.setattr(s, "write", write)
    reg = ops.ShadowRegistry()
    reg.register("trainer", s)
    w = params[2]   # the second Linear's weight
    off = offs[2]
    assert reg.lookup(w, 1) is None and not writes   # never written: not handed out
    s.refresh()
    assert writes == [False] and not s.stale()
    assert reg.lookup(w, 1) == (shadow.data_ptr() + 2 * off, 1, None) and len(writes) == 1
    assert reg.lookup(w, 2) is None and reg.lookup(w, 0) is None   # the bf16 shadow serves bf16 operands only
    assert reg.lookup(torch.zeros(4), 1) is None   # outside the flat buffer

    with torch.no_grad():
        w.mul_(2.0)   # in-place op
    assert s.stale()
    assert reg.lookup(w, 1) is not None and len(writes) == 2 and torch.equal(shadow, flat.to(torch.bfloat16))
    with torch.no_grad():
        w[:2].zero_()   # through a view of the parameter
    assert reg.lookup(w, 1) is not None and len(writes) == 3

    m.load_state_dict({k: torch.full_like(v, 0.25) for k, v in m.state_dict().items()})
    assert s.stale()
    assert reg.lookup(w, 1) is not None and len(writes) == 4 and float(shadow[off]) == 0.25

    flat.add_(1.0)   # through the flat buffer
    assert reg.lookup(params[0], 1) is not None and len(writes) == 5

    params[0].data.copy_(torch.ones_like(params[0]))   # p.data: a new alias with its own counter — not visible
    assert not s.stale() and reg.lookup(params[0], 1) is not None and len(writes) == 5

    reg.drop("trainer")
    assert reg.lookup(w, 1) is None and reg.sets() == []


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_embed_helper_reports_the_first_touched_pad(dtype):
    """tests/util.py embed / assert_pads_untouched (the strided-view GPU tests stand on them): a clean buffer passes, one overwritten pad
    element — the first pad column right of the view, last row — is reported at that position; fp32 and bf16 alike."""
    from util import embed, assert_pads_untouched, bits
    M, C, left, right = 5, 8, 8, 16
    t = (torch.arange(M * C, dtype=torch.float32).reshape(M, C) / 7).to(dtype)
    buf, view = embed(t, left, right, poison="bits")
    assert buf.shape == (M, left + C + right) and buf.dtype == dtype and view.stride() == (left + C + right, 1)
    assert view.data_ptr() == buf.data_ptr() + left * buf.element_size() and torch.equal(view, t)
    assert bool(torch.isnan(buf[:, :left]).all()) and bool(torch.isnan(buf[:, left + C:]).all())
    assert_pads_untouched(buf, left, C, "clean")
    view.mul_(2.0)   # writes inside the view are not the helper's business
    assert_pads_untouched(buf, left, C, "payload rewritten")
    buf[M - 1, left + C] = 0.0
    with pytest.raises(AssertionError, match=rf"row {M - 1}, column {left + C}\)"):
        assert_pads_untouched(buf, left, C, "one pad element")
    # a canonical NaN (what arithmetic on a poisoned neighbour would store) is not the poison either
    buf2, _ = embed(t, left, right, poison="bits")
    buf2[0, 0] = float("nan")
    with pytest.raises(AssertionError, match=r"row 0, column 0\)"):
        assert_pads_untouched(buf2, left, C, "canonical NaN")
    # input poison: plain NaN everywhere outside the view, and the integer view sees any change
    ibuf, iview = embed(t, 0, 8, poison="nan")
    snap = bits(ibuf).clone()
    assert bool(torch.isnan(ibuf[:, C:]).all()) and torch.equal(iview, t) and torch.equal(bits(ibuf), snap)
    ibuf[2, C + 1] = 1.0
    assert not torch.equal(bits(ibuf), snap)
