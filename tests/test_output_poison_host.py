"""The output poison of tests/util.py on CPU tensors: what poisoned_outputs fills, what it lets through, what it records, and what
unwritten() reports (the GPU sweep that uses it: tests/test_output_contract_gpu.py)."""
import pytest
import torch

from adnm_hip import ops
from util import POISONED_MODULES, WORKSPACE, bits, output_pattern, pattern_mask, poison_bits, poisoned_outputs, unwritten

CPU = torch.device("cpu")
DTYPES = [torch.float32, torch.bfloat16, torch.float64, torch.float16, torch.int8, torch.uint8, torch.int16, torch.int32, torch.int64, torch.bool,
          torch.float8_e4m3fn]


def test_pattern_0_is_the_poison_the_column_tests_use_and_pattern_1_differs():
    for dt in (torch.float32, torch.bfloat16):
        assert output_pattern(dt, 0)[1] == poison_bits(dt) and output_pattern(dt, 1)[1] != poison_bits(dt)
    for dt in DTYPES:
        assert output_pattern(dt, 0)[1] != output_pattern(dt, 1)[1]
    assert output_pattern(torch.uint8, 0)[1] == 0x5A and output_pattern(torch.int32, 0)[1] == 0x5A5A5A5A
    assert output_pattern(torch.int32, 1)[1] == 0xA5A5A5A5 - (1 << 32) and output_pattern(torch.int64, 1)[1] == 0xA5A5A5A5A5A5A5A5 - (1 << 64)


@pytest.mark.parametrize("pattern", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_every_dtype_arrives_filled(monkeypatch, dtype, pattern):
    with poisoned_outputs(monkeypatch, pattern) as p:
        a = ops.torch.empty((3, 5), dtype=dtype, device=CPU)
        b = ops.torch.empty_like(a)
        c = ops.torch.empty_like(torch.zeros((4, 6), dtype=dtype).t())          # a strided layout is kept and filled too
    assert c.shape == (6, 4) and c.stride() == (1, 6)
    for t in (a, b, c):
        assert t.dtype == dtype and bool(pattern_mask(t, pattern).all()) and not bool(pattern_mask(t, 1 - pattern).any())
        if dtype.is_floating_point and dtype != torch.float8_e4m3fn:
            assert bool(torch.isnan(t.float()).all()), "a floating poison is a NaN"
        else:
            raw = torch.as_strided(t, (t.numel(),), (1,)).view(torch.uint8)   # the memory itself (a copy of a bool would normalise it)
            assert bytes(raw.tolist()) == bytes([(0x5A, 0xA5)[pattern]]) * (t.numel() * t.element_size())
    assert len(p.records) == 3


def test_the_proxy_forwards_everything_else_and_ends_with_the_context(monkeypatch):
    import importlib
    mods = [importlib.import_module(n) for n in POISONED_MODULES]
    assert len(mods) == 7
    with poisoned_outputs(monkeypatch, 0) as p:
        for m in mods:
            assert m.torch is p
        assert ops.torch.float32 is torch.float32 and ops.torch.autograd.Function is torch.autograd.Function and ops.torch.zeros is torch.zeros
        assert float(ops.torch.zeros(3).sum()) == 0.0 and not p.records, "only empty / empty_like are recorded"
    for m in mods:
        assert m.torch is torch
    assert ops._ws(32, CPU).numel() == 32 and len(p.records) == 0


def test_meta_passes_through_unfilled_and_unrecorded(monkeypatch):
    with poisoned_outputs(monkeypatch, 0) as p:
        t = ops.torch.empty((4, 3, 2), device="meta")
        assert t.device.type == "meta" and t.stride() == (6, 2, 1)
        assert not p.records


def test_records_name_the_caller_and_tag_workspaces(monkeypatch):
    def some_wrapper():
        mu = ops.torch.empty(7, dtype=torch.float32)
        return mu
    with poisoned_outputs(monkeypatch, 1) as p:
        some_wrapper()
        ws = ops._ws(40, CPU)                      # the real ops._ws, whose `torch` is the proxy now
        take = ops.GRADS.take(0, (2, 3), CPU) if hasattr(ops, "GRADS") else None
    assert bool(pattern_mask(ws, 1).all()), "a workspace is poisoned as well"
    t, site, role, where = p.records[0]
    assert site == "test_output_poison_host.py some_wrapper" and role == "mu" and where.startswith("test_output_poison_host.py:") and t.numel() == 7
    assert p.records[1][2] == WORKSPACE and p.records[1][1] == "test_output_poison_host.py test_records_name_the_caller_and_tag_workspaces"
    if take is not None:
        assert p.records[2][1] == "ops.py take" and bool(pattern_mask(take, 1).all())


def _two_runs(monkeypatch, body):
    recs = []
    for pattern in (0, 1):
        with poisoned_outputs(monkeypatch, pattern) as p:
            body(pattern)
        recs.append(p.records)
    return recs


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64, torch.uint8, torch.int32, torch.bool], ids=str)
def test_unwritten_flags_exactly_the_planted_tail(monkeypatch, dtype):
    """a 'kernel' that writes all but the last 3 of 1030 elements, and a second output it writes in full"""
    def body(pattern):
        y = ops.torch.empty(1030, dtype=dtype)
        full = ops.torch.empty((5, 6), dtype=dtype)
        ws = ops._ws(64, CPU)                      # never written: a workspace is not this check's business
        y[:1027] = torch.ones(1027).to(dtype)
        full.copy_(torch.ones(5, 6).to(dtype))
    r0, r1 = _two_runs(monkeypatch, body)
    found = unwritten(r0, r1)
    assert list(found) == [("test_output_poison_host.py body", "y")]
    n, where, first = found[("test_output_poison_host.py body", "y")]
    assert (n, first) == (3, 1027) and where.startswith("test_output_poison_host.py:")


def test_a_written_byte_that_equals_a_pattern_is_not_reported(monkeypatch):
    """a label or colour byte may be 0x5A or 0xA5, an int32 count 0x5A5A5A5A: written in both runs, it matches one run's pattern only"""
    def body(pattern):
        lab = ops.torch.empty(16, dtype=torch.uint8)
        cnt = ops.torch.empty(4, dtype=torch.int32)
        lab.copy_(torch.tensor([0x5A, 0xA5] * 8, dtype=torch.uint8))
        cnt.copy_(torch.tensor([0x5A5A5A5A, 0xA5A5A5A5 - (1 << 32), 0, 1], dtype=torch.int32))
    r0, r1 = _two_runs(monkeypatch, body)
    assert int(pattern_mask(r0[0][0], 0).sum()) == 8 and int(pattern_mask(r1[0][0], 1).sum()) == 8, "each run alone sees its own pattern"
    assert unwritten(r0, r1) == {}


def test_unwritten_refuses_runs_that_allocated_differently(monkeypatch):
    r0, r1 = _two_runs(monkeypatch, lambda pattern: ops.torch.empty(4 + pattern))
    with pytest.raises(AssertionError, match="same tensors in the same order"):
        unwritten(r0, r1)


def test_a_float_result_never_equals_the_poison():
    """arithmetic on the poison gives the canonical NaN or keeps the payload; a value a kernel computes from clean inputs is neither"""
    x = torch.empty(4)
    bits(x).fill_(poison_bits(torch.float32))
    assert not bool(pattern_mask(torch.zeros(4), 0).any()) and bool(pattern_mask(x, 0).all()) and not bool(pattern_mask(x, 1).any())
