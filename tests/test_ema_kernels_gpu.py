"""adnm_ema_update / adnm_ema_swap on flat buffers, element by element: the update against its fp64 statement (tests/ema_ref.py), the
exact cases d = 0 and d = 1, the warm-up of d from the device's step counter, the counter in info, the skip flag of a monitored step,
the swap on raw bit patterns, and the refusals on entry.  Every buffer a kernel writes lies between poisoned margins."""
import pytest
import torch

from adnm_hip import lib
from ema_ref import assert_ema_step, warmup_decay
from util import assert_pads_untouched, bits, embed

pytestmark = pytest.mark.gpu
DEV = "cuda"
# one partial 16-byte trip; a few workgroups; many; one quad more than a full pass of the kernels' grid (2048 workgroups x 256 lanes x 2
# quads per trip, include/adnm_hip.h): lane 0 of workgroup 0 takes a second grid-stride trip, with only its first quad in range
FULL_PASS = 2048 * 256 * 2 * 4
SIZES = [4, 1028, 1048580, FULL_PASS + 4]
PAD = 4   # floats: the payload stays 16-byte aligned


def _st():
    return torch.cuda.current_stream().cuda_stream


def _flat(t, poison):
    """1-D fp32 tensor -> (buffer with poisoned margins, the aligned view holding t)"""
    buf, view = embed(t.reshape(1, -1), PAD, PAD, poison=poison)
    return buf, view[0]


def _info():
    buf, view = embed(torch.zeros(1, 2, device=DEV), 1, 1, poison="bits")
    return buf, view[0]


def _state(t):
    return torch.tensor([float(t), 0.0, 0.0, 0.0], dtype=torch.float32, device=DEV)


def _rand(n, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(n, device=DEV, generator=g) * scale


def _update(p, ema, state, decay, warmup, info, stats=None):
    lib.call("adnm_ema_update", p.data_ptr(), ema.data_ptr(), p.numel(), state.data_ptr(), float(decay), int(warmup), info.data_ptr(),
             None if stats is None else stats.data_ptr(), _st())


@pytest.mark.parametrize("n", SIZES)
def test_update_against_the_fp64_statement_and_info_counts_calls(n):
    pbuf, p = _flat(_rand(n, 1), "nan")
    ebuf, ema = _flat(_rand(n, 2, 3.0), "bits")
    ibuf, info = _info()
    state = _state(7)
    for call, (decay, warmup) in enumerate([(0.999, 0), (0.999, 1), (0.9, 0)], start=1):
        before = ema.clone()
        _update(p, ema, state, decay, warmup, info)
        d, count = info.tolist()
        assert count == call, f"info[1] = {count} after {call} calls"
        want = warmup_decay(decay, 7) if warmup else decay
        assert abs(d - want) <= 4 * 2.0 ** -24 * want, (d, want)
        assert_ema_step(ema, before, p, d, f"n={n} decay={decay} warmup={warmup}")
        assert not torch.equal(ema, before)
        assert_pads_untouched(ebuf, PAD, n, "ema")
        assert_pads_untouched(ibuf, 1, 2, "info")
    assert bool(torch.isnan(pbuf[0, :PAD]).all()) and bool(torch.isnan(pbuf[0, PAD + n:]).all())


@pytest.mark.parametrize("n", SIZES)
def test_decay_0_copies_p_and_decay_1_leaves_ema_alone(n):
    p = _flat(_rand(n, 3), "nan")[1]
    ebuf, ema = _flat(_rand(n, 4), "bits")
    ibuf, info = _info()
    before = ema.clone()
    _update(p, ema, _state(3), 1.0, 0, info)
    assert torch.equal(bits(ema), bits(before)), "decay = 1 changed bits of ema"
    assert info.tolist() == [1.0, 1.0]
    _update(p, ema, _state(3), 0.0, 0, info)
    assert torch.equal(bits(ema), bits(p)), "decay = 0 did not leave ema bit-equal to p"
    assert info.tolist() == [0.0, 2.0]
    assert_pads_untouched(ebuf, PAD, n, "ema")
    assert_pads_untouched(ibuf, 1, 2, "info")


# t = 79 / 80 / 81 is where (1 + t) / (10 + t) crosses 0.9 (81 / 90); for 0.999 the crossing lies at t = 8990: every t here is on the ramp
@pytest.mark.parametrize("decay", [0.9, 0.999])
@pytest.mark.parametrize("t", [1, 2, 79, 80, 81, 89, 90, 1000])
def test_warmup_follows_the_step_counter(decay, t):
    p = _flat(_rand(4, 5), "nan")[1]
    ebuf, ema = _flat(_rand(4, 6), "bits")
    ibuf, info = _info()
    before = ema.clone()
    _update(p, ema, _state(t), decay, 1, info)
    d = info.tolist()[0]
    ramp = (1.0 + t) / (10.0 + t)
    want = min(decay, ramp)
    assert abs(d - want) <= 4 * 2.0 ** -24 * want, f"t={t} decay={decay}: d = {d!r}, fp64 {want!r}"
    decay32 = float(torch.tensor(decay, dtype=torch.float32))
    assert (d == decay32) == (decay32 <= ramp), f"t={t} decay={decay}: d = {d!r} is on the wrong side of the min (ramp {ramp!r})"
    assert_ema_step(ema, before, p, d, f"t={t} decay={decay}")
    assert_pads_untouched(ebuf, PAD, 4, "ema")
    assert_pads_untouched(ibuf, 1, 2, "info")


@pytest.mark.parametrize("n", [4, 1028, FULL_PASS + 4])
def test_skip_flag_leaves_ema_and_info_alone(n):
    p = _flat(_rand(n, 7), "nan")[1]
    ebuf, ema = _flat(_rand(n, 8), "bits")
    ibuf, info = _info()
    info.copy_(torch.tensor([0.25, 5.0]))
    stats = torch.zeros(9, dtype=torch.float64, device=DEV)   # adnm_step_guard's block: eight doubles, then the skip flag as an int
    stats.view(torch.int32)[16] = 1
    ema0, ebuf0, ibuf0 = ema.clone(), ebuf.clone(), ibuf.clone()
    _update(p, ema, _state(4), 0.5, 1, info, stats)
    assert torch.equal(bits(ebuf), bits(ebuf0)), "a skipped step wrote ema"
    assert torch.equal(bits(ibuf), bits(ibuf0)), "a skipped step wrote info"
    stats.view(torch.int32)[16] = 0   # the same block, flag clear: the update runs
    _update(p, ema, _state(4), 0.5, 1, info, stats)
    d, count = info.tolist()
    assert count == 6.0 and abs(d - 5.0 / 14.0) <= 4 * 2.0 ** -24 * (5.0 / 14.0), (d, count)   # (1 + 4) / (10 + 4) < 0.5
    assert_ema_step(ema, ema0, p, d, f"n={n}, flag clear")
    assert_pads_untouched(ebuf, PAD, n, "ema")
    assert_pads_untouched(ibuf, 1, 2, "info")


def _patterns(n, seed):
    """random 32-bit patterns as fp32, NaNs with payloads among them"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    raw = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int64, device=DEV, generator=g).to(torch.int32)
    raw[::3] |= 0x7FC00000            # quiet NaNs, random payloads and signs
    raw[1::7] = (raw[1::7] & ~0x00400000) | 0x7F800001   # signalling NaNs
    return raw.view(torch.float32)


@pytest.mark.parametrize("n", SIZES)
def test_swap_exchanges_bit_patterns_and_twice_is_the_identity(n):
    a, b = _patterns(n, 9), _patterns(n, 10)
    assert bool(torch.isnan(a).any()) and not torch.equal(bits(a), bits(b))
    pbuf, p = _flat(a, "bits")
    ebuf, ema = _flat(b, "bits")
    lib.call("adnm_ema_swap", p.data_ptr(), ema.data_ptr(), n, _st())
    assert torch.equal(bits(p), bits(b)) and torch.equal(bits(ema), bits(a)), "one swap did not exchange the buffers"
    lib.call("adnm_ema_swap", p.data_ptr(), ema.data_ptr(), n, _st())
    assert torch.equal(bits(p), bits(a)) and torch.equal(bits(ema), bits(b)), "two swaps are not the identity"
    assert_pads_untouched(pbuf, PAD, n, "p")
    assert_pads_untouched(ebuf, PAD, n, "ema")


def test_refusals_on_entry_write_nothing():
    so = lib.load()
    buf = _patterns(64, 11)
    keep = buf.clone()
    info = torch.full((2,), 3.0, device=DEV)
    state = _state(1)
    P, E, S, I = buf.data_ptr(), buf.data_ptr() + 128, state.data_ptr(), info.data_ptr()
    upd = lambda p, e, n, s=S, i=I: so.adnm_ema_update(p, e, n, s, 0.5, 0, i, None, _st())
    swap = lambda p, e, n: so.adnm_ema_swap(p, e, n, _st())
    for call, text in [(lambda: upd(P, E, 0), "multiple of 4"), (lambda: upd(P, E, 6), "multiple of 4"), (lambda: upd(P + 4, E, 8), "16-byte aligned"),
                       (lambda: upd(P, E + 4, 8), "16-byte aligned"), (lambda: upd(None, E, 8), "null pointer"),
                       (lambda: upd(P, None, 8), "null pointer"), (lambda: upd(P, E, 8, s=None), "null pointer"),
                       (lambda: upd(P, E, 8, i=None), "null pointer"), (lambda: upd(P, P + 16, 8), "overlap"),
                       (lambda: swap(P, E, 0), "multiple of 4"), (lambda: swap(P, E, 6), "multiple of 4"),
                       (lambda: swap(P + 4, E, 8), "16-byte aligned"), (lambda: swap(P, E + 4, 8), "16-byte aligned"),
                       (lambda: swap(None, E, 8), "null pointer"), (lambda: swap(P, None, 8), "null pointer"),
                       (lambda: swap(P, P + 16, 8), "overlap"), (lambda: swap(P + 16, P, 8), "overlap"), (lambda: swap(P, P, 8), "overlap")]:
        assert call() != 0 and text in lib.last_error(), (text, lib.last_error())
    torch.cuda.synchronize()
    assert torch.equal(bits(buf), bits(keep)) and info.tolist() == [3.0, 3.0], "a refused call wrote something"
