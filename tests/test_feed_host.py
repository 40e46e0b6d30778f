"""The host side of the resident data feed, without a GPU: EpochOrder against the real torch DataLoader (same generator,
same batches, epoch after epoch), the split over ranks, resume in the middle of an epoch, and adnm_batch_fetch at the C boundary
(declared, exported, additive, refusing bad arguments before any launch)."""
import ctypes
import io

import pytest
import torch
from torch.utils.data import DataLoader

from adnm_hip import lib
from adnm_hip.dataio import EpochOrder


def _loader_epochs(n, batch, epochs, shuffle=True, generator=None):
    """the real thing: the sample tags of every batch of `epochs` consecutive epochs"""
    data = [torch.tensor([i]) for i in range(n)]
    loader = DataLoader(data, batch_size=batch, shuffle=shuffle, drop_last=True, generator=generator)
    return [[b.flatten().tolist() for b in loader] for _ in range(epochs)]


def _order_epochs(order, epochs):
    out = []
    for _ in range(epochs):
        order.next_epoch()
        out.append([order.next_batch().tolist() for _ in range(len(order))])
    return out


def test_order_equals_the_real_loader_with_an_explicit_generator():
    g1, g2 = torch.Generator().manual_seed(1234), torch.Generator().manual_seed(1234)
    want = _loader_epochs(11, 4, 3, generator=g1)
    got = _order_epochs(EpochOrder(11, 4, shuffle=True, generator=g2), 3)
    assert len(want[0]) == 2 and want[0] != want[1], "the fixture itself: two batches per epoch, a new order every epoch"
    assert got == want
    assert torch.equal(g1.get_state(), g2.get_state()), "the generator is left where the loader leaves it"


def test_order_equals_the_real_loader_with_the_default_generator():
    torch.manual_seed(77)
    want = _loader_epochs(11, 4, 3)
    state = torch.get_rng_state()
    torch.manual_seed(77)
    got = _order_epochs(EpochOrder(11, 4, shuffle=True), 3)
    assert got == want
    assert torch.equal(state, torch.get_rng_state())


def test_sequential_order_equals_the_sequential_loader():
    order = EpochOrder(11, 4, shuffle=False)
    assert order.next_epoch().dtype == torch.int32 and order.perm.tolist() == list(range(11))
    assert _order_epochs(EpochOrder(11, 4, shuffle=False), 2) == _loader_epochs(11, 4, 2, shuffle=False) == [[[0, 1, 2, 3], [4, 5, 6, 7]]] * 2


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_split_the_single_process_batch(world):
    n, B = 26, 2
    want = _loader_epochs(n, B * world, 2, generator=torch.Generator().manual_seed(5))
    ranks = [EpochOrder(n, B, generator=torch.Generator().manual_seed(5), rank=r, world=world) for r in range(world)]
    assert all(len(o) == n // (B * world) == len(want[0]) for o in ranks)
    for epoch in range(2):
        for o in ranks:
            o.next_epoch()
        for step in range(len(ranks[0])):
            parts = [o.next_batch().tolist() for o in ranks]
            assert all(len(p) == B for p in parts)
            assert sum(parts, []) == want[epoch][step]


def test_resume_in_the_middle_of_an_epoch():
    whole = _order_epochs(EpochOrder(11, 2, generator=torch.Generator().manual_seed(9)), 3)
    a = EpochOrder(11, 2, generator=torch.Generator().manual_seed(9))
    a.next_epoch()
    for _ in range(len(a)):
        a.next_batch()
    a.next_epoch()
    a.next_batch()
    buf = io.BytesIO()
    torch.save({"feed": a.state_dict(), "best": 1.5}, buf)       # beside other schedule_stats entries, through torch's default loader
    buf.seek(0)
    sd = torch.load(buf)["feed"]
    b = EpochOrder(11, 2, generator=torch.Generator().manual_seed(4242))
    b.load_state_dict(sd)
    assert (b.epoch, b.pos) == (2, 1)
    rest = [b.next_batch().tolist() for _ in range(len(b) - 1)]
    with pytest.raises(IndexError):
        b.next_batch()
    b.next_epoch()
    nxt = [b.next_batch().tolist() for _ in range(len(b))]
    assert rest == whole[1][1:] and nxt == whole[2]
    with pytest.raises(ValueError):
        EpochOrder(12, 2).load_state_dict(sd)


def test_resume_with_the_default_generator():
    torch.manual_seed(3)
    whole = _order_epochs(EpochOrder(7, 3), 2)
    torch.manual_seed(3)
    a = EpochOrder(7, 3)
    a.next_epoch()
    a.next_batch()
    sd = a.state_dict()
    torch.manual_seed(999)
    b = EpochOrder(7, 3)
    b.load_state_dict(sd)
    assert [b.next_batch().tolist()] == whole[0][1:]
    b.next_epoch()
    assert [b.next_batch().tolist() for _ in range(len(b))] == whole[1]


def test_refusals():
    with pytest.raises(ValueError, match="no full batch"):
        EpochOrder(5, 3, world=2)
    with pytest.raises(ValueError):
        EpochOrder(8, 2, rank=2, world=2)
    o = EpochOrder(5, 2)
    with pytest.raises(RuntimeError, match="no epoch yet"):
        o.next_batch()
    o.next_epoch()
    o.next_batch(), o.next_batch()
    with pytest.raises(IndexError, match="step 2 of an epoch of 2"):
        o.next_batch()


def test_batch_fetch_is_declared_and_exported_and_the_abi_version_stays():
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    assert "adnm_batch_fetch" in protos, "adnm_batch_fetch is not declared in include/adnm_hip.h"
    assert hasattr(so, "adnm_batch_fetch"), "adnm_batch_fetch declared but not exported"
    ret, args = protos["adnm_batch_fetch"]
    assert ret == "int" and args[-1] == "adnm_stream_t" and args[4] == "const int32_t*" and len(args) == 12
    assert lib.load().adnm_abi_version() == 11


def test_batch_fetch_checks_its_arguments_on_the_host():
    f = lib.load().adnm_batch_fetch
    p = 4096   # stands for a device address: nothing is dereferenced or launched before a refusal

    def refused(what, store=p, n=7, T=5, hw=64, order=p, olen=7, pos=0, x=p, tgt=p, B=3, T_in=2):
        assert f(store, n, T, hw, order, olen, pos, x, tgt, B, T_in, None) == -1, what
        return lib.last_error()

    for k in ("store", "order", "x", "tgt"):
        assert "null pointer" in refused(k, **{k: None})
    assert "batch must be in [1, 65535]" in refused("B = 0", B=0)
    assert "batch must be in [1, 65535]" in refused("B over the grid limit", B=65536, olen=1 << 20, n=1 << 20)
    assert "T_in" in refused("T_in = 0", T_in=0)
    assert "T_in" in refused("T_in = T", T_in=5)
    assert "T_in" in refused("T_in > T", T_in=6)
    assert "hw" in refused("hw = 0", hw=0)
    assert "outside an order" in refused("pos < 0", pos=-1)
    assert "outside an order" in refused("pos near the end of int64", pos=(1 << 63) - 2)
    assert "outside an order" in refused("pos + B > order_len", pos=5)
    assert "2^31" in refused("n_samples = 2^31", n=1 << 31)
    assert "2^31" in refused("order_len = 2^31", olen=1 << 31)
    assert "4-byte aligned" in refused("x at an odd address", x=p + 2)
