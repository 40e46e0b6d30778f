"""The guarded, poisoned workspace allocator of tests/util.py on CPU tensors: what it hands out, what it lets pass and what it catches
(the GPU sweep that uses it: tests/test_workspace_contract_gpu.py)."""
import pytest
import torch

from adnm_hip import ops
from util import guarded_workspaces, poison_bits

POISON = poison_bits(torch.float32)
CPU = torch.device("cpu")


@pytest.mark.parametrize("n", [4, 16, 40, 4096, 5000, 3 << 20])
def test_payload_arrives_poisoned_and_a_full_write_passes(monkeypatch, n):
    with guarded_workspaces(monkeypatch) as g:
        ws = ops._ws(n, CPU)                        # the patched allocator, as a wrapper calls it
        assert ws.dtype == torch.uint8 and ws.numel() == max(n, 16) and ws.data_ptr() % 512 == ws.untyped_storage().data_ptr() % 512
        assert bool((ws.view(torch.int32) == POISON).all()), "the payload must arrive fully poisoned"
        assert bool(torch.isnan(ws.view(torch.float32)).all())
        ws.zero_()                                  # a kernel that writes its workspace end to end
        g.check()
        assert g.calls == 1 and g.records[0][2] == n and "test_workspace_guard_host.py" in g.records[0][3]
    assert ops._ws(32, CPU).numel() == 32 and g.calls == 1, "the patch ends with the context"


def test_rear_guard_size():
    from util import GuardedWorkspaces as G
    assert [G.rear_bytes(n) for n in (0, 16, 4096, 4097, 10000, 1 << 20, 5 << 20)] == [4096, 4096, 4096, 8192, 12288, 1 << 20, 1 << 20]


@pytest.mark.parametrize("n,past", [(16, 0), (40, 0), (40, 4095), (8192, 8191), (2 << 20, (1 << 20) - 1)])
def test_a_byte_past_the_payload_fails_with_its_offset(monkeypatch, n, past):
    with guarded_workspaces(monkeypatch) as g:
        ws = g.alloc(n, CPU)
        buf = g.records[0][0]
        buf[4096 + ws.numel() + past] = 0
        with pytest.raises(AssertionError, match=rf"workspace of {n} bytes taken by .*test_a_byte_past.*offset {past} from the end of the payload.*rear guard"):
            g.check()


@pytest.mark.parametrize("n,before", [(16, 1), (4096, 1), (4096, 4096)])
def test_a_byte_before_the_payload_fails_with_a_negative_offset(monkeypatch, n, before):
    with guarded_workspaces(monkeypatch) as g:
        ws = g.alloc(n, CPU)
        buf = g.records[0][0]
        buf[4096 - before] = 0
        with pytest.raises(AssertionError, match=rf"offset -{ws.numel() + before} from the end of the payload.*front guard"):
            g.check()


def test_a_guard_byte_rewritten_with_its_own_value_is_not_a_hit_and_other_values_are(monkeypatch):
    """the check is bytewise: the poison's own bytes (A5 A5 C5 7F, little endian) in place pass, any other value at any byte fails"""
    with guarded_workspaces(monkeypatch) as g:
        ws = g.alloc(64, CPU)
        buf = g.records[0][0]
        end = 4096 + ws.numel()
        buf[end:end + 4] = torch.tensor([0xA5, 0xA5, 0xC5, 0x7F], dtype=torch.uint8)
        g.check()
        buf[end + 3] = 0x7E
        with pytest.raises(AssertionError, match="offset 3 from"):
            g.check()


def test_every_workspace_is_checked(monkeypatch):
    with guarded_workspaces(monkeypatch) as g:
        a, b, c = (ops._ws(n, CPU) for n in (100, 200, 300))
        assert g.calls == 3
        g.check()
        g.records[1][0][4096 + 200 + 7] = 1
        with pytest.raises(AssertionError, match="workspace of 200 bytes.*offset 7 "):
            g.check()
