"""GraphedForward's client protocol (adnm_hip.evaluator.ForwardClient) on torch-only toy models: which method runs when, inside or outside
the capture, what a second call and a second shape do, and that a first call refused at any stage leaves nothing behind."""
import pytest
import torch

from adnm_hip.evaluator import ForwardClient, GraphedForward

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE, OTHER = (2, 5, 1, 16, 12), (1, 5, 1, 16, 12)


class Counting(torch.nn.Module):
    """the identity as a fresh tensor (a graph's static output must not alias its static input), counting its calls"""

    def __init__(self):
        super().__init__()
        self.calls = 0

    def forward(self, x):
        self.calls += 1
        return x * 1.0


class Recording(ForwardClient):
    def __init__(self, fail_at=None):
        self.record, self.ents, self.fail_at = [], [], fail_at

    def _note(self, method, ent):
        self.record.append((method, torch.cuda.is_current_stream_capturing()))
        if not any(e is ent for e in self.ents):
            self.ents.append(ent)
        if method == self.fail_at:   # on its first use only
            self.fail_at = None
            raise ValueError(f"refused in {method}")

    def open(self, ent, x):
        self._note("open", ent)

    def model_input(self, ent, sx):
        self._note("model_input", ent)
        return sx

    def check(self, ent, out):
        self._note("check", ent)

    def after(self, ent, sx, out):
        self._note("after", ent)


FIRST_CALL = [("open", False), ("model_input", False), ("model_input", False), ("check", False), ("model_input", True), ("after", True)]


def test_client_protocol():
    model, client = Counting().to(DEV), Recording()
    fwd = GraphedForward(model, client=client)
    x, y = torch.rand(SHAPE, device=DEV), torch.rand(SHAPE, device=DEV)
    out = fwd(x)
    assert torch.equal(out, x) and model.calls == 3
    assert client.record == FIRST_CALL and len(client.ents) == 1
    # the same shape again: a replay and nothing else
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    out = fwd(y)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before, "a replay allocated"
    assert torch.equal(out, y) and model.calls == 3 and client.record == FIRST_CALL
    # a second shape: the same sequence on an entry of its own
    z = torch.rand(OTHER, device=DEV)
    assert torch.equal(fwd(z), z) and model.calls == 6
    assert client.record == FIRST_CALL + FIRST_CALL and len(client.ents) == 2 and len(fwd._graphs) == 2
    assert fwd.entry(x) is client.ents[0] and fwd.entry(z) is client.ents[1]
    fwd.close()
    fwd.close()
    assert len(fwd._graphs) == 0
    assert torch.equal(fwd(x), x) and model.calls == 9 and client.record == FIRST_CALL * 3 and len(client.ents) == 3
    fwd.close()


@pytest.mark.parametrize("stage", ["open", "check", "after"])
def test_failed_first_call_leaves_no_entry(stage):
    model, client = Counting().to(DEV).train(), Recording(fail_at=stage)
    fwd = GraphedForward(model, client=client)
    x = torch.rand(SHAPE, device=DEV)
    with pytest.raises(ValueError, match=f"refused in {stage}"):
        fwd(x)
    assert not torch.cuda.is_current_stream_capturing()
    assert model.training
    assert len(fwd._graphs) == 0
    assert model.calls == {"open": 0, "check": 2, "after": 3}[stage]
    out = fwd(x)
    torch.cuda.synchronize()
    assert torch.equal(out, x) and model.training and len(fwd._graphs) == 1
    assert client.record[-6:] == FIRST_CALL
    fwd.close()
