"""FlatTrainer(monitor=True) on more than one rank, on the CPU (fused=False, 2 gloo ranks): a batch that poisons the gradient of ONE rank
makes BOTH ranks skip the step — the decision is taken after the all-reduce, on gradients that are the same bits everywhere, so no
flag is exchanged — and the run goes on as if the batch had never been seen.  fp32 and bf16 wire, plain and staged (overlap) form."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

CONFIGS = [(rd, ov) for rd in ("f32", "bf16") for ov in (False, True)]


class Staged3(nn.Module):
    """three stages through forward_stages(), a skip tensor across a cut (the shape ADNM-UNet offers)"""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.a, self.m, self.b = nn.Linear(8, 16), nn.Linear(16, 16), nn.Linear(16, 4)

    def forward(self, x):
        a = (x,)
        for fn, _ in self.forward_stages():
            a = fn(*a)
        return a[0]

    def forward_stages(self):
        s0 = lambda x: (torch.tanh(self.a(x)),)
        s1 = lambda h: (torch.tanh(self.m(h)) + h, h)
        s2 = lambda h, skip: (self.b(h + 0.5 * skip),)
        return [(s0, [self.a]), (s1, [self.m]), (s2, [self.b])]


def _loss(o, t):
    return (o - t).pow(2).mean()


def _trainer(model, **kw):
    from adnm_hip.trainer import FlatTrainer
    return FlatTrainer(model, _loss, lr=1e-2, eps=1e-9, weight_decay=1e-2, max_norm=0.5, use_graph=False, fused=False, **kw)


def _state(tr):
    return [t.numpy().copy() for t in (tr.flat_p, tr.exp_avg, tr.exp_avg_sq)]


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adnm-unet_amd"))
    out = {}
    for ci, (rd, ov) in enumerate(CONFIGS):
        torch.manual_seed(100 + rank)
        xs = [torch.randn(2, 8) for _ in range(3)]
        ts = [torch.randn(2, 4) for _ in range(3)]
        if rank == 1:
            xs[1][0, 0] = float("inf")   # the second batch of rank 1 alone: its gradient of a.weight holds 0 * inf = NaN
        tr = _trainer(Staged3(), reduce_dtype=rd, overlap=ov, monitor=True)
        tr.step(xs[0], ts[0])
        before = _state(tr)
        tr.step(xs[1], ts[1])
        skipped = _state(tr)
        st = tr.stats()
        steps_host = tr._steps
        g_finite = bool(torch.isfinite(tr.flat_g).all())
        tr.step(xs[2], ts[2])
        after = _state(tr)
        st_end = tr.stats()
        tr.close()
        # the same two ranks on the first and the third batch only, without the monitor
        twin = _trainer(Staged3(), reduce_dtype=rd, overlap=ov)
        twin.step(xs[0], ts[0])
        twin.step(xs[2], ts[2])
        clean = _state(twin)
        twin.close()
        out[ci] = dict(before=before, skipped=skipped, after=after, clean=clean, stats=st, stats_end=st_end, steps_host=steps_host,
                       g_finite=g_finite)
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_one_poisoned_rank_makes_both_ranks_skip():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for ci, (rd, ov) in enumerate(CONFIGS):
        a, b, what = res[0][ci], res[1][ci], f"reduce_dtype={rd} overlap={ov}"
        for r in (a, b):
            assert not r["g_finite"], f"{what}: the poisoned batch left the averaged gradient finite: the test checks nothing"
            assert r["stats"]["skipped"] == 1 and r["stats"]["steps"] == 1, (what, r["stats"])
            assert r["steps_host"] == 1, f"{what}: the host's step counter (bias correction of the torch path) advanced on a skipped step"
            assert r["stats_end"]["skipped"] == 1 and r["stats_end"]["steps"] == 2, (what, r["stats_end"])
            for x, y in zip(r["before"], r["skipped"]):
                assert (x == y).all(), f"{what}: the skipped step moved parameters or moments"
            for x, y in zip(r["after"], r["clean"]):
                assert (x == y).all(), f"{what}: the step after the skip differs from a run that never saw the poisoned batch"
        # the loss statistic is each rank's own: rank 1's poisoned batch may or may not have a finite loss, rank 0's three are finite
        assert a["stats_end"]["loss_nonfinite"] == 0
        for key in ("skipped", "after"):
            for x, y in zip(a[key], b[key]):
                assert (x == y).all(), f"{what}: replicas diverged ({key})"
