"""FlatTrainer(ema_decay=...) on more than one rank, on the CPU (fused=False, 2 gloo ranks, monitor=True): three steps, the second
skipped on BOTH ranks because of one rank's poisoned batch.  The average moves with the applied steps only, follows its recurrence
(fp64 statement, the kernel's bound) and holds the same bits on both ranks."""
import os
import queue
import socket
import sys
import time

import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from ema_ref import assert_ema_step, warmup_decay

CONFIGS = [(ov, warm) for ov in (False, True) for warm in (True, False)]
DECAY = 0.9


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


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adnm-unet_amd"))
    from adnm_hip.trainer import FlatTrainer
    out = {}
    for ci, (ov, warm) in enumerate(CONFIGS):
        torch.manual_seed(100 + rank)
        xs = [torch.randn(2, 8) for _ in range(3)]
        ts = [torch.randn(2, 4) for _ in range(3)]
        if rank == 1:
            xs[1][0, 0] = float("inf")   # the second batch of rank 1 alone
        tr = FlatTrainer(Staged3(), _loss, lr=1e-2, eps=1e-9, weight_decay=1e-2, max_norm=0.5, use_graph=False, fused=False, overlap=ov,
                         monitor=True, ema_decay=DECAY, ema_warmup=warm)
        tr.prepare(xs[0], ts[0])   # lays the buffers out: the average is born as a copy of the parameters
        born = torch.equal(tr.ema, tr.flat_p) and tr.ema.data_ptr() != tr.flat_p.data_ptr() and tr.ema_info() == {"decay": 0.0, "updates": 0}
        steps = []
        for x, t in zip(xs, ts):
            before = tr.ema.numpy().copy()   # (numpy: what crosses the process boundary owns its memory)
            tr.step(x, t)
            steps.append(dict(before=before, p=tr.flat_p.numpy().copy(), ema=tr.ema.numpy().copy(), info=tr.ema_info(), stats=tr.stats()))
        sd = tr.state_dict()
        out[ci] = dict(born=born, steps=steps, names=sorted(sd["ema"]), decay=sd["ema_decay"], warm=sd["ema_warmup"], info_sd=sd["ema_info"].tolist())
        tr.close()
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_average_skips_with_the_step_and_is_the_same_on_both_ranks():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res, deadline = {}, time.monotonic() + 180
    try:
        while len(res) < 2:   # (a rank that died is noticed at once, not when the time limit runs out)
            try:
                rank, out = q.get(timeout=1)
                res[rank] = out
            except queue.Empty:
                assert all(p.exitcode in (None, 0) for p in procs), f"a rank died: exit codes {[p.exitcode for p in procs]}"
                assert time.monotonic() < deadline, "the ranks did not finish in 180 s"
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:   # (the partner of a dead rank waits in a collective: nothing is left running)
            if p.is_alive():
                p.terminate()
    for ci, (ov, warm) in enumerate(CONFIGS):
        a, b, what = res[0][ci], res[1][ci], f"overlap={ov} warmup={warm}"
        for r in (a, b):
            for s in r["steps"]:
                s.update({k: torch.from_numpy(s[k]) for k in ("before", "p", "ema")})
            s1, s2, s3 = r["steps"]
            assert r["born"], f"{what}: the average does not start as a copy of the parameters with zero counters"
            assert s2["stats"]["skipped"] == 1 and s3["stats"]["steps"] == 2, (what, s3["stats"])
            assert [s["info"]["updates"] for s in r["steps"]] == [1, 1, 2], what
            # the skipped step: neither the average nor its two floats moved
            assert torch.equal(s2["ema"].view(torch.int32), s1["ema"].view(torch.int32)) and s2["info"] == s1["info"], what
            assert not torch.equal(s3["ema"], s2["ema"]), f"{what}: the step after the skip left the average alone"
            for t, s in ((1, s1), (2, s3)):   # the optimiser step the update belongs to
                want = warmup_decay(DECAY, t) if warm else float(torch.tensor(DECAY, dtype=torch.float32))
                assert abs(s["info"]["decay"] - want) <= 4 * 2.0 ** -24 * want, (what, t, s["info"], want)
            # the recurrence (step 3: the average before it is the one the skipped step left)
            assert_ema_step(s1["ema"], s1["before"], s1["p"], s1["info"]["decay"], f"{what}: step 1")
            assert torch.equal(s3["before"], s2["ema"])
            assert_ema_step(s3["ema"], s3["before"], s3["p"], s3["info"]["decay"], f"{what}: step 3")
            assert r["decay"] == DECAY and r["warm"] is warm and r["info_sd"] == [s3["info"]["decay"], 2.0]
            assert len(r["names"]) == 6
        for x, y in zip(a["steps"], b["steps"]):
            assert torch.equal(x["ema"].view(torch.int32), y["ema"].view(torch.int32)), f"{what}: the averages of the two ranks differ"
            assert torch.equal(x["p"], y["p"]) and x["info"] == y["info"], what
