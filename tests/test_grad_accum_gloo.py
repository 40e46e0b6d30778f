"""Gradient accumulation on more than one rank, on the CPU: 2 gloo ranks x accum_steps=2 x micro-batch 2 must train like one process on
the concatenated batch of 8, with ONE all-reduce per non-empty bucket per optimiser step and none on the micro-steps before it —
in the plain and the staged (overlap) form, on the fp32 and the bf16 wire."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

CONFIGS = [(rd, ov) for rd in ("f32", "bf16") for ov in (False, True)]
K, MICRO, STEPS = 2, 2, 3


class Staged3(nn.Module):
    """three stages through forward_stages() (the form ADNM-UNet offers); `skip` crosses a cut unchanged and is used again in the last
    stage, as the U-Net's skip tensors are; `dead` never receives a gradient"""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.a, self.m, self.b = nn.Linear(8, 16), nn.Linear(16, 16), nn.Linear(16, 4)
        self.dead = nn.Linear(16, 16)
        self.s = nn.Parameter(torch.tensor(1.0))

    def forward(self, x):
        a = (x,)
        for fn, _ in self.forward_stages():
            a = fn(*a)
        return a[0]

    def forward_stages(self):
        s0 = lambda x: (torch.tanh(self.a(x)),)
        s1 = lambda h: (torch.tanh(self.m(h)) + h, h)
        s2 = lambda h, skip: (self.b(h + 0.5 * skip) * self.s,)
        return [(s0, [self.a]), (s1, [self.m]), (s2, [self.b, _Holder(self.s)])]


class _Holder(nn.Module):
    def __init__(self, p):
        super().__init__()
        self.p = p


def _loss(o, t):
    return (o - t).pow(2).mean()


def _trainer(model, **kw):
    from adnm_hip.trainer import FlatTrainer
    return FlatTrainer(model, _loss, lr=1e-2, eps=1e-9, weight_decay=1e-2, max_norm=0.5, use_graph=False, fused=False, **kw)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adnm-unet_amd"))
    calls = [0]
    real = dist.all_reduce

    def counted(*a, **kw):
        calls[0] += 1
        return real(*a, **kw)
    dist.all_reduce = counted
    out = {}
    for ci, (rd, ov) in enumerate(CONFIGS):
        model = Staged3()
        tr = _trainer(model, reduce_dtype=rd, overlap=ov, accum_steps=K)
        torch.manual_seed(100 + rank)
        xs = [torch.randn(MICRO, 8) for _ in range(STEPS * K)]
        ts = [torch.randn(MICRO, 4) for _ in range(STEPS * K)]
        counts = []
        for x, t in zip(xs, ts):
            calls[0] = 0
            tr.step(x, t)
            counts.append(calls[0])
        assert tr.staged == ov and len(tr.buckets) == (3 if ov else 1) and tr._steps == STEPS and tr.micro_step == 0
        out[ci] = {"final": [p.detach().numpy().copy() for p in model.parameters()], "g": tr.flat_g.numpy().copy(),
                   "xs": [x.numpy().copy() for x in xs], "ts": [t.numpy().copy() for t in ts], "counts": counts,
                   "nonempty": sum(hi > lo for lo, hi in tr.buckets)}
        tr.close()
    dist.all_reduce = real
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_with_accumulation_equal_the_global_batch():
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
        # one all-reduce per non-empty bucket on the LAST micro-step of a cycle — what accum_steps=1 issues per step — and none before it
        want = [0] * (K - 1) + [a["nonempty"]]
        assert a["nonempty"] == (3 if ov else 1), what
        assert a["counts"] == want * STEPS and b["counts"] == want * STEPS, (what, a["counts"], b["counts"])
        for pa, pb in zip(a["final"], b["final"]):
            assert (pa == pb).all(), f"{what}: replicas diverged"
        assert (a["g"] == b["g"]).all(), f"{what}: averaged gradients differ between the ranks"
        if rd != "f32":
            continue
        # single process, no accumulation, on the concatenated batch of world x K x MICRO = 8
        model = Staged3()
        tr = _trainer(model, overlap=ov)
        for i in range(STEPS):
            x = torch.cat([torch.from_numpy(r["xs"][i * K + j]) for r in (a, b) for j in range(K)])
            t = torch.cat([torch.from_numpy(r["ts"][i * K + j]) for r in (a, b) for j in range(K)])
            assert x.shape[0] == 8
            tr.step(x, t)
        for pa, p in zip(a["final"], model.parameters()):
            assert torch.allclose(torch.from_numpy(pa), p.detach(), atol=2e-6, rtol=1e-5), what
        tr.close()
