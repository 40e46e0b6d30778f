"""Validator.done() on more than one rank: its reduction (adnm_hip.validate.reduce_block) on two synthetic CPU blocks, 2 gloo ranks —
both ranks end with the elementwise double sum of the two blocks, after ONE all-reduce."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

T, NTHR = 5, 4
N = 4 + T * (4 * NTHR + 3)


def _block(rank):
    """what a rank's epoch could have left: integer counts beyond fp32's exact range, fractional sums"""
    g = torch.Generator().manual_seed(7 + rank)
    blk = torch.rand(N, dtype=torch.float64, generator=g) * 1e3
    blk[1], blk[2], blk[3] = 11 + rank, 44 + 4 * rank, rank
    tab = blk[4:].view(T, 4 * NTHR + 3)
    tab[:, :4 * NTHR] = torch.randint(0, 1 << 40, (T, 4 * NTHR), generator=g).double() + (1 << 30)
    return blk


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adnm-unet_amd"))
    from adnm_hip import validate
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    mine = _block(rank)
    out = validate.reduce_block(mine.clone(), dist.group.WORLD)
    same = validate.reduce_block(mine.clone(), None)     # no group: untouched
    try:
        validate.reduce_block(mine.float(), dist.group.WORLD)
        refused = False
    except RuntimeError:
        refused = True
    res = validate.aggregate(out.numpy(), [20, 30, 35, 40], T, 48 * 48, 38 * 38)
    q.put((rank, dict(out=out.numpy().copy(), calls=len(calls), untouched=bool(torch.equal(same, mine)), refused=refused, samples=res["samples"],
                      batches=res["batches"], nonfinite=res["nonfinite"], tp=res["threshold_metrics"][20]["TP"])))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_end_with_the_sum_of_their_blocks():
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
    want = (_block(0) + _block(1)).numpy()
    for r in (0, 1):
        assert res[r]["out"].dtype == want.dtype and (res[r]["out"] == want).all(), f"rank {r}: not the double sum of the two blocks"
        assert res[r]["calls"] == 1, f"rank {r}: {res[r]['calls']} all-reduces"
        assert res[r]["untouched"] and res[r]["refused"]
        assert (res[r]["batches"], res[r]["samples"], res[r]["nonfinite"]) == (23, 92, 1)
        assert res[r]["tp"] == want[4:].reshape(T, -1)[:, 0].sum()
    assert (res[0]["out"] == res[1]["out"]).all()
