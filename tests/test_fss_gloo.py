"""Validator.done() with pools, persistence and fss on more than one rank, 2 gloo ranks on the CPU: the ONE allocation (main block, the two
pooled tables, the two FSS tables) is summed with ONE all-reduce, and aggregates to what a single process gets on the union of the two
ranks' batches (counts and sums add, so the union's block is the sum of the blocks)."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

T, THR, POOLS, FSS = 5, [20, 30, 35, 40], ((4, 4), (16, 8)), (1, 5, 33)
HW, AREA = 48 * 48, 38 * 38


def _block(rank):
    """what a rank's epoch could have left: integer counts, fractional sums, a header, integer FSS sums with C <= sqrt(A F)"""
    n = len(THR)
    rng = np.random.default_rng(23 + rank)
    main = rng.integers(1, 1 << 30, (T, 4 * n + 3)).astype(np.float64)
    main[:, 4 * n:] += rng.random((T, 3))
    pooled = rng.integers(0, 1 << 30, T * (len(POOLS) + len(POOLS) + 1) * 4 * n).astype(np.float64)
    fss = rng.integers(1, 1 << 40, (2 * T * len(FSS) * n, 3)).astype(np.float64)
    fss[:, 2] = np.floor(np.sqrt(fss[:, 0] * fss[:, 1]) * rng.random(len(fss)))
    return torch.from_numpy(np.concatenate([[1.5 + rank, 3 + rank, 12 + 4 * rank, rank], main.ravel(), pooled, fss.ravel()]))


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adnm-unet_amd"))
    from adnm_hip.validate import Validator, block_doubles, fss_doubles
    from models.loss import enRainfallLoss
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    val = Validator(torch.nn.Identity(), enRainfallLoss(), T, 90.0, THR, process_group=dist.group.WORLD, pools=POOLS, persistence=True, fss=FSS)
    mine = _block(rank)
    assert mine.numel() == sum(block_doubles(T, len(THR), POOLS, True)) + sum(fss_doubles(T, len(THR), FSS, True))
    val._block, val._frame = mine.clone(), (48, 48)      # the state an epoch of 48 x 48 frames leaves (no GPU here: the block is on the CPU)
    res = val.done(per_lead=True)
    q.put((rank, dict(res=repr(res), calls=len(calls), untouched=bool(torch.equal(val._block, mine)))))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_aggregate_to_the_union_with_one_all_reduce():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adnm-unet_amd"))
    from adnm_hip.validate import aggregate
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
    union = (_block(0) + _block(1)).numpy()
    want = aggregate(union, THR, T, HW, AREA, pools=POOLS, persistence=True, per_lead=True, fss=FSS)
    assert (want["batches"], want["samples"], want["nonfinite"]) == (7, 28, 1) and set(want["pooled"]) == set(POOLS)
    assert list(want["fss"]) == list(FSS) == list(want["persistence"]["fss"]) == list(want["per_lead"]["fss"]) == list(want["per_lead"]["persistence"]["fss"])
    # the union's score is the score of the summed sums, not a mean of the ranks' scores
    tab = union[-2 * T * len(FSS) * 3 * len(THR):-T * len(FSS) * 3 * len(THR)].reshape(T, len(FSS), 3 * len(THR)).sum(0)
    assert want["fss"][5][30] == 2.0 * tab[1, 5] / (tab[1, 3] + tab[1, 4]) and 0.0 < want["fss"][5][30] < 1.0
    for r in (0, 1):
        assert res[r]["calls"] == 1, f"rank {r}: {res[r]['calls']} all-reduces"
        assert res[r]["untouched"], "done() reduced the epoch's block in place"
        assert res[r]["res"] == repr(want), f"rank {r}: not the single-process result on the union"
