"""Validator.done() with advection on more than one rank, 2 gloo ranks on the CPU: the ONE allocation (main block, the pooled and FSS
tables, then the advection baseline's two appended tables) is summed with ONE all-reduce, and aggregates to what a single process gets
on the union of the two ranks' batches: the rank sums appear under "advection"."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

T, THR, POOLS, FSS = 5, [20, 30, 35, 40], ((4, 4), (16, 8)), (1, 5, 33)
HW, AREA = 48 * 48, 38 * 38
NBASE = len(POOLS) + 1


def _block(rank):
    """what a rank's epoch could have left: test_fss_gloo's block, then the advected field's pooled table and its FSS table"""
    n = len(THR)
    rng = np.random.default_rng(41 + rank)
    main = rng.integers(1, 1 << 30, (T, 4 * n + 3)).astype(np.float64)
    main[:, 4 * n:] += rng.random((T, 3))
    pooled = rng.integers(0, 1 << 30, T * (len(POOLS) + NBASE) * 4 * n).astype(np.float64)
    fss = rng.integers(1, 1 << 40, (3 * T * len(FSS) * n, 3)).astype(np.float64)         # the forecast's, persistence's, the advection's
    fss[:, 2] = np.floor(np.sqrt(fss[:, 0] * fss[:, 1]) * rng.random(len(fss)))
    third = T * len(FSS) * n
    adv_pooled = rng.integers(1, 1 << 30, T * NBASE * 4 * n).astype(np.float64)
    return torch.from_numpy(np.concatenate([[1.5 + rank, 3 + rank, 12 + 4 * rank, rank], main.ravel(), pooled, fss[:2 * third].ravel(), adv_pooled,
                                            fss[2 * third:].ravel()]))


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adnm-unet_amd"))
    from adnm_hip.validate import Validator, advection_doubles, block_doubles, fss_doubles, reduce_block
    from models.loss import enRainfallLoss
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    val = Validator(torch.nn.Identity(), enRainfallLoss(), T, 90.0, THR, process_group=dist.group.WORLD, pools=POOLS, persistence=True, fss=FSS,
                    advection=(16, 4))
    mine = _block(rank)
    assert mine.numel() == (sum(block_doubles(T, len(THR), POOLS, True)) + sum(fss_doubles(T, len(THR), FSS, True))
                            + sum(advection_doubles(T, len(THR), POOLS, FSS, True)))
    val._block, val._frame = mine.clone(), (48, 48)      # the state an epoch of 48 x 48 frames leaves (no GPU here: the block is on the CPU)
    res = val.done(per_lead=True)
    done_calls = len(calls)
    summed = reduce_block(mine.clone(), dist.group.WORLD)
    q.put((rank, dict(res=repr(res), calls=done_calls, reduce_calls=len(calls) - done_calls, untouched=bool(torch.equal(val._block, mine)),
                      summed=summed.numpy().copy())))
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
    n = len(THR)
    union = (_block(0) + _block(1)).numpy()
    want = aggregate(union, THR, T, HW, AREA, pools=POOLS, persistence=True, per_lead=True, fss=FSS, advection=True)
    assert (want["batches"], want["samples"], want["nonfinite"]) == (7, 28, 1)
    adv = want["advection"]
    assert set(adv) == {"threshold_metrics", "FAR", "pooled", "fss"} and set(adv["pooled"]) == set(POOLS) and list(adv["fss"]) == list(FSS)
    assert set(want["per_lead"]["advection"]) == {"threshold_metrics", "pooled", "fss"}
    # the rank SUMS appear under "advection": the appended tables are the last two parts of the block
    n6 = T * len(FSS) * 3 * n
    atab = union[-n6 - T * NBASE * 4 * n:-n6].reshape(T, NBASE, 4 * n)
    ftab = union[-n6:].reshape(T, len(FSS), 3 * n).sum(0)
    for k, thr in enumerate(THR):
        for j, name in enumerate(("TP", "FN", "FP", "TN")):
            assert adv["threshold_metrics"][thr][name] == atab[:, 0, 4 * k + j].sum()
            assert adv["pooled"][(16, 8)]["threshold_metrics"][thr][name] == atab[:, 2, 4 * k + j].sum()
            assert (want["per_lead"]["advection"]["threshold_metrics"][thr][name] == atab[:, 0, 4 * k + j]).all()
    assert adv["fss"][5][30] == 2.0 * ftab[1, 5] / (ftab[1, 3] + ftab[1, 4]) and 0.0 < adv["fss"][5][30] < 1.0
    assert repr(adv) != repr(want["persistence"])
    for r in (0, 1):
        assert res[r]["calls"] == 1, f"rank {r}: {res[r]['calls']} all-reduces in done()"
        assert res[r]["reduce_calls"] == 1 and (res[r]["summed"] == union).all(), "reduce_block: not the elementwise sum, or not one all-reduce"
        assert res[r]["untouched"], "done() reduced the epoch's block in place"
        assert res[r]["res"] == repr(want), f"rank {r}: not the single-process result on the union"
