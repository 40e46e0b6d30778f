"""Validator.done() with nprob on more than one rank, 2 gloo ranks on the CPU: the ONE allocation (main block, the FSS table, the
neighbourhood probability's histogram) is summed with ONE all-reduce, and the reduced block equals, integer for integer, the block a single
process gets on the concatenated batches of the two ranks (counts add, so the union's table is the sum of the tables)."""
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
T, THR, FSS, NPROB, SCALE, H, W = 3, [20.0, 30.0, 35.0, 40.0], (1, 5), (1, 5, 17), 90.0, 24, 28
SAMPLES = (2, 3)   # per rank


def _fields(rank):
    import nprob_ref as N
    return N.sparse_fields(SAMPLES[rank] * T, H, W, 31 + rank)


def _block(fields, seed, samples):
    """what an epoch on `fields` could have left: a header, integer counts in the main and FSS tables, the yardstick's histogram"""
    import nprob_ref as N
    n = len(THR)
    rng = np.random.default_rng(seed)
    main = rng.integers(1, 1 << 30, (T, 4 * n + 3)).astype(np.float64)
    fss = rng.integers(1, 1 << 40, T * len(FSS) * 3 * n).astype(np.float64)
    tab = N.table(fields[0], fields[1], THR, SCALE, NPROB, T).astype(np.float64)
    return torch.from_numpy(np.concatenate([[1.5, 1, samples, 0], main.ravel(), fss, tab.ravel()])), tab


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path[:0] = [os.path.join(os.path.dirname(HERE), "adnm-unet_amd"), HERE]
    from adnm_hip.validate import Validator, block_doubles, fss_doubles, nprob_doubles, reduce_block
    from models.loss import enRainfallLoss
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    val = Validator(torch.nn.Identity(), enRainfallLoss(), T, SCALE, THR, process_group=dist.group.WORLD, fss=FSS, nprob=NPROB)
    mine, _ = _block(_fields(rank), 23 + rank, SAMPLES[rank])
    assert mine.numel() == block_doubles(T, len(THR))[0] + fss_doubles(T, len(THR), FSS)[0] + nprob_doubles(T, len(THR), NPROB)
    val._block, val._frame = mine.clone(), (H, W)      # the state an epoch leaves (no GPU here: the block is on the CPU)
    res = val.done(per_lead=True)
    n_calls = len(calls)
    reduced = reduce_block(mine.clone(), dist.group.WORLD)
    q.put((rank, dict(res=repr(res), calls=n_calls, untouched=bool(torch.equal(val._block, mine)), reduced=reduced.numpy().tobytes())))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_reduce_to_the_block_of_the_concatenated_batches():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "adnm-unet_amd"))
    from adnm_hip.validate import aggregate, nprob_doubles
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
    blocks = [_block(_fields(r), 23 + r, SAMPLES[r]) for r in range(2)]
    union = (blocks[0][0] + blocks[1][0]).numpy()
    # the single-rank table of the two ranks' batches, one behind the other
    both = tuple(np.concatenate([_fields(0)[i], _fields(1)[i]]) for i in range(2))
    _, tab = _block(both, 0, sum(SAMPLES))
    size = nprob_doubles(T, len(THR), NPROB)
    assert size == tab.size == T * len(THR) * (4 + 52 + 580)
    assert (union[-size:].view(np.int64) == tab.ravel().view(np.int64)).all(), "the sum of the ranks' tables is not the table of the concatenated batches"
    assert tab.sum() == sum(SAMPLES) * T * H * W * len(THR) * len(NPROB) and (tab[:, :, 5:] > 0).any(), "an empty table: nothing is compared"
    want = aggregate(union, THR, T, H * W, (H - 10) * (W - 10), per_lead=True, fss=FSS, nprob=NPROB)
    assert (want["batches"], want["samples"]) == (2, 5) and list(want["nprob"]) == list(NPROB) == list(want["per_lead"]["nprob"])
    assert want["nprob"][5][20]["histogram"].sum() == sum(SAMPLES) * T * H * W
    for r in (0, 1):
        assert res[r]["calls"] == 1, f"rank {r}: {res[r]['calls']} all-reduces"
        assert res[r]["untouched"], "done() reduced the epoch's block in place"
        assert res[r]["reduced"] == union.tobytes(), f"rank {r}: the reduced block is not the union's, bit for bit"
        assert res[r]["res"] == repr(want), f"rank {r}: not the single-process result on the union"
