"""Validator.done() with tracks on more than one rank, 2 gloo ranks on the CPU: the ONE allocation (main block, the objects table, the tracks
table) is summed with ONE all-reduce, and the reduced block equals, integer for integer, the block a single process gets on the concatenated
batches of the two ranks (tracks never leave their sample, so the union's table is the sum of the tables)."""
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
T, THR, SCALE, H, W, MV = 4, [20.0, 30.0, 35.0, 40.0], 90.0, 24, 28, 2
SAMPLES = (2, 3)   # per rank


def _fields(rank):
    import tracks_ref as R
    return R.discs(SAMPLES[rank], T, H, W, 31 + rank), R.discs(SAMPLES[rank], T, H, W, 41 + rank)


def _block(fields, seed, samples):
    """what an epoch on `fields` could have left: a header, integer counts in the main and objects tables, the yardstick's tracks table"""
    import tracks_ref as R
    n = len(THR)
    rng = np.random.default_rng(seed)
    main = rng.integers(1, 1 << 30, (T, 4 * n + 3)).astype(np.float64)
    objects = rng.integers(1, 1 << 40, T * 2 * n * 23).astype(np.float64)
    tab = R.table(fields[0], fields[1], THR, SCALE, MV).astype(np.float64)
    return torch.from_numpy(np.concatenate([[1.5, 1, samples, 0], main.ravel(), objects, tab.ravel()])), tab


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path[:0] = [os.path.join(os.path.dirname(HERE), "adnm-unet_amd"), HERE]
    from adnm_hip.validate import Validator, block_doubles, objects_doubles, reduce_block, tracks_doubles
    from models.loss import enRainfallLoss
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    val = Validator(torch.nn.Identity(), enRainfallLoss(), T, SCALE, THR, process_group=dist.group.WORLD, objects=True, tracks=MV)
    mine, _ = _block(_fields(rank), 23 + rank, SAMPLES[rank])
    assert mine.numel() == block_doubles(T, len(THR))[0] + objects_doubles(T, len(THR), True) + tracks_doubles(T, len(THR), MV)
    val._block, val._frame = mine.clone(), (H, W)      # the state an epoch leaves (no GPU here: the block is on the CPU)
    res = val.done(per_lead=True)
    n_calls = len(calls)
    reduced = reduce_block(mine.clone(), dist.group.WORLD)
    q.put((rank, dict(res=repr(res), calls=n_calls, untouched=bool(torch.equal(val._block, mine)), reduced=reduced.numpy().tobytes())))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_reduce_to_the_block_of_the_concatenated_batches():
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "adnm-unet_amd"))
    from adnm_hip.validate import aggregate, track_entries, tracks_doubles
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
    size = tracks_doubles(T, len(THR), MV)
    assert size == tab.size == 2 * len(THR) * (7 + 4 * T)
    assert (union[-size:].view(np.int64) == tab.ravel().view(np.int64)).all(), "the sum of the ranks' tables is not the table of the concatenated batches"
    assert tab[:, 0, 0].min() > 0 and (tab[0] != tab[1]).any(), "an empty table: nothing is compared"
    want = aggregate(union, THR, T, H * W, (H - 10) * (W - 10), per_lead=True, objects=True, tracks=MV)
    assert (want["batches"], want["samples"]) == (2, 5) and "tracks" in want and "tracks" not in want["per_lead"]
    assert repr(want["tracks"]) == repr(track_entries(tab, 5, THR, T, MV)) and want["tracks"][20]["target"]["count"] == int(tab[0, 0, 0])
    for r in (0, 1):
        assert res[r]["calls"] == 1, f"rank {r}: {res[r]['calls']} all-reduces"
        assert res[r]["untouched"], "done() reduced the epoch's block in place"
        assert res[r]["reduced"] == union.tobytes(), f"rank {r}: the reduced block is not the union's, bit for bit"
        assert res[r]["res"] == repr(want), f"rank {r}: not the single-process result on the union"
