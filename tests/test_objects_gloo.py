"""Validator.done() with objects= on more than one rank, 2 gloo ranks on the CPU: the objects table is the last part of the ONE allocation,
which is summed with ONE all-reduce, and aggregates to what a single process gets on the union of the two ranks' batches (every column is
a sum over samples, so the union's block is the sum of the blocks)."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

T, THR, FSS, FRAME, MIN_AREA = 4, [20, 30, 35, 40], (1, 5), (16, 64), 3
HW, AREA = 16 * 64, 6 * 54


def _rows(rng, frames):
    """a consistent (T, 2, nthr, 23) table of `frames` frames per row: objects drawn per field, their areas binned, some of them matched"""
    tab = np.zeros((T, 2, len(THR), 23), dtype=np.float64)
    for t in range(T):
        for f in range(2):
            for k in range(len(THR)):
                n = int(rng.integers(0, 6 * frames // (k + 1)))
                areas = np.maximum((rng.exponential(30.0 / (k + 1), n)).astype(np.int64), MIN_AREA)
                hit = rng.random(n) < (0.7 if f == 0 else 0.5)
                tab[t, f, k, :6] = (n, areas.sum(), (areas * areas).sum(), min(int(areas.max(initial=0)) * frames // 2, int(areas.sum())), hit.sum(), areas[hit].sum())
                tab[t, f, k, 6:] = np.bincount(np.frexp(areas.astype(np.float64))[1] - 1, minlength=17)
    return tab


def _block(rank):
    """what a rank's half epoch could have left: a header, a main table, integer FSS sums and an objects table"""
    n = len(THR)
    rng = np.random.default_rng(71 + rank)
    samples = 12 + 4 * rank
    main = rng.integers(1, 1 << 30, (T, 4 * n + 3)).astype(np.float64)
    main[:, 4 * n:] += rng.random((T, 3))
    fss = rng.integers(1, 1 << 40, (T * len(FSS) * n, 3)).astype(np.float64)
    fss[:, 2] = np.floor(np.sqrt(fss[:, 0] * fss[:, 1]) * rng.random(len(fss)))
    return torch.from_numpy(np.concatenate([[1.5 + rank, 3 + rank, samples, rank], main.ravel(), fss.ravel(), _rows(rng, samples).ravel()]))


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adnm-unet_amd"))
    from adnm_hip.validate import Validator, block_doubles, fss_doubles, objects_doubles, reduce_block
    from models.loss import enRainfallLoss
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    val = Validator(torch.nn.Identity(), enRainfallLoss(), T, 90.0, THR, process_group=dist.group.WORLD, fss=FSS, objects=MIN_AREA)
    mine = _block(rank)
    assert mine.numel() == block_doubles(T, len(THR))[0] + sum(fss_doubles(T, len(THR), FSS)) + objects_doubles(T, len(THR), MIN_AREA)
    val._block, val._frame = mine.clone(), FRAME      # the state a half epoch of 16 x 64 frames leaves (no GPU here: the block is on the CPU)
    res = val.done(per_lead=True)
    in_done = len(calls)
    summed = reduce_block(mine.clone(), dist.group.WORLD)
    q.put((rank, dict(res=res, calls=in_done, untouched=bool(torch.equal(val._block, mine)), summed=summed.numpy())))
    dist.barrier()
    dist.destroy_process_group()


def _same_tree(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same_tree(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is b
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return bool(((a == b) | ((a != a) & (b != b))).all())


def test_two_ranks_aggregate_to_the_union_with_one_all_reduce():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adnm-unet_amd"))
    from adnm_hip.validate import aggregate, object_entries
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
    want = aggregate(union, THR, T, HW, AREA, per_lead=True, fss=FSS, objects=MIN_AREA)
    assert (want["batches"], want["samples"], want["nonfinite"]) == (7, 28, 1)
    # the union's entries are those of the summed table, not a mean of the ranks' entries
    n = T * 2 * len(THR) * 23
    tab = union[-n:].reshape(T, 2, len(THR), 23)
    assert _same_tree(want["objects"], object_entries(tab.sum(0), 28 * T, THR, MIN_AREA)) and _same_tree(want["per_lead"]["objects"], object_entries(tab, 28, THR, MIN_AREA))
    o = want["objects"]
    assert o["min_area"] == MIN_AREA and o[20]["target"]["count"] == int(tab[:, 0, 0, 0].sum()) > 0
    assert o[20]["target"]["per_frame"] == tab[:, 0, 0, 0].sum() / (28 * T)
    assert 0.5 < o[20]["object_POD"] < 0.9 and 0.3 < o[20]["object_FAR"] < 0.7, "_rows matches about 70 % of the observed and 50 % of the forecast objects"
    assert int(o[20]["target"]["size_histogram"].sum()) == o[20]["target"]["count"]
    for r in (0, 1):
        assert res[r]["calls"] == 1, f"rank {r}: {res[r]['calls']} all-reduces in done()"
        assert res[r]["untouched"], "done() reduced the epoch's block in place"
        assert (res[r]["summed"].view(np.int64) == union.view(np.int64)).all(), f"rank {r}: reduce_block is not the sum of the blocks"
        assert _same_tree(res[r]["res"], want), f"rank {r}: not the single-process result on the union"
