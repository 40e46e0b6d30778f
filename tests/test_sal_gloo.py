"""Validator.done() with sal= on more than one rank, 2 gloo ranks on the CPU: the SAL table is the last part of the ONE allocation, which is
summed with ONE all-reduce, and aggregates to what a single process gets on the union of the two ranks' batches (every column is a sum over
frames, counts and scores alike, so the union's block is the sum of the blocks and a mean is the summed score over the summed count)."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

T, THR, FSS, FRAME, SPEC = 4, [20, 30, 35, 40], (1, 5), (16, 64), dict(min_area=3, intensity=list(range(90)) + [400])
HW, AREA = 16 * 64, 6 * 54


def _rows(rng, frames):
    """a consistent (T, nthr, 12) table of `frames` frames per row: A on every frame, L1 on most, S on fewer with the threshold"""
    tab = np.zeros((T, len(THR), 12), dtype=np.float64)
    for t in range(T):
        a, l1 = rng.uniform(-2, 2, frames), rng.uniform(0, 1, frames)
        has_l1 = rng.random(frames) < 0.9
        for k in range(len(THR)):
            has_s = has_l1 & (rng.random(frames) < 0.8 / (k + 1))
            s, l2 = rng.uniform(-2, 2, frames), rng.uniform(0, 1, frames)
            missed = ~has_s & (rng.random(frames) < 0.3)
            false = ~has_s & ~missed & (rng.random(frames) < 0.3)
            tab[t, k] = (frames, a.sum(), np.abs(a).sum(), has_l1.sum(), l1[has_l1].sum(), has_s.sum(), s[has_s].sum(), np.abs(s[has_s]).sum(), l2[has_s].sum(),
                         (l1 + l2)[has_s].sum(), missed.sum(), false.sum())
    return tab


def _block(rank):
    """what a rank's half epoch could have left: a header, a main table, integer FSS sums and a SAL table"""
    n = len(THR)
    rng = np.random.default_rng(81 + rank)
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
    from adnm_hip.validate import Validator, block_doubles, fss_doubles, reduce_block, sal_doubles
    from models.loss import enRainfallLoss
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    val = Validator(torch.nn.Identity(), enRainfallLoss(), T, 90.0, THR, process_group=dist.group.WORLD, fss=FSS, sal=SPEC)
    mine = _block(rank)
    assert mine.numel() == block_doubles(T, len(THR))[0] + sum(fss_doubles(T, len(THR), FSS)) + sal_doubles(T, len(THR), SPEC)
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
    from adnm_hip.validate import aggregate, sal_entries
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
    want = aggregate(union, THR, T, HW, AREA, per_lead=True, fss=FSS, sal=SPEC)
    assert (want["batches"], want["samples"], want["nonfinite"]) == (7, 28, 1)
    # the union's entries are those of the summed table, not a mean of the ranks' entries
    n = T * len(THR) * 12
    tab = union[-n:].reshape(T, len(THR), 12)
    spec = (3, tuple(SPEC["intensity"]))
    assert _same_tree(want["sal"], sal_entries(tab.sum(0), THR, spec)) and _same_tree(want["per_lead"]["sal"], sal_entries(tab, THR, spec))
    o = want["sal"]
    assert o["min_area"] == 3 and o["intensity"] == spec[1] and o[20]["frames_A"] == 28 * T and o[20]["A"] == tab[:, 0, 1].sum() / (28 * T)
    assert 0 < o[40]["frames_S"] < o[20]["frames_S"] <= o[20]["frames_L1"] < o[20]["frames_A"], "_rows defines S on fewer frames as the threshold rises"
    assert o[20]["abs_S"] >= abs(o[20]["S"]) and o[20]["L"] > o[20]["L2"] > 0
    halves = [sal_entries(_block(r).numpy()[-n:].reshape(T, len(THR), 12).sum(0), THR, spec)[20]["S"] for r in (0, 1)]
    assert o[20]["S"] != 0.5 * (halves[0] + halves[1]), "the ranks have other frame counts: the union's mean is not the mean of their means"
    for r in (0, 1):
        assert res[r]["calls"] == 1, f"rank {r}: {res[r]['calls']} all-reduces in done()"
        assert res[r]["untouched"], "done() reduced the epoch's block in place"
        assert (res[r]["summed"].view(np.int64) == union.view(np.int64)).all(), f"rank {r}: reduce_block is not the sum of the blocks"
        assert _same_tree(res[r]["res"], want), f"rank {r}: not the single-process result on the union"
