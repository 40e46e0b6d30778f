"""Validator.done() with joint=True on more than one rank, 2 gloo ranks on the CPU: the joint histogram is the last part of the ONE
allocation, which is summed with ONE all-reduce, and aggregates to what a single process gets on the union of the two ranks' batches
(counts add, so the union's block is the sum of the blocks)."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

T, THR, FSS, FRAME, SCALE = 4, [20, 30, 35, 40], (1, 5), (16, 64), 90.0
HW, AREA, R, L = 16 * 64, 6 * 54, 32, 91


def _block(rank):
    """what a rank's half epoch could have left: a header, integer counts, fractional sums, integer FSS sums, a spectrum table, and a joint
    histogram near the diagonal whose forecast runs low, with the main table's counts taken from it"""
    from adnm_hip.validate import joint_counts_at
    n = len(THR)
    rng = np.random.default_rng(61 + rank)
    samples = 12 + 4 * rank
    o = np.minimum((rng.exponential(9.0, (T, samples * HW)) * (rng.random((T, samples * HW)) < 0.2)).astype(np.int64), L - 1)
    f = np.clip(np.rint(o * 0.8 + rng.normal(0, 2.0, o.shape) * (o > 0)), 0, L - 1).astype(np.int64)
    joint = np.stack([np.bincount(o[t] * L + f[t], minlength=L * L).reshape(L, L) for t in range(T)]).astype(np.float64)
    main = rng.integers(1, 1 << 30, (T, 4 * n + 3)).astype(np.float64)
    main[:, 4 * n:] += rng.random((T, 3))
    for k, thr in enumerate(THR):
        main[:, 4 * k:4 * k + 4] = np.stack(joint_counts_at(joint, thr), axis=1)
    fss = rng.integers(1, 1 << 40, (T * len(FSS) * n, 3)).astype(np.float64)
    fss[:, 2] = np.floor(np.sqrt(fss[:, 0] * fss[:, 1]) * rng.random(len(fss)))
    spec = rng.random((T, R, 3)) * 1e4 + 1.0
    spec[..., 2] = np.sqrt(spec[..., 0] * spec[..., 1]) * (2 * rng.random((T, R)) - 1)
    return torch.from_numpy(np.concatenate([[1.5 + rank, 3 + rank, samples, rank], main.ravel(), fss.ravel(), spec.ravel(), joint.ravel()]))


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adnm-unet_amd"))
    from adnm_hip.validate import Validator, block_doubles, fss_doubles, joint_doubles, reduce_block, spectrum_doubles
    from models.loss import enRainfallLoss
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    val = Validator(torch.nn.Identity(), enRainfallLoss(), T, SCALE, THR, process_group=dist.group.WORLD, fss=FSS, spectrum=True, joint=True)
    mine = _block(rank)
    assert mine.numel() == block_doubles(T, len(THR))[0] + sum(fss_doubles(T, len(THR), FSS)) + spectrum_doubles(T, FRAME) + joint_doubles(T, SCALE)
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
    from adnm_hip.validate import aggregate, joint_entries
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
    want = aggregate(union, THR, T, HW, AREA, per_lead=True, fss=FSS, spectrum=FRAME, joint=L)
    assert (want["batches"], want["samples"], want["nonfinite"]) == (7, 28, 1)
    # the union's entries are those of the summed counts, not a mean of the ranks' entries
    tab = union[-T * L * L:].reshape(T, L, L)
    assert _same_tree(want["joint"], joint_entries(tab.sum(0))) and _same_tree(want["per_lead"]["joint"], joint_entries(tab))
    j = want["joint"]
    assert int(j["histogram"].sum()) == 28 * HW * T and (want["per_lead"]["joint"]["histogram"].sum(axis=(1, 2)) == 28 * HW).all()
    assert j["curves"]["bias"][35] < j["curves"]["bias"][5] < 1.0 and j["mean_error"] < 0 and 0.5 < j["correlation"] < 1.0, "the forecast of _block runs low"
    for thr in THR:
        assert all(want["threshold_metrics"][thr][k] == j["curves"][k][thr] for k in ("TP", "FN", "FP", "TN"))
    for r in (0, 1):
        assert res[r]["calls"] == 1, f"rank {r}: {res[r]['calls']} all-reduces in done()"
        assert res[r]["untouched"], "done() reduced the epoch's block in place"
        assert (res[r]["summed"].view(np.int64) == union.view(np.int64)).all(), f"rank {r}: reduce_block is not the sum of the blocks"
        assert _same_tree(res[r]["res"], want), f"rank {r}: not the single-process result on the union"
