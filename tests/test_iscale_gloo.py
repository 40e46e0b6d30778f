"""Validator.done() with intensity_scale=True on more than one rank, 2 gloo ranks on the CPU: the ONE allocation (main block, the baseline's
pooled table, the forecast's and the baseline's intensity-scale tables) is summed with ONE all-reduce, and aggregates to what a single process
gets on the union of the two ranks' batches (the sums add, so the union's block is the sum of the blocks)."""
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iscale_ref as R   # noqa: E402

T, THR, FRAME = 3, [20, 30, 35, 40], (24, 40)
HW, AREA = FRAME[0] * FRAME[1], (FRAME[0] - 10) * (FRAME[1] - 10)
LEVELS = R.levels(*FRAME)[1] + 1
SAMPLES = (4, 6)   # per rank


def _block(rank):
    """what a rank's epoch could have left: integer counts, fractional sums, a header, and the block sums of the rank's own random frames"""
    n = len(THR)
    rng = np.random.default_rng(41 + rank)
    main = rng.integers(1, 1 << 30, (T, 4 * n + 3)).astype(np.float64)
    main[:, 4 * n:] += rng.random((T, 3))
    pooled = rng.integers(0, 1 << 30, T * 4 * n).astype(np.float64)
    tables = []
    for density in (0.3, 0.45):      # the forecast's table, the baseline's
        rows = np.zeros((T, LEVELS, 3 * n))
        for t in range(T):
            a, b = (np.where(rng.random((SAMPLES[rank],) + FRAME) < d, rng.random((SAMPLES[rank],) + FRAME), 0.0).astype(np.float32) for d in (0.4, density))
            rows[t] = R.ref_sums(a, b, THR, 90.0).sum(axis=0)
        tables.append(rows.ravel())
    return torch.from_numpy(np.concatenate([[1.5 + rank, 3 + rank, SAMPLES[rank], rank], main.ravel(), pooled] + tables))


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adnm-unet_amd"))
    from adnm_hip.validate import Validator, block_doubles, iscale_doubles
    from models.loss import enRainfallLoss
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    val = Validator(torch.nn.Identity(), enRainfallLoss(), T, 90.0, THR, process_group=dist.group.WORLD, persistence=True, intensity_scale=True)
    mine = _block(rank)
    assert mine.numel() == sum(block_doubles(T, len(THR), (), True)) + sum(iscale_doubles(T, len(THR), FRAME, True))
    val._block, val._frame = mine.clone(), FRAME      # the state an epoch of 24 x 40 frames leaves (no GPU here: the block is on the CPU)
    res = val.done(per_lead=True)
    q.put((rank, dict(res=repr(res), calls=len(calls), untouched=bool(torch.equal(val._block, mine)))))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_aggregate_to_the_union_with_one_all_reduce():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adnm-unet_amd"))
    from adnm_hip.validate import aggregate, intensity_scale_entries
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
    want = aggregate(union, THR, T, HW, AREA, persistence=True, per_lead=True, intensity_scale=FRAME)
    assert (want["batches"], want["samples"], want["nonfinite"]) == (7, 10, 1)
    assert list(want)[-3:] == ["persistence", "intensity_scale", "per_lead"] and list(want["persistence"])[-1] == "intensity_scale"
    # the union's score is the score of the summed sums, not a mean of the ranks' scores
    size = T * LEVELS * 3 * len(THR)
    tab = union[-2 * size:-size].reshape(T, LEVELS, 3 * len(THR))
    mine = intensity_scale_entries(tab.sum(axis=0), 10 * T, FRAME, THR)[30]
    e = want["intensity_scale"][30]
    assert np.array_equal(e["mse"], mine["mse"]) and (e["mse"] > 0).all() and abs(e["mse"].sum() - e["mse_total"]) < 1e-15
    assert want["per_lead"]["intensity_scale"][30]["mse"].shape == (T, LEVELS) and e["mse"].shape == (LEVELS,) and want["intensity_scale"]["domain_px"] == 64
    for r in (0, 1):
        assert res[r]["calls"] == 1, f"rank {r}: {res[r]['calls']} all-reduces"
        assert res[r]["untouched"], "done() reduced the epoch's block in place"
        assert res[r]["res"] == repr(want), f"rank {r}: not the single-process result on the union"
