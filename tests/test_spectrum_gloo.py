"""Validator.done() with spectrum=True on more than one rank, 2 gloo ranks on the CPU: the spectrum table is the last part of the ONE
allocation, which is summed with ONE all-reduce, and aggregates to what a single process gets on the union of the two ranks' batches
(the sums add, so the union's block is the sum of the blocks)."""
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

T, THR, FSS, FRAME = 4, [20, 30, 35, 40], (1, 5), (16, 64)
HW, AREA, R = 16 * 64, 6 * 54, 32


def _block(rank):
    """what a rank's half epoch could have left: a header, integer counts, fractional sums, integer FSS sums, and a spectrum table with
    a forecast that loses power towards the small scales and |C| <= sqrt(P_o P_f)"""
    n = len(THR)
    rng = np.random.default_rng(41 + rank)
    main = rng.integers(1, 1 << 30, (T, 4 * n + 3)).astype(np.float64)
    main[:, 4 * n:] += rng.random((T, 3))
    fss = rng.integers(1, 1 << 40, (T * len(FSS) * n, 3)).astype(np.float64)
    fss[:, 2] = np.floor(np.sqrt(fss[:, 0] * fss[:, 1]) * rng.random(len(fss)))
    spec = rng.random((T, R, 3)) * 1e4 / (1.0 + np.arange(R))[None, :, None] ** 2
    spec[..., 1] = spec[..., 0] * np.linspace(1.0, 0.2, R)[None, :] * (0.9 + 0.2 * rng.random((T, R)))
    spec[..., 2] = np.sqrt(spec[..., 0] * spec[..., 1]) * (2 * rng.random((T, R)) - 1)
    return torch.from_numpy(np.concatenate([[1.5 + rank, 3 + rank, 12 + 4 * rank, rank], main.ravel(), fss.ravel(), spec.ravel()]))


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adnm-unet_amd"))
    from adnm_hip.validate import Validator, block_doubles, fss_doubles, spectrum_doubles
    from models.loss import enRainfallLoss
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    val = Validator(torch.nn.Identity(), enRainfallLoss(), T, 90.0, THR, process_group=dist.group.WORLD, fss=FSS, spectrum=True)
    mine = _block(rank)
    assert mine.numel() == block_doubles(T, len(THR))[0] + sum(fss_doubles(T, len(THR), FSS)) + spectrum_doubles(T, FRAME)
    val._block, val._frame = mine.clone(), FRAME      # the state a half epoch of 16 x 64 frames leaves (no GPU here: the block is on the CPU)
    res = val.done(per_lead=True)
    q.put((rank, dict(res=repr(res), calls=len(calls), untouched=bool(torch.equal(val._block, mine)))))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_aggregate_to_the_union_with_one_all_reduce():
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "adnm-unet_amd"))
    from adnm_hip import ops
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
    want = aggregate(union, THR, T, HW, AREA, per_lead=True, fss=FSS, spectrum=FRAME)
    assert (want["batches"], want["samples"], want["nonfinite"]) == (7, 28, 1)
    # the union's spectrum is that of the summed sums, not a mean of the ranks' spectra
    tab = union[-T * R * 3:].reshape(T, R, 3).sum(0)
    n_r, wavelength = ops.spectrum_bins(*FRAME)
    sp = want["spectrum"]
    assert np.allclose(sp["forecast"], tab[:, 1] / (n_r * 28 * T), rtol=1e-15) and np.allclose(sp["ratio"], tab[:, 1] / tab[:, 0], rtol=1e-15)
    assert np.isfinite(sp["coherence"]).all() and (np.abs(sp["coherence"]) <= 1).all()
    assert sp["ratio"][1] >= 0.5 and (sp["ratio"][1:] < 0.5).any() and 64.0 / 31 < sp["effective_resolution_px"] <= 64.0
    assert want["per_lead"]["spectrum"]["ratio"].shape == (T, R)
    for r in (0, 1):
        assert res[r]["calls"] == 1, f"rank {r}: {res[r]['calls']} all-reduces"
        assert res[r]["untouched"], "done() reduced the epoch's block in place"
        assert res[r]["res"] == repr(want), f"rank {r}: not the single-process result on the union"
