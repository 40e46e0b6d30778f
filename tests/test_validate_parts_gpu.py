"""The Validator's launches follow validate.block_parts: with every option on, one step calls the Validator's entry points in the order of
the block's parts, once eagerly on the scratch block and once under capture, and each table-writing call gets its part's offset in the
block; with every option off, only the two entry points of the main block run.  This pins the sequence the captured graph holds."""
import pytest
import torch

from adnm_hip import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
FAMILY = ("adnm_valid_", "adnm_trec_", "adnm_advect")
ORDER = ["adnm_valid_accum", "adnm_valid_ssim_accum", "adnm_valid_pool_accum", "adnm_valid_pool_accum", "adnm_valid_fss_accum", "adnm_valid_fss_accum",
         "adnm_trec_motion", "adnm_advect", "adnm_valid_pool_accum", "adnm_valid_fss_accum", "adnm_valid_spectrum_accum", "adnm_valid_joint_accum"]
WRITERS = ("adnm_valid_pool_accum", "adnm_valid_fss_accum", "adnm_valid_spectrum_accum", "adnm_valid_joint_accum")


class LastFrames(torch.nn.Module):
    def forward(self, x):
        return x[:, -1:, 0].float().expand(-1, 3, -1, -1) * 0.9


def _one_step(monkeypatch, **options):
    """-> (the Validator after one step, the calls of its entry points as (name, args))"""
    from adnm_hip.validate import Validator
    from models.loss import RainfallLoss
    gen = torch.Generator().manual_seed(7)
    x, tgt = torch.rand(2, 2, 1, 16, 16, generator=gen).to(DEV), torch.rand(2, 3, 1, 16, 16, generator=gen).to(DEV)
    calls, call = [], lib.call

    def recorder(name, *args):
        if name.startswith(FAMILY):
            calls.append((name, args))
        return call(name, *args)
    val = Validator(LastFrames(), RainfallLoss(), 3, 90.0, (20, 30), **options)
    with monkeypatch.context() as m:
        m.setattr(lib, "call", recorder)
        val.step(x, tgt)
    torch.cuda.synchronize()
    return val, calls


def test_launches_and_table_pointers_follow_the_parts(monkeypatch):
    from adnm_hip import ops
    from adnm_hip.validate import block_parts
    val, calls = _one_step(monkeypatch, pools=(4,), persistence=True, fss=(5,), advection=(8, 2), spectrum=True, joint=True)
    try:
        assert [name for name, _ in calls] == ORDER + ORDER   # the eager run on the scratch block, then the capture
        parts, total = block_parts(3, 2, ((4, 4),), True, (5,), True, (16, 16), ops.joint_levels(90.0))
        assert len(parts) == 9 and val._block.numel() == total
        tables = [args[4] for name, args in calls[len(ORDER):] if name in WRITERS]
        assert tables == [val._block.data_ptr() + 8 * p.offset for p in parts[1:]]
        assert all(args[2] == val._block.data_ptr() for name, args in calls[len(ORDER):] if name in ORDER[:2])   # the main block itself
    finally:
        val.close()


def test_no_option_launches_the_main_block_alone(monkeypatch):
    from adnm_hip.validate import block_doubles
    val, calls = _one_step(monkeypatch)
    try:
        assert [name for name, _ in calls] == ORDER[:2] * 2
        assert val._block.numel() == block_doubles(3, 2)[0]
    finally:
        val.close()
