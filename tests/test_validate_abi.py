"""The entry points of the on-device validation epoch at the C boundary, without a GPU: declared in include/adnm_hip.h, exported by the
library, additive (they left the ABI version as it was), and refusing shapes outside their limits before any launch."""
import ctypes

from adnm_hip import lib

NEW = ("adnm_valid_accum", "adnm_valid_ssim_accum")
QUERIES = ("adnm_valid_block_bytes", "adnm_valid_accum_ws_bytes", "adnm_valid_ssim_accum_ws_bytes")


def test_new_prototypes_are_declared_and_exported_and_the_abi_version_stays():
    protos = lib.parse_header()
    so = ctypes.CDLL(lib.LIB_PATH)
    for name in NEW + QUERIES:
        assert name in protos, f"{name} is not declared in include/adnm_hip.h"
        assert hasattr(so, name), f"{name} declared but not exported"
    for name in NEW:
        assert protos[name][0] == "int" and protos[name][1][-1] == "adnm_stream_t"
    for name in QUERIES:
        assert protos[name][0] == "int64_t"
    assert lib.load().adnm_abi_version() == 11


def test_workspace_queries_refuse_what_the_kernels_cannot_take():
    q = lib.query
    assert q("adnm_valid_accum_ws_bytes", 80, 20, 128 * 128, 4) == 4 * 80 * 19 * 4      # 4 workgroups per frame, 19 fp32 columns
    assert q("adnm_valid_ssim_accum_ws_bytes", 80, 20, 128, 128, 4) == q("adnm_eval_ssim_ws_bytes", 80, 128, 128) > 0
    assert q("adnm_valid_block_bytes", 20, 4) == 8 * (4 + 20 * 19)
    for name, args in (("adnm_valid_accum_ws_bytes", lambda fr, T, hw, n: (fr, T, hw, n)),
                       ("adnm_valid_ssim_accum_ws_bytes", lambda fr, T, hw, n: (fr, T, hw // 64, 64, n))):
        assert q(name, *args(80, 20, 4096, 4)) > 0
        assert q(name, *args(80, 7, 4096, 4)) == -1, "T does not divide frames"
        assert q(name, *args(80, 0, 4096, 4)) == -1, "T = 0"
        assert q(name, *args(80, 20, 4096, 0)) == -1 and q(name, *args(80, 20, 4096, 9)) == -1, "nthr outside 1..8"
        assert q(name, *args(80, 20, 1 << 24, 4)) == -1, "hw >= 2^24"
        assert q(name, *args(65540, 20, 4096, 4)) == -1, "frames > 65535"
    assert q("adnm_valid_ssim_accum_ws_bytes", 80, 20, 10, 64, 4) == -1, "no valid region for the 11 x 11 window"
    assert q("adnm_valid_block_bytes", 0, 4) == -1 and q("adnm_valid_block_bytes", 20, 9) == -1


def test_arguments_are_checked_on_the_host():
    so = lib.load()
    thr = (ctypes.c_float * 4)(20, 30, 35, 40)
    assert so.adnm_valid_accum(None, 16, 16, None, thr, 4, 90.0, 0.57, 0.25, 0.0, 16, 1 << 20, 10, 5, 64, None) == -1 and "null pointer" in lib.last_error()
    assert so.adnm_valid_accum(16, 16, 12, None, thr, 4, 90.0, 0.57, 0.25, 0.0, 16, 1 << 20, 10, 5, 64, None) == -1 and "8-byte aligned" in lib.last_error()
    assert so.adnm_valid_accum(16, 16, 16, None, thr, 4, 90.0, 0.57, 0.25, 0.0, 16, 1 << 20, 10, 3, 64, None) == -1 and "bad shape" in lib.last_error()
    assert so.adnm_valid_accum(16, 16, 16, None, thr, 9, 90.0, 0.57, 0.25, 0.0, 16, 1 << 20, 10, 5, 64, None) == -1 and "bad shape" in lib.last_error()
    assert so.adnm_valid_accum(16, 16, 16, None, thr, 4, 90.0, 0.57, 0.25, 0.0, 16, 8, 10, 5, 64, None) == -3 and "workspace" in lib.last_error()
    assert so.adnm_valid_ssim_accum(16, None, 16, 4, 90.0, 16, 1 << 20, 10, 5, 16, 16, None) == -1 and "null pointer" in lib.last_error()
    assert so.adnm_valid_ssim_accum(16, 16, 16, 4, 90.0, 16, 1 << 20, 10, 5, 8, 8, None) == -1 and "10 x 10" in lib.last_error()
    assert so.adnm_valid_ssim_accum(16, 16, 16, 4, 90.0, 16, 1 << 20, 10, 4, 16, 16, None) == -1 and "bad shape" in lib.last_error()
    assert so.adnm_valid_ssim_accum(16, 16, 16, 4, 90.0, 16, 8, 10, 5, 16, 16, None) == -3 and "workspace" in lib.last_error()
