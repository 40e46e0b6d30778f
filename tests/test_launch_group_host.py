"""CPU-side checks of the launch group (include/adnm_hip.h: adnm_group_*): the refusals happen on the host, before any launch."""
import pytest

from adnm_hip import lib, ops


@pytest.fixture(autouse=True)
def _closed_group():
    lib.load().adnm_group_clear()
    yield
    lib.load().adnm_group_clear()


def test_empty_group_launches_nothing_and_is_ok():
    L = lib.load()
    assert L.adnm_group_begin() == 0
    assert L.adnm_group_pending() == 0
    assert L.adnm_group_launch(None) == 0
    assert L.adnm_group_begin() == 0, "the launch closed the group: a new one opens"
    assert L.adnm_group_clear() == 0
    assert L.adnm_group_launch(None) == 0, "nothing recorded, no group open: still nothing to do"


def test_nested_begin_is_refused():
    L = lib.load()
    assert L.adnm_group_begin() == 0
    assert L.adnm_group_begin() == -1 and "already open" in lib.last_error()
    assert L.adnm_group_clear() == 0
    assert L.adnm_group_begin() == 0


def test_queue_flushes_are_refused_while_a_group_is_open():
    L = lib.load()
    fq, lq = L.adnm_foldq_create(), L.adnm_leafq_create()
    try:
        assert L.adnm_foldq_flush(fq, None) == 0 and L.adnm_leafq_flush(lq, None) == 0   # empty queues, no group: fine
        assert L.adnm_group_begin() == 0
        assert L.adnm_foldq_flush(fq, None) == -1 and "launch group is open" in lib.last_error()
        assert L.adnm_leafq_flush(lq, None) == -1 and "launch group is open" in lib.last_error()
        assert L.adnm_group_launch(None) == 0
        assert L.adnm_foldq_flush(fq, None) == 0 and L.adnm_leafq_flush(lq, None) == 0
    finally:
        L.adnm_foldq_destroy(fq)
        L.adnm_leafq_destroy(lq)


def test_bracket_clears_the_group_on_an_exception():
    with pytest.raises(KeyError):
        with ops.GROUP:
            assert ops.GROUP.open
            raise KeyError("inside the bracket")
    assert not ops.GROUP.open
    assert lib.load().adnm_group_begin() == 0, "the exception path closed the library's group"


def test_nested_bracket_is_refused_and_leaves_nothing_open():
    with pytest.raises(RuntimeError, match="already open"):
        with ops.GROUP:
            with ops.GROUP:
                pass
    assert not ops.GROUP.open
    assert lib.load().adnm_group_begin() == 0


def test_split_offsets_are_disjoint_inside_a_bracket_and_zero_outside():
    assert ops.GROUP.split_offsets(1024, 5000) == (0, 0)
    assert ops.GROUP.split_offsets(1024, 5000) == (0, 0)
    with pytest.raises(KeyError):
        with ops.GROUP:
            assert ops.GROUP.split_offsets(300, 5000) == (0, 0)
            assert ops.GROUP.split_offsets(256, 100) == (512, 5120)
            assert ops.GROUP.split_offsets(256, 100) == (768, 5376)
            raise KeyError("leave without a stream")
    assert ops.GROUP.split_offsets(1024, 5000) == (0, 0)
