"""validate.block_parts, the one statement of the Validator block's order, without a GPU: for all 64 on/off combinations of {pools,
persistence, fss, advection, spectrum, joint} the parts are the documented ones in the documented order, contiguous from 0, uniquely
named, and as large as the five *_doubles helpers say; and for the block with every option on, each group of entries aggregate returns
is what it returns when that group's tables are the only ones there are, so no table is read at another's offset."""
import itertools
import math

import numpy as np
import pytest

from adnm_hip import ops
from adnm_hip.validate import (HEADER, advection_doubles, aggregate, baseline_pools, block_doubles, block_parts, fss_doubles, joint_doubles,
                               spectrum_doubles)
from test_joint_host import _same_tree   # bitwise, NaN equal to NaN, the keys in order

T, THR, POOLS, FSS, FRAME, SCALE = 3, [20, 30.5], ((4, 4), (16, 8)), (1, 5), (16, 32), 6.5
L = 7   # ops.joint_levels(SCALE)
HW, AREA = FRAME[0] * FRAME[1], (FRAME[0] - 10) * (FRAME[1] - 10)
COMBOS = list(itertools.product((False, True), repeat=6))


def _options(pools, persistence, fss, advection, spectrum, joint):
    return dict(pools=POOLS if pools else (), persistence=persistence, fss=FSS if fss else (), advection=advection,
                spectrum=FRAME if spectrum else None, joint=L if joint else None)


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "".join("01"[v] for v in c))
def test_parts_of_every_option_set(combo):
    pools, persistence, fss, advection, spectrum, joint = combo
    kw = _options(*combo)
    n, base = len(THR), baseline_pools(kw["pools"])
    parts, total = block_parts(T, n, **kw)
    want = [("main", "main", None, (), (HEADER + T * (4 * n + 3),), True),
            ("pooled", "pool", "pred", POOLS, (T, len(POOLS), 4 * n), pools),
            ("persistence/pooled", "pool", "last", base, (T, len(base), 4 * n), persistence),
            ("fss", "fss", "pred", (), (T, len(FSS), 3 * n), fss),
            ("persistence/fss", "fss", "last", (), (T, len(FSS), 3 * n), fss and persistence),
            ("advection/pooled", "pool", "adv", base, (T, len(base), 4 * n), advection),
            ("advection/fss", "fss", "adv", (), (T, len(FSS), 3 * n), fss and advection),
            ("spectrum", "spectrum", "pred", (), (T, max(FRAME) // 2, 3), spectrum),
            ("joint", "joint", "pred", (), (T, L, L), joint)]
    assert [tuple(p[:5]) for p in parts] == [w[:5] for w in want if w[5]]
    assert len({p.name for p in parts}) == len(parts)
    at = 0
    for p in parts:                      # ascending and contiguous from 0
        assert p.offset == at and p.size == math.prod(p.shape) > 0
        at += p.size
    assert ops.joint_levels(SCALE) == L
    helpers = (block_doubles(T, n, kw["pools"], persistence) + fss_doubles(T, n, kw["fss"], persistence)
               + advection_doubles(T, n, kw["pools"], kw["fss"], advection) + (spectrum_doubles(T, kw["spectrum"]), joint_doubles(T, SCALE if joint else None)))
    assert total == at == sum(p.size for p in parts) == sum(helpers)
    size = {p.name: p.size for p in parts}
    assert helpers == tuple(size.get(w[0], 0) for w in want)   # each helper's figure is its part's, in the block's order


# the groups of entries, each with the smallest option set under which aggregate returns the same entries, and the parts that are the group's
GROUPS = {"pooled": (dict(pools=POOLS), ("pooled",)),
          "persistence": (dict(pools=POOLS, fss=FSS, persistence=True), ("persistence/pooled", "persistence/fss")),
          "fss": (dict(fss=FSS), ("fss",)),
          "advection": (dict(pools=POOLS, fss=FSS, advection=True), ("advection/pooled", "advection/fss")),
          "spectrum": (dict(spectrum=FRAME), ("spectrum",)),
          "joint": (dict(joint=L), ("joint",))}


@pytest.fixture(scope="module")
def full():
    """the block with every option on, integers (no two tables alike), and what aggregate makes of it"""
    kw = _options(*(True,) * 6)
    parts, total = block_parts(T, len(THR), **kw)
    blk = np.random.default_rng(20).integers(1, 1000, total).astype(np.float64)
    blk[:HEADER] = (12.5, 6, 12, 1)
    blk.setflags(write=False)
    return blk, {p.name: p for p in parts}, aggregate(blk, THR, T, HW, AREA, per_lead=True, **kw)


@pytest.mark.parametrize("group", list(GROUPS))
def test_each_group_of_entries_comes_from_its_own_tables(full, group):
    """The block is cut down to main plus the group's tables.  A baseline's entries are keyed by the forecast's pools and scales, so its
    option set keeps the forecast's pooled and FSS tables: those are there as ZEROS, which nothing of the group may read."""
    blk, whole, res = full
    kw, mine = GROUPS[group]
    parts, total = block_parts(T, len(THR), **kw)
    cut = np.zeros(total)
    for p in parts:
        if p.name == "main" or p.name in mine:
            cut[p.offset:p.offset + p.size] = blk[whole[p.name].offset:whole[p.name].offset + p.size]
    assert {p.name for p in parts} >= set(mine) and all(whole[p.name].shape == p.shape for p in parts)
    alone = aggregate(cut, THR, T, HW, AREA, per_lead=True, **kw)
    assert _same_tree(res[group], alone[group]), f"{group}: not the entries of its tables alone"
    assert _same_tree(res["per_lead"][group], alone["per_lead"][group]), f"per_lead/{group}: not the entries of its tables alone"
    if group == "fss":
        assert _same_tree(res["fss_useful"], alone["fss_useful"])
    plain = aggregate(blk[:whole["main"].size], THR, T, HW, AREA, per_lead=True)
    assert _same_tree({k: res[k] for k in plain if k != "per_lead"}, {k: plain[k] for k in plain if k != "per_lead"})
    assert _same_tree({k: res["per_lead"][k] for k in plain["per_lead"]}, plain["per_lead"])


def test_key_order_with_every_option_on(full):
    res = full[2]
    tail = ["pooled", "persistence", "fss", "fss_useful", "advection", "spectrum", "joint", "per_lead"]
    assert list(res)[-len(tail):] == tail and list(res["per_lead"])[-6:] == [k for k in tail[:-1] if k != "fss_useful"]
    for name in ("persistence", "advection"):
        assert list(res[name]) == ["threshold_metrics", "FAR", "pooled", "fss"] and list(res["per_lead"][name]) == ["threshold_metrics", "pooled", "fss"]
