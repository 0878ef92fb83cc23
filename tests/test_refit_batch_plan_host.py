"""CPU: twk_refit_batch_plan_host (csrc/refit_batch_plan.h, the code a batched refit plans its launches with) against a numpy
restatement, word for word: tree k of n_k nodes and s_k slots takes ceil(n_k / 256) node blocks and ceil(s_k / 256) slot blocks in
the order given; per block (tree, tree-local index of the first thread); per tree the running node and slot offsets and the first
block of either kind; the totals. And its refusals: no tree, a tree without a node or a slot, 2^31 or more of anything."""
import ctypes as C

import numpy as np
import pytest

BLOCK = 256
SIZES = {
    "one": [1],
    "around-a-block": [255, 256, 257],
    "ones": [1, 1, 1],
    "mixed": [2049, 1, 511, 512],
    "many": [1] * 1100,
}


def _restate(nodes, slots):
    """The plan, in plain numpy."""
    nodes, slots = np.asarray(nodes, np.int64), np.asarray(slots, np.int64)
    out = {}
    for key, counts in (("node", nodes), ("slot", slots)):
        blocks = (counts + BLOCK - 1) // BLOCK
        out[key + "Offsets"] = np.concatenate(([0], np.cumsum(counts)[:-1]))
        out[key + "BlockFirst"] = np.concatenate(([0], np.cumsum(blocks)[:-1]))
        table = [(k, BLOCK * b) for k in range(counts.size) for b in range(int(blocks[k]))]
        out[key + "BlockTable"] = np.array(table, np.int64).reshape(-1, 2)
    out.update(trees=nodes.size, nodeBlocks=out["nodeBlockTable"].shape[0], slotBlocks=out["slotBlockTable"].shape[0], blockThreads=BLOCK, nodes=int(nodes.sum()), slots=int(slots.sum()))
    return out


@pytest.mark.parametrize("name", sorted(SIZES))
@pytest.mark.parametrize("slots_of", ["n + 1", "same", "reversed"])
def test_the_plan_equals_its_restatement(twk, name, slots_of):
    """Node counts from the list; slot counts n + 1 (a tree over n + 1 triangles has n nodes), the same list, and the list reversed
    (so that node and slot blocks of a tree differ in number)."""
    nodes = SIZES[name]
    slots = {"n + 1": [n + 1 for n in nodes], "same": list(nodes), "reversed": list(reversed(nodes))}[slots_of]
    got, want = twk.refit_batch_plan_host(nodes, slots), _restate(nodes, slots)
    for key in ("trees", "nodeBlocks", "slotBlocks", "blockThreads", "nodes", "slots"):
        assert got[key] == want[key], (key, got[key], want[key])
    for key in ("nodeOffsets", "slotOffsets", "nodeBlockFirst", "slotBlockFirst", "nodeBlockTable", "slotBlockTable"):
        assert np.array_equal(np.asarray(got[key], np.int64), want[key]), key
    # what the tables are for: every block lies inside one tree, and a tree's blocks cover it once, in order
    for key, counts in (("nodeBlockTable", nodes), ("slotBlockTable", slots)):
        table = got[key]
        assert np.all(table[:, 1] < np.asarray(counts)[table[:, 0]]) and np.all(table[:, 1] % BLOCK == 0)
        assert np.all(np.diff(table[:, 0]) >= 0)
        for k in range(len(counts)):
            assert np.array_equal(table[table[:, 0] == k, 1], np.arange(0, counts[k], BLOCK)), (key, k)


def test_the_totals_come_without_the_tables(twk):
    L = twk._lib
    n, s = np.array([300, 2], np.int32), np.array([301, 3], np.int32)
    ip = C.POINTER(C.c_int)
    plan = L.RefitBatchPlan()
    assert L.lib.twk_refit_batch_plan_host(n.ctypes.data_as(ip), s.ctypes.data_as(ip), 2, C.byref(plan), None, None, None, None, None, None) == L.TWK_SUCCESS
    assert (plan.trees, plan.nodeBlocks, plan.slotBlocks, plan.blockThreads, plan.nodes, plan.slots) == (2, 3, 3, BLOCK, 302, 304)


def test_refusals(twk):
    L = twk._lib
    ip = C.POINTER(C.c_int)
    plan = L.RefitBatchPlan()

    def refused(nodes, slots, *words, count=None, with_plan=True):
        n, s = np.asarray(nodes, np.int32), np.asarray(slots, np.int32)
        rc = L.lib.twk_refit_batch_plan_host(n.ctypes.data_as(ip) if n.size else None, s.ctypes.data_as(ip) if s.size else None, n.size if count is None else count,
                                             C.byref(plan) if with_plan else None, None, None, None, None, None, None)
        text = L.lib.twk_last_error().decode()
        assert rc == L.TWK_ERROR_INVALID_VALUE and "twk_refit_batch_plan_host" in text, (rc, text)
        for w in words:
            assert w in text, text

    refused([], [], "no tree")
    refused([1], [1], "no tree", count=0)
    refused([1], [1], "no tree", count=-3)
    refused([4, 0], [5, 1], "without a node")
    refused([4, 3], [5, 0], "without a slot")
    refused([4, -1], [5, 2], "without a node")
    refused([1], [1], "NULL", with_plan=False)
    big = 1 << 30
    refused([big, big], [1, 1], "2^31")                    # 2^31 nodes
    refused([1, 1], [big, big], "2^31")                    # 2^31 slots
    refused([big, big - 1], [1, 1], "2^31")                # 2^31 - 1 nodes, but 2^31 threads: the last block is rounded up
    with pytest.raises(twk.TwkError):
        twk.refit_batch_plan_host([1, 2], [0, 2])
    assert L.lib.twk_refit_batch_plan_host(None, None, 2, C.byref(plan), None, None, None, None, None, None) == L.TWK_ERROR_INVALID_VALUE
