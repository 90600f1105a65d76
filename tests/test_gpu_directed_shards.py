"""The sharded search of a directed graph against the CPU oracle.

A shard of a directed graph is given its owned out-rows (pm_shard_desc's shape for symmetric graphs); the shards
exchange them into the in-rows of the vertices they own when their contexts are built, superstep 0 pulls over
those, and the push-form later supersteps send what crosses a shard boundary as messages until the state is
replicated after superstep PM_HANDOFF (directed inputs: 0 replicates straight after superstep 0).  Every result
file and the counters must equal the oracle's for every shard count and hand-off.  The shards run as threads
of this process on one device (pm_run_beta_local_shards); one RCCL rank exercises the communicator itself.

The oracle's figures below were computed on the CPU; each case asserts them so that an input which no longer
exercises its path (no survivors, no hubs, a symmetric graph) fails here rather than passes empty."""
import numpy as np
import pytest

import fuzzypatternmatching_amd as pm
import directed_inputs as di
import pmtest

pytestmark = pytest.mark.gpu

DEFAULT = pm.DEFAULT_HUB_THRESHOLD


def _run_both(off, col, pattern, tmp_path, shards, labels=None, nranks=1, hub_threshold=DEFAULT):
    a, b = tmp_path / "oracle", tmp_path / "shards"
    so = di.run_oracle(off, col, pattern, a, labels, nranks, hub_threshold)
    sg = di.run_shards(off, col, pattern, b, shards, labels, nranks, hub_threshold)
    return so, sg, pmtest.compare_result_dirs(str(a), str(b), nranks)


# (input (scale, p_gen, back), pattern, label alphabet or None, result ranks, -d, hubs, shards,
#  oracle final_vertices, oracle iterations or None, environment)
MIXED_CASES = [
    ((12, 4, 0), "cycle", 8, 2, DEFAULT, 0, 2, 109, None, {}),
    ((13, 4, 0), "cycle", 16, 2, 16, 1277, 3, 47, 2, {}),
    ((14, 4, 2), "tree", None, 4, 32, 1827, 4, 36, None, {}),
    ((12, 4, 2), "cycle", 8, 2, DEFAULT, 0, 3, 510, 2, {}),
    ((12, 4, 2), "cycle", 8, 2, DEFAULT, 0, 3, 510, 2, {"PM_SPLIT_LINES": "1"}),
    ((13, 4, 3), "cycle", 16, 2, 24, 1129, 5, 182, None, {}),
    # push form on the replica in the later LCC calls (cycle flags)
    ((12, 4, 2), "triangle", 6, 1, DEFAULT, 0, 2, 765, 2, {}),
    # one label on three template vertices, diameters 2 and 3
    ((12, 4, 2), "wstar", 6, 1, 64, 299, 2, 676, None, {}),
    ((13, 4, 3), "wspider", 6, 2, 48, 776, 3, 1195, None, {}),
    ((10, 1, 0), "tree", 16, 1, DEFAULT, 0, 4, 22, None, {}),
]


@pytest.mark.parametrize("inp,pat,alphabet,nranks,thr,nhubs,shards,final_v,iters,env", MIXED_CASES)
def test_directed_shards_match_oracle(inp, pat, alphabet, nranks, thr, nhubs, shards, final_v, iters, env, tmp_path,
                                      monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    off, col = di.mixed(*inp)
    assert not di.is_symmetric(off, col)
    assert di.hubs(off, thr) == nhubs
    labels = None if alphabet is None else pmtest.hash_labels(off.shape[0] - 1, alphabet)
    so, sg, diffs = _run_both(off, col, di.PATTERNS[pat], tmp_path, shards, labels, nranks, thr)
    assert so["final_vertices"] == final_v
    if iters is not None:
        assert so["iterations"] == iters
    if inp == (12, 4, 2) and pat == "cycle":
        assert so["lcc_calls"] == 6
    assert diffs == []
    di.check_counters(so, sg)
    if nhubs:
        assert sg["hubs"] > 0


def test_directed_shards_empty_result(tmp_path):
    """Pure one-way R-MAT with degree labels: nothing outlives the later supersteps; the empty result is exact."""
    off, col = di.mixed(12, 2, 0)
    assert not di.is_symmetric(off, col)
    so, sg, diffs = _run_both(off, col, di.PATTERNS["tree"], tmp_path, 2)
    assert so["final_vertices"] == 0 and so["lcc_edges"] == 40824
    assert diffs == []
    di.check_counters(so, sg)


@pytest.mark.parametrize("L,nranks,thr,shards,expect", [
    (600, 3, 100, 2, (307, 612, 301)), (600, 3, 100, 3, (307, 612, 301)),
    (600, 3, DEFAULT, 2, (307, 612, 301)), (600, 3, DEFAULT, 3, (307, 612, 301)),
    (1500, 2, DEFAULT, 3, (757, 1512, 751))])
def test_directed_shards_long_row(L, nranks, thr, shards, expect, tmp_path):
    """M[1] is longer than a push-form piece after superstep 0 and half of it dies in superstep 1: the sharded
    senders' and the verify's piece launches; with -d 100 vertex 1 is a delegate (its out-row split)."""
    off, col, labels = di.star(L)
    assert not di.is_symmetric(off, col)
    if thr < DEFAULT:
        assert di.hubs(off, thr) == 1 and np.diff(off)[1] >= thr
    so, sg, diffs = _run_both(off, col, di.PATTERNS["tree"], tmp_path, shards, labels, nranks, thr)
    assert (so["final_vertices"], so["final_edges"], so["paths"]) == expect
    assert diffs == []
    di.check_counters(so, sg)


@pytest.mark.parametrize("shards", [2, 5])
def test_directed_shards_known_answer(shards, tmp_path):
    """The 8 one-way pairs of test_gpu_directed.py::test_directed_known_answer: most shards own nothing."""
    pairs = [(0, 1), (1, 2), (1, 3), (3, 5), (4, 5), (5, 6), (2, 1), (6, 5)]
    labels = np.array([3, 4, 7, 2, 3, 5, 7], np.uint64)
    off, col = pmtest.csr_from_edges([a for a, b in pairs], [b for a, b in pairs], 7)
    assert not di.is_symmetric(off, col)
    so, sg, diffs = _run_both(off, col, di.PATTERNS["tree"], tmp_path, shards, labels)
    assert so["final_vertices"] == 0 and so["lcc_edges"] == 14
    assert diffs == []
    di.check_counters(so, sg)


def _handoff_input(which):
    if which == "tree":
        off, col = di.mixed(14, 4, 2)
        return off, col, None, "tree", 4, 32, 4
    if which == "cycle":
        off, col = di.mixed(12, 4, 2)
        return off, col, pmtest.hash_labels(off.shape[0] - 1, 8), "cycle", 2, DEFAULT, 3
    off, col, labels = di.star(600)
    return off, col, labels, "tree", 3, 100, 2


@pytest.mark.parametrize("which", ["tree", "cycle", "star"])
def test_directed_shards_handoff(which, tmp_path, monkeypatch):
    """PM_HANDOFF = 0 (the replica straight after superstep 0), 1 and the default (2): identical results; each
    sharded push superstep adds its exchange, so the default makes more collective calls than PM_HANDOFF=0."""
    off, col, labels, pat, nranks, thr, shards = _handoff_input(which)
    a = tmp_path / "oracle"
    so = di.run_oracle(off, col, di.PATTERNS[pat], a, labels, nranks, thr)
    assert so["final_vertices"] > 0
    calls, steps = {}, {}
    for h in ("0", "1", None):
        if h is None:
            monkeypatch.delenv("PM_HANDOFF", raising=False)
        else:
            monkeypatch.setenv("PM_HANDOFF", h)
        b = tmp_path / f"shards_{h}"
        sg = di.run_shards(off, col, di.PATTERNS[pat], b, shards, labels, nranks, thr)
        assert pmtest.compare_result_dirs(str(a), str(b), nranks) == [], h
        di.check_counters(so, sg)
        calls[h], steps[h] = sg["comm_calls"], sg["shard_push_supersteps"]
        assert sg["shard_in_entries"] > 0
    assert calls[None] > calls["0"], calls
    assert calls["1"] > calls["0"], calls
    assert steps["0"] == 0 and steps["1"] == 1 and steps[None] >= 1, steps


def test_directed_rccl_shard_single_rank(tmp_path):
    """pm_create_shard with one rank and symmetric = 0: the RCCL communicator carries the sharded push
    supersteps' exchanges and the replica of a directed search."""
    off, col = di.mixed(12, 4, 2)
    labels = pmtest.hash_labels(off.shape[0] - 1, 8)
    deg = np.diff(off).astype(np.uint32)
    uid = pm.comm_unique_id()
    m = pm.ShardedPatternMatcher(off.shape[0] - 1, off, col, deg, di.PATTERNS["cycle"], 1, 0, uid, nranks=2,
                                 symmetric=False)
    m.set_labels(labels)
    sg = m.run_beta(str(tmp_path / "rccl"), max_iterations=100)
    m.close()
    so = di.run_oracle(off, col, di.PATTERNS["cycle"], tmp_path / "oracle", labels, 2)
    assert so["final_vertices"] == 510
    assert pmtest.compare_result_dirs(str(tmp_path / "oracle"), str(tmp_path / "rccl"), 2) == []
    di.check_counters(so, sg)
    assert sg["comm_calls"] > 0
