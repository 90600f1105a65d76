"""Directed inputs shared by the sharded directed-graph tests (test_gpu_directed_shards.py, the multi-process
and CLI tests beside it): graph builders, the patterns, and the comparison with the CPU oracle."""
import os

import numpy as np

import fuzzypatternmatching_amd as pm
import oracle
import pmtest

PATTERNS = {
    "tree": os.path.join(pmtest.ROOT, "patterns", "rmat_log2_tree_pattern"),
    "cycle": os.path.join(pmtest.ROOT, "patterns", "rmat_log2_cycle4_pattern"),
    "triangle": os.path.join(pmtest.ROOT, "patterns", "triangle_tail_pattern"),
    "wstar": os.path.join(pmtest.ROOT, "patterns", "wide_star_pattern"),      # diameter 2
    "wspider": os.path.join(pmtest.ROOT, "patterns", "wide_spider_pattern"),  # diameter 3
}


def mixed_pairs(scale, p_gen, back):
    """The generator's pairs (u, v) of every generator rank as directed edges u -> v; back > 0 appends the
    reverse v -> u of every pair whose index % back == 0.  With degree labels a pure one-way R-MAT (back = 0)
    leaves nothing after the later supersteps -- only edges present in both directions outlive superstep 1 --
    so the mixed graphs keep survivors."""
    und = [oracle.rmat_rank_edges(scale, p_gen, r) for r in range(p_gen)]
    u = np.concatenate([x[0] for x in und]).astype(np.uint64)
    v = np.concatenate([x[1] for x in und]).astype(np.uint64)
    if back > 0:
        k = np.arange(u.shape[0]) % back == 0
        u, v = np.concatenate([u, v[k]]), np.concatenate([v, u[k]])
    return u, v


def mixed(scale, p_gen, back):
    u, v = mixed_pairs(scale, p_gen, back)
    return pmtest.csr_from_edges(u, v, 1 << scale)


def star(L):
    """The 7-vertex tree embedding in both directions, plus L vertices of label 7 with an edge into vertex 1;
    only every even-numbered one also has the edge back from vertex 1.  M[1] holds 3 + L entries after
    superstep 0 (more than a push-form piece for L >= 254) and half of the extra ones die in superstep 1."""
    pairs = [(0, 1), (1, 2), (1, 3), (3, 5), (4, 5), (5, 6)]
    src = [a for a, b in pairs] + [b for a, b in pairs]
    dst = [b for a, b in pairs] + [a for a, b in pairs]
    for k in range(L):
        src.append(7 + k)
        dst.append(1)
        if k % 2 == 0:
            src.append(1)
            dst.append(7 + k)
    labels = np.array([3, 4, 7, 2, 3, 5, 7] + [7] * L, np.uint64)
    off, col = pmtest.csr_from_edges(src, dst, 7 + L)
    return off, col, labels


def is_symmetric(off, col):
    n = off.shape[0] - 1
    src = np.repeat(np.arange(n, dtype=np.uint64), np.diff(off).astype(np.int64))
    a = np.sort(src * np.uint64(n) + col.astype(np.uint64))
    b = np.sort(col.astype(np.uint64) * np.uint64(n) + src)
    return bool(np.array_equal(a, b))


def hubs(off, threshold):
    return int((np.diff(off) >= threshold).sum())


def check_counters(so, sg):
    assert sg["iterations"] == so["iterations"] and sg["terminated"] == so["terminated"]
    assert sg["final_vertices"] == so["final_vertices"] and sg["final_edges"] == so["final_edges"]
    assert sg["lcc_edges"] == so["lcc_edges"]
    assert sg["nlcc_edges"] == so["nlcc_edges"]
    assert sg["tds_edges"] == so["tds_edges"]
    assert sg["walks"] == so["paths"]


def run_oracle(off, col, pattern, out, labels=None, nranks=1, hub_threshold=pm.DEFAULT_HUB_THRESHOLD):
    return oracle.run(off, col, pattern, None if out is None else str(out), labels=labels, nranks=nranks,
                      max_iterations=100, hub_threshold=hub_threshold)


def run_shards(off, col, pattern, out, shards, labels=None, nranks=1, hub_threshold=pm.DEFAULT_HUB_THRESHOLD):
    g = pm.Graph(off, col, False, nranks, hub_threshold)
    return pm.run_beta_local_shards(g, pattern, shards, "" if out is None else str(out), max_iterations=100,
                                    labels=labels)
