"""A directed 2-partition graph launched as two processes without a GPU: both meet over TCP, read their own
shards and fail alike at the device within the bootstrap timeout -- a directed graph is placed like a symmetric
one, so neither process takes the former fall-back (one context on rank 0 while the other waits for it)."""
import os
import socket
import subprocess

import numpy as np
import pytest

import fuzzypatternmatching_amd as pm
import pmtest

BIN = os.path.join(pmtest.ROOT, "fuzzypatternmatching_amd", "csrc", "tools", "bin")
TREE = os.path.join(pmtest.ROOT, "patterns", "rmat_log2_tree_pattern")


def _port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_directed_launched_ranks_without_gpu(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    g = pm.rmat_graph(10, 2)
    src = np.repeat(np.arange(g.n, dtype=np.uint64), np.diff(g.off).astype(np.int64))
    keep = src < g.col  # every pair one way only
    off, col = pmtest.csr_from_edges(src[keep], g.col[keep], g.n)
    base = str(tmp_path / "g")
    pm.write_graph(base, pm.Graph(off, col, False, 2), 2)
    assert pm.graph_partitions(base) == 2
    assert pm.read_graph_shard(base, 2, 1)[3]["symmetric"] is False
    out = tmp_path / "out"
    out.mkdir()
    port = _port()
    procs = []
    for r in range(2):
        env = dict(os.environ, PM_RANK=str(r), PM_WORLD_SIZE="2", PM_MASTER_ADDR="127.0.0.1",
                   PM_MASTER_PORT=str(port), PM_BOOTSTRAP_TIMEOUT="60")
        procs.append(subprocess.Popen([os.path.join(BIN, "run_pattern_matching_beta"), "-i", base, "-p", TREE,
                                       "-o", str(out)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                      text=True))
    outs = [p.communicate(timeout=120) for p in procs]
    for p, (so, se) in zip(procs, outs):
        assert p.returncode != 0, (so, se)
        assert "one context on rank 0" not in so, so
        assert "no HIP device" in se, se
    assert "2 ranks launched by PM" in outs[0][0]
    assert not os.listdir(out)
