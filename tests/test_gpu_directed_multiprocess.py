"""A directed graph searched by two processes (as test_gpu_multiprocess.py does for symmetric graphs): each takes
half of the directed pairs, routes them to the owners of their sources with pm.partition_edges over gloo, holds
its shard context (pm_create_shard_host_comm, symmetric = 0) on device 0, and the exchanges -- the in-row build,
the sharded push supersteps' messages, the replica -- go through TorchHostComm.  The search runs twice on the
same contexts; the result files and both runs' counters must equal the oracle's."""
import json
import os
import socket

import pytest
import torch.multiprocessing as mp

import fuzzypatternmatching_amd as pm
import directed_inputs as di
import pmtest

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        n = 1 << 12
        u, v = di.mixed_pairs(12, 4, 2)
        src, dst = u[rank::world], v[rank::world]  # this process's half of the pairs
        off, col, deg = pm.partition_edges(src, dst, n)
        comm = pm.TorchHostComm()
        m = pm.ShardedPatternMatcher(n, off, col, deg, di.PATTERNS["cycle"], world, rank, device=0, nranks=2,
                                     symmetric=False, host_comm=comm)
        m.set_labels(pmtest.hash_labels(n, 8))
        st = m.run_beta(os.path.join(out_dir, "shards"), max_iterations=100)  # collective; shard 0 writes
        st2 = m.run_beta("", max_iterations=100)  # a second search on the same contexts
        m.close()
        with open(os.path.join(out_dir, f"stats{rank}.json"), "w") as f:
            json.dump({"first": st, "second": st2}, f)
    finally:
        dist.destroy_process_group()


def test_directed_sharded_processes_match_oracle(tmp_path):
    world = 2
    mp.start_processes(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True,
                       start_method="spawn")
    off, col = di.mixed(12, 4, 2)
    assert not di.is_symmetric(off, col)
    labels = pmtest.hash_labels(off.shape[0] - 1, 8)
    so = di.run_oracle(off, col, di.PATTERNS["cycle"], tmp_path / "oracle", labels, 2)
    assert so["final_vertices"] == 510 and so["iterations"] == 2
    assert pmtest.compare_result_dirs(str(tmp_path / "oracle"), str(tmp_path / "shards"), 2) == []
    stats = [json.load(open(tmp_path / f"stats{r}.json")) for r in range(world)]
    for s in stats:
        for run in ("first", "second"):
            di.check_counters(so, s[run])
            assert s[run]["comm_calls"] > 0
    assert sum(s["first"]["shard_entries"] for s in stats) == int(off[-1])
