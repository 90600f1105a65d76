"""The drop-in executable on a directed P-partition graph: ingest_edge_list with no -u (directed, the reference's
default) writes P partitions, and run_pattern_matching_beta places the search like a symmetric graph's in all
three modes -- in-process shards, one thread and GPU per shard (PM_SHARDS=1 here), launched processes each
reading its own shard -- with the same "Shards ..." line and no fall-back to one context on rank 0.  Every
per-rank result file must equal the P-rank oracle's."""
import os
import socket
import subprocess

import numpy as np
import pytest

import fuzzypatternmatching_amd as pm
import directed_inputs as di
import oracle
import pmtest

pytestmark = pytest.mark.gpu

BIN = os.path.join(pmtest.ROOT, "fuzzypatternmatching_amd", "csrc", "tools", "bin")
CLI = os.path.join(BIN, "run_pattern_matching_beta")
CYCLE = di.PATTERNS["cycle"]
N = 1 << 13


def _port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.fixture(scope="module")
def edges_txt(tmp_path_factory):
    u, v = di.mixed_pairs(13, 4, 3)
    txt = tmp_path_factory.mktemp("directed_cli") / "edges.txt"
    np.savetxt(txt, np.stack([u, v], 1), fmt="%d")
    # -v label files: hash labels of 16 letters (the 4-cycle pattern keeps 182 vertices on them)
    labels = pmtest.hash_labels(N, 16)
    for i, part in enumerate(np.array_split(np.arange(N), 2)):
        with open(txt.parent / f"lab.{i}", "w") as f:
            f.write("".join(f"{x} {labels[x]}\n" for x in part))
    return txt


def _ingest(txt, base, P):
    r = subprocess.run([os.path.join(BIN, "ingest_edge_list"), "-o", str(base), "-n", str(P), "-d", "48", str(txt)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    g = pm.read_graph(str(base))
    assert not g.symmetric and g.nranks == P and g.hub_threshold == 48
    assert di.hubs(g.off, 48) > 0
    return g


def _oracle(g, out):
    so = oracle.run(g.off, g.col, CYCLE, str(out), labels=pmtest.hash_labels(g.n, 16), nranks=g.nranks,
                    hub_threshold=g.hub_threshold, threads=oracle.default_threads())
    assert so["final_vertices"] == 182
    return so


def _cmd(txt, base, out):
    return [CLI, "-i", str(base), "-v", str(txt.parent / "lab"), "-p", CYCLE, "-o", str(out)]


def _cli(txt, base, out, env=None):
    os.makedirs(out, exist_ok=True)
    return subprocess.run(_cmd(txt, base, out), capture_output=True, text=True,
                          env=dict(os.environ, **(env or {})), timeout=300)


def test_cli_directed_in_process_shards(edges_txt, tmp_path):
    g = _ingest(edges_txt, tmp_path / "g", 4)
    r = _cli(edges_txt, tmp_path / "g", tmp_path / "gpu")
    assert r.returncode == 0, r.stderr
    assert "Shards 4 (in-process on one GPU)" in r.stdout, r.stdout
    assert "one context on rank 0" not in r.stdout
    _oracle(g, tmp_path / "oracle")
    assert pmtest.compare_result_dirs(str(tmp_path / "oracle"), str(tmp_path / "gpu"), 4) == []


def test_cli_directed_gpu_threads_one_shard(edges_txt, tmp_path):
    g = _ingest(edges_txt, tmp_path / "g", 4)
    r = _cli(edges_txt, tmp_path / "g", tmp_path / "gpu", env={"PM_SHARDS": "1"})
    assert r.returncode == 0, r.stderr
    assert "one GPU each" in r.stdout, r.stdout
    assert "one context on rank 0" not in r.stdout
    _oracle(g, tmp_path / "oracle")
    assert pmtest.compare_result_dirs(str(tmp_path / "oracle"), str(tmp_path / "gpu"), 4) == []


def test_cli_directed_launched_processes(edges_txt, tmp_path):
    g = _ingest(edges_txt, tmp_path / "g", 2)
    port = _port()
    out = tmp_path / "gpu"
    out.mkdir()
    procs = []
    for q in range(2):
        env = dict(os.environ, PM_RANK=str(q), PM_WORLD_SIZE="2", PM_MASTER_ADDR="127.0.0.1",
                   PM_MASTER_PORT=str(port), PM_BOOTSTRAP_TIMEOUT="90")
        procs.append(subprocess.Popen(_cmd(edges_txt, tmp_path / "g", out), env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = []
    try:
        outs = [p.communicate(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, (so, se)
    assert "Shards 2 (2 processes, host collectives of 2 ranks)" in outs[0][0], outs[0][0]
    assert all("one context on rank 0" not in so for so, se in outs)
    _oracle(g, tmp_path / "oracle")
    assert pmtest.compare_result_dirs(str(tmp_path / "oracle"), str(out), 2) == []
