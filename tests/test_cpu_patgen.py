"""tests/patgen.py on the CPU: the generator is deterministic and obeys the line rules, the host loader takes its
16-vertex / 16-position patterns (and still refuses a 17th position), and the oracle gives the fixed families' known
answers on copies plus decoys."""
import filecmp
import os

import numpy as np
import pytest

import fuzzypatternmatching_amd as pm
import oracle
import patgen

FIXED = ["chain16_ends", "ring15_tail", "fan7", "fan4", "star5"]
RANDOM_SEEDS = list(range(64))


def _write(fam, d):
    return patgen.write_pattern(d, fam["labels"], fam["pairs"], fam["diameter"], fam["lines"])


def test_generator_is_deterministic_per_seed(tmp_path):
    for seed in (0, 7, 31):
        a, b = patgen.random_template(seed), patgen.random_template(seed)
        assert a == b
        _write(a, tmp_path / f"a{seed}")
        _write(b, tmp_path / f"b{seed}")
        for name in os.listdir(tmp_path / f"a{seed}" / "0"):
            assert filecmp.cmp(tmp_path / f"a{seed}" / "0" / name, tmp_path / f"b{seed}" / "0" / name, shallow=False)
        ga = patgen.planted_graph(a, 3, 2, True, seed, hub=True)
        gb = patgen.planted_graph(b, 3, 2, True, seed, hub=True)
        assert all(np.array_equal(x, y) for x, y in zip(ga[:3], gb[:3])) and ga[3] == gb[3]
    assert patgen.random_template(1) != patgen.random_template(2)
    assert {patgen.random_template(s)["K"] for s in RANDOM_SEEDS} >= {3, 16}


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_templates_obey_the_line_rules(seed):
    t = patgen.random_template(seed)
    K, labels = t["K"], t["labels"]
    assert 2 <= K <= 16 and len(labels) == K and len(t["lines"]) == 5
    edges = {(a, b) for a, b in t["pairs"]} | {(b, a) for a, b in t["pairs"]}
    assert len(t["pairs"]) in (K - 1, K)  # a tree or one cycle
    for pl, (walk, vc) in enumerate(t["lines"]):
        assert 3 <= len(walk) <= 16
        assert all((a, b) in edges for a, b in zip(walk, walk[1:])), "the walk follows template edges"
        if pl < 4:  # distinct interior labels, equal end labels, a cycle closes on its source and a path does not
            ls = [labels[x] for x in walk]
            assert ls[0] == ls[-1] and (walk[0] == walk[-1]) == bool(vc)
            assert all(ls.count(x) == 1 for x in ls[1:-1])
        else:
            assert vc == 0 and walk.index(walk[-1]) == len(walk) - 1
    assert patgen.lines_ok(labels, t["lines"])


@pytest.mark.parametrize("name", FIXED)
def test_host_loader_accepts_the_fixed_families(name, tmp_path):
    fam = patgen.family(name)
    s = pm.pattern_summary(_write(fam, tmp_path / name))
    K = len(fam["labels"])
    assert s["vertex_count"] == K and s["edge_count"] == 2 * len(fam["pairs"]) and s["diameter"] == fam["diameter"]
    assert s["vertex_data"] == fam["labels"]
    adj = [0] * K
    for a, b in fam["pairs"]:
        adj[a] |= 1 << b
        adj[b] |= 1 << a
    assert s["adj"] == adj
    assert len(s["lines"]) == 5
    for got, (walk, vc) in zip(s["lines"], fam["lines"]):
        assert got["indices"] == walk and got["labels"] == [fam["labels"][t] for t in walk]
        assert (got["C"], got["VC"], got["IL"], got["SV"]) == (len(walk) - 2, vc, 1, 0)
        assert got["enumeration"] == [walk.index(t) for t in walk]


def test_sixteen_vertices_and_positions_are_the_limit(tmp_path):
    chain = patgen.family("chain16_ends")
    s = pm.pattern_summary(_write(chain, tmp_path / "ok"))
    assert s["vertex_count"] == 16 and s["adj"][15] == 1 << 14
    assert all(l["C"] == 14 and len(l["indices"]) == 16 for l in s["lines"])
    ring = patgen.family("ring15_tail")
    s = pm.pattern_summary(_write(ring, tmp_path / "ring"))
    assert s["lines"][0]["enumeration"][-1] == 0 and s["lines"][3]["indices"][0] == 14
    # a 17-position walk (out to t15 and one step back) is refused
    long = list(range(16)) + [14]
    patgen.write_pattern(tmp_path / "long", chain["labels"], chain["pairs"], 15, chain["lines"][:4] + [(long, 0)])
    with pytest.raises(pm.PMError, match="longer than 16 positions"):
        pm.pattern_summary(str(tmp_path / "long"))


@pytest.mark.parametrize("name", FIXED)
@pytest.mark.parametrize("nranks", [1, 3])
def test_oracle_known_answers(name, nranks, tmp_path):
    """Copies plus decoys, no background: every copy survives whole, every decoy passes LCC and falls to the lines
    (so a second iteration runs)."""
    fam = patgen.family(name)
    pat = _write(fam, tmp_path / name)
    copies, decoys = 3, 2
    off, col, labels, _ = patgen.planted_graph(fam, copies, decoys, False, 1)
    so = oracle.run(off, col, pat, str(tmp_path / "out"), labels=labels, nranks=nranks)
    v, e, w = fam["answer"]
    assert (so["final_vertices"], so["final_edges"], so["paths"]) == (v * copies, e * copies, w * copies)
    assert so["iterations"] == 2 and so["terminated"] == 1 and so["nlcc_edges"] > 0
    # without the decoys nothing is removed after superstep 0's label test: one iteration
    off, col, labels, _ = patgen.planted_graph(fam, copies, 0, False, 1)
    s0 = oracle.run(off, col, pat, None, labels=labels, nranks=nranks)
    assert (s0["final_vertices"], s0["iterations"]) == (v * copies, 1)
