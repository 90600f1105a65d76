"""GPU parity on wide templates (tests/patgen.py): up to 16 template vertices, 16-position walks, more than four
relevant label runs next to one label and five template vertices on one label -- the far side of the thresholds
that superstep 0 (build_tiling, k_lcc_first), the packed 16-bit template masks and the walk storage are specialised
on, which no directory under patterns/ reaches.  Every result file and counter against the CPU oracle, bit for bit,
on graphs of about 10^3 vertices: planted copies, decoys that pass LCC and fall to the lines, a sparse background
that uses every label value (so neighbouring pattern runs do not touch), and a hub variant whose planted hub row
(1,100 further neighbours) crosses the light limit, the heavy segment and entry 1024.

Each case first checks the oracle's own statistics (no blow-up, something survives, the lines removed something),
and each single-context case asserts through PatternMatcher.layout_stats() that the tiling selected the
specialisation the family is named for."""
import numpy as np
import pytest

import fuzzypatternmatching_amd as pm
import oracle
import patgen
import pmtest

pytestmark = pytest.mark.gpu

FIXED = ["chain16_ends", "ring15_tail", "fan7", "fan4", "star5"]
VARIANTS = ["plain", "hub"]
COPIES, DECOYS = 5, 3
# graph seeds for which the oracle alone meets _check_oracle (found on the CPU)
GRAPH_SEED = {("fan4", "plain"): 2}
HUB_THRESHOLD = 512  # sharded runs: only the planted hub (about 1,100 entries) is a delegate
# random templates whose planted graph (seed = template seed, hub when seed % 4 == 0) meets _check_oracle
RANDOM_SEEDS = [0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 21, 36]
RANDOM_SHARDED = [0, 7, 12, 36]
TOP_BIT_HOLDERS = {"chain16_ends": 1, "ring15_tail": 1, "fan7": 2, "fan4": 2, "star5": 5}  # per copy
COUNTERS = ("iterations", "terminated", "final_vertices", "final_edges", "lcc_edges", "nlcc_edges", "tds_edges")

_cache = {}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("templates")


def _check_oracle(so):
    assert so["paths"] <= 200000, "the case drifted into blow-up"
    assert so["final_vertices"] > 0, "nothing survives: the case proves nothing"
    assert so["iterations"] >= 2 and so["nlcc_edges"] > 0, "the lines remove nothing"


def _case(workdir, key, nranks=1, thr=pm.DEFAULT_HUB_THRESHOLD, background=True):
    """(pattern dir, off, col, labels, oracle stats, oracle result dir, family) of a fixed family / variant or of a
    random template (key = seed); the graph and each oracle run are computed once per module."""
    gk = (key, background)
    if gk not in _cache:
        if isinstance(key, tuple):
            fam = patgen.family(key[0])
            seed, hub, tag = GRAPH_SEED.get(key, 1), key[1] == "hub", f"{key[0]}_{key[1]}_{int(background)}"
        else:
            fam = patgen.random_template(key)
            seed, hub, tag = key, key % 4 == 0, f"random{key}"
        pat = patgen.write_pattern(workdir / tag / "pattern", fam["labels"], fam["pairs"], fam["diameter"],
                                   fam["lines"])
        off, col, labels, _ = patgen.planted_graph(fam, COPIES, DECOYS, background, seed, hub=hub)
        _cache[gk] = (pat, off, col, labels, fam, tag)
    pat, off, col, labels, fam, tag = _cache[gk]
    ok = (gk, nranks, thr)
    if ok not in _cache:
        out = str(workdir / tag / f"oracle_{nranks}_{thr}")
        so = oracle.run(off, col, pat, out, labels=labels, nranks=nranks, hub_threshold=thr)
        _cache[ok] = (so, out)
    so, out = _cache[ok]
    _check_oracle(so)
    return pat, off, col, labels, so, out, fam


def _compare(so, sg, odir, gdir, nranks):
    print({k: sg[k] for k in COUNTERS + ("walks", "tds_chunks", "exact_lines", "split_lines", "hubs")})
    assert pmtest.compare_result_dirs(odir, str(gdir), nranks) == []
    assert tuple(sg[k] for k in COUNTERS) == tuple(so[k] for k in COUNTERS)
    assert sg["walks"] == so["paths"]


def _check_layout(name, variant, ls):
    """The specialisation the family is named for (a case that ends up in the common path must fail)."""
    print(name, variant, ls)
    if name == "chain16_ends":  # two separate runs next to every label
        assert (ls["k1_wide"], ls["max_nrel"], ls["max_nadm"]) == (0, 2, 2) and ls["phase_a_mask"] & 2
    elif name == "ring15_tail":  # t0: ring neighbours and the tail, three separate runs
        assert (ls["k1_wide"], ls["max_nrel"], ls["max_nadm"]) == (0, 3, 3) and ls["phase_a_mask"] & 4
    elif name == "fan7":  # six separate runs next to the centre: the wide kernel, the full label test everywhere
        assert (ls["k1_wide"], ls["max_nrel"], ls["max_nadm"], ls["phase_a_mask"]) == (1, 6, 6, 8)
    elif name == "fan4":  # three runs that touch merge into one admission compare
        assert (ls["k1_wide"], ls["max_nrel"], ls["max_nadm"], ls["phase_a_mask"]) == (0, 3, 1, 1)
    elif name == "star5":  # five template vertices on one label: the LDS keep_bits loop
        assert ls["max_nkeep"] == 5 and ls["max_nkeep"] > 4 and ls["k1_wide"] == 0
    if variant == "hub":
        assert ls["heavy_rows"] >= 1  # (fan7: k1_heavy_tile of the wide instantiation)


def _bit15(m):
    return int(np.count_nonzero(m.export_state()[0] & 0x8000))


@pytest.mark.parametrize("nranks", [1, 3])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", FIXED)
def test_default_path(name, variant, nranks, workdir, tmp_path):
    """Three searches on one context: from the second on the first later superstep's kernel is chosen from the
    previous search's survivors, so both k_lcc_step instantiations meet the oracle."""
    pat, off, col, labels, so, odir, fam = _case(workdir, (name, variant), nranks)
    m = pm.PatternMatcher(pm.Graph(off, col, True, nranks), pat, labels=labels)
    try:
        _check_layout(name, variant, m.layout_stats())
        for i in range(3):
            _compare(so, m.run_beta(str(tmp_path / f"gpu{i}")), odir, tmp_path / f"gpu{i}", nranks)
        if len(fam["labels"]) == 16:
            assert _bit15(m) >= COPIES  # template bit 15 is set in the final state
    finally:
        m.close()


@pytest.mark.parametrize("name", FIXED)
def test_known_answers(name, workdir, tmp_path):
    """Copies plus decoys without background: every copy survives whole and every decoy is removed by the lines."""
    pat, off, col, labels, so, odir, fam = _case(workdir, (name, "plain"), background=False)
    m = pm.PatternMatcher(pm.Graph(off, col, True, 1), pat, labels=labels)
    try:
        sg = m.run_beta(str(tmp_path / "gpu"))
        _compare(so, sg, odir, tmp_path / "gpu", 1)
        v, e, w = fam["answer"]
        assert (sg["final_vertices"], sg["final_edges"], sg["walks"]) == (v * COPIES, e * COPIES, w * COPIES)
        assert sg["iterations"] == 2
        tpub = m.export_state()[0]
        K = len(fam["labels"])
        # the highest template bit (bit 15 of chain16_ends and ring15_tail) sits on the copies' vertices that can
        # take that role: the leaves that share the last leaf's label, else one vertex per copy
        assert int(np.count_nonzero(tpub & (1 << (K - 1)))) == TOP_BIT_HOLDERS[name] * COPIES
        assert int(np.count_nonzero(tpub >> K)) == 0 and int(np.count_nonzero(tpub)) == v * COPIES
    finally:
        m.close()


def _single_run(name, variant, workdir, tmp_path, nranks=1, searches=1):
    pat, off, col, labels, so, odir, fam = _case(workdir, (name, variant), nranks)
    m = pm.PatternMatcher(pm.Graph(off, col, True, nranks), pat, labels=labels)
    try:
        _check_layout(name, variant, m.layout_stats())
        for i in range(searches):
            sg = m.run_beta(str(tmp_path / f"gpu{i}"))
            _compare(so, sg, odir, tmp_path / f"gpu{i}", nranks)
        sg["long_row_supersteps"] = m.layout_stats()["long_row_supersteps"]
    finally:
        m.close()
    return so, sg


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", FIXED)
def test_exact_path(name, variant, workdir, tmp_path, monkeypatch):
    """PM_FUSED_LINES=0: every line through the per-position k_tp_* / k_tds_* kernels."""
    monkeypatch.setenv("PM_FUSED_LINES", "0")
    so, sg = _single_run(name, variant, workdir, tmp_path)
    assert sg["exact_lines"] >= 5 and sg["tds_chunks"] > 0


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", FIXED)
def test_chunked_tds(name, variant, workdir, tmp_path, monkeypatch):
    """PM_TDS_CAP=3 (61 where the oracle keeps more than 1,000 walks: star5): the fused TDS line overflows its walk
    storage and the exact path enumerates the walk tree in chunks of at most that many walks per level -- fewer than
    the walks the line keeps, so the last level alone takes several chunks."""
    cap = 61 if _case(workdir, (name, variant))[4]["paths"] > 1000 else 3
    monkeypatch.setenv("PM_TDS_CAP", str(cap))
    so, sg = _single_run(name, variant, workdir, tmp_path)
    assert so["paths"] > cap
    assert sg["tds_chunks"] > 1 and sg["tds_chunks"] > so["paths"] // cap


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", FIXED)
def test_pull_long_rows_in_pieces(name, variant, workdir, tmp_path, monkeypatch):
    """PM_PULL_LONG=8: pull-superstep rows above 8 entries are worked in pieces (k_lcc_step_pieces) and packed by
    k_long_pack; two searches (the second runs the pieces launch only where the first listed rows).  The planted
    hub keeps its template neighbours and its valid extra leaves, more than 8 entries, so the hub variant must have
    listed rows; the plain variant's rows may all be shorter."""
    monkeypatch.setenv("PM_PULL_LONG", "8")
    so, sg = _single_run(name, variant, workdir, tmp_path, nranks=3, searches=2)
    print("long-row supersteps", sg["long_row_supersteps"])
    if variant == "hub":
        assert sg["long_row_supersteps"] > 0


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", FIXED)
def test_sharded(name, variant, split, workdir, tmp_path, monkeypatch):
    """Three shards, the planted hub a delegate (split by target owner); PM_SPLIT_LINES=1: every line with a source
    runs split by owner and its effects are exchanged (star5: the wide 64-bit code exchange, 5 bits per label)."""
    if split:
        monkeypatch.setenv("PM_SPLIT_LINES", "1")
    pat, off, col, labels, so, odir, fam = _case(workdir, (name, variant), 3, HUB_THRESHOLD)
    g = pm.Graph(off, col, True, 3, hub_threshold=HUB_THRESHOLD)
    sg = pm.run_beta_local_shards(g, pat, 3, str(tmp_path / "gpu"), labels=labels)
    _compare(so, sg, odir, tmp_path / "gpu", 3)
    assert sg["hubs"] == (1 if variant == "hub" else 0)
    if split:
        assert sg["split_lines"] > 0


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_templates(seed, workdir, tmp_path):
    """Seeded random trees and unicyclic templates of 3..16 vertices with repeated labels."""
    pat, off, col, labels, so, odir, fam = _case(workdir, seed, 2)
    m = pm.PatternMatcher(pm.Graph(off, col, True, 2), pat, labels=labels)
    try:
        print(seed, fam["K"], fam["lines"], m.layout_stats())
        for i in range(2):
            _compare(so, m.run_beta(str(tmp_path / f"gpu{i}")), odir, tmp_path / f"gpu{i}", 2)
    finally:
        m.close()


@pytest.mark.parametrize("seed", RANDOM_SHARDED)
def test_random_templates_sharded(seed, workdir, tmp_path, monkeypatch):
    if seed % 2 == 0:
        monkeypatch.setenv("PM_SPLIT_LINES", "1")
    pat, off, col, labels, so, odir, fam = _case(workdir, seed, 2, HUB_THRESHOLD)
    g = pm.Graph(off, col, True, 2, hub_threshold=HUB_THRESHOLD)
    sg = pm.run_beta_local_shards(g, pat, 3, str(tmp_path / "gpu"), labels=labels)
    _compare(so, sg, odir, tmp_path / "gpu", 2)
    assert sg["hubs"] == (1 if seed % 4 == 0 else 0)
