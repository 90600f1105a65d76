"""Pattern and graph generator for the wide-template parity tests (tests/test_gpu_templates.py,
tests/test_cpu_patgen.py): templates of up to 16 vertices with walks of up to 16 positions, written in the format of
the directories under patterns/, and small graphs with planted copies, decoys and a sparse background.

A template is (labels, pairs, diameter, lines): labels[t] the label of template vertex t, pairs the undirected
template edges, lines a list of (walk, VC) with walk the template indices I[0..C+1].  Lines 0..3 are path / cycle
token passing, lines >= 4 template-driven search (oracle/pm_oracle.cpp nlcc_path / tds):

  * a VC = 0 path line only has sources whose T holds both I[0] and I.back(), so its first and last label are equal;
  * on lines 0..3 every interior label occurs once in the walk (the per-(vertex, source) token dedup makes the
    reference order-dependent otherwise);
  * E[k] is the position of the first occurrence of I[k] in the walk (0 at the end of a VC = 1 line).

Everything is a pure function of its arguments: numpy.random.default_rng(seed) only."""
import os

import numpy as np

import pmtest

MAX_WALK = 16  # the loader accepts C + 2 <= 16 walk positions


def enumeration(walk):
    return [walk.index(t) for t in walk]


def write_pattern(dir, labels, pairs, diameter, lines):
    """Writes <dir>/0/pattern_{edge,edge_data,vertex,vertex_data,stat,nlc,non_local_constraint}; returns dir."""
    d = os.path.join(os.fspath(dir), "0")
    os.makedirs(d, exist_ok=True)
    eid = {}
    for a, b in pairs:
        eid.setdefault((min(a, b), max(a, b)), len(eid))
    directed = sorted({(a, b) for a, b in pairs} | {(b, a) for a, b in pairs})
    files = {
        "pattern_edge": [f"{s} {t}" for s, t in directed],
        "pattern_edge_data": [f"{s} {t} {eid[(min(s, t), max(s, t))]} 55" for s, t in directed],
        "pattern_vertex": [""],
        "pattern_vertex_data": [f"{t} {int(l)}" for t, l in enumerate(labels)],
        "pattern_stat": [f"diameter : {diameter}"],
        "pattern_nlc": [],
        "pattern_non_local_constraint": [],
    }
    for pl, (walk, vc) in enumerate(lines):
        walk = [int(t) for t in walk]
        L = " ".join(str(int(labels[t])) for t in walk)
        I = " ".join(map(str, walk))
        E = " ".join(map(str, enumeration(walk)))
        agg = " ".join(["0"] * len(walk) if pl < 4 else ["0"] + ["1"] * (len(walk) - 1))
        files["pattern_nlc"].append(f"{L} : {I} : {len(walk) - 2} : {int(vc)} : 1 : 0")
        files["pattern_non_local_constraint"].append(f"{I} : {E} : {agg}")
    for name, ls in files.items():
        with open(os.path.join(d, name), "w") as f:
            f.write("".join(l + "\n" for l in ls))
    return os.fspath(dir)


# ---------------------------------------------------------------------------------------------------------------
# The fixed families.  Pattern labels are odd, so a background that uses every value puts other vertices between
# neighbouring pattern runs of the label-major order (no two relevant runs touch: nadm = nrel); fan4 is the gapless
# counterpart (consecutive labels: its centre's three relevant runs merge into one).
#
# Each entry: labels, pairs, diameter, lines, decoy = (labels, pairs) of a graph that passes LCC and falls to the
# lines, hub = the template vertex of highest degree, hub_leaf = a template neighbour of it (the label of the hub
# copy's hub_valid valid extra leaves: at most 8, and enough that the hub keeps more than 8 entries after superstep
# 0 -- star5 takes 4, each further leaf multiplies its walks), answer = (final_vertices, final_edges, walks) per
# planted copy.

def _chain16_ends():
    labels = [1] + [3 + 2 * i for i in range(14)] + [1]
    pairs = [(i, i + 1) for i in range(15)]
    fwd, rev = list(range(16)), list(range(15, -1, -1))
    # decoy: the interior t1..t14 closed to a 15-ring by one vertex with the end label
    dl = [1] + labels[1:15]
    dp = [(i, i + 1) for i in range(14)] + [(14, 0)]
    return dict(labels=labels, pairs=pairs, diameter=15,
                lines=[(fwd, 0), (rev, 0), (fwd, 0), (rev, 0), (fwd, 0)],
                decoy=(dl, dp), hub=7, hub_leaf=8, hub_valid=8, answer=(16, 30, 1))


def _ring15_tail():
    labels = [1 + 2 * i for i in range(16)]
    pairs = [(i, (i + 1) % 15) for i in range(15)] + [(0, 15)]
    cyc = lambda s: [(s + i) % 15 for i in range(15)] + [s]
    # decoy: a 30-ring carrying the ring labels twice round, a tail on both vertices with t0's label
    dl = labels[:15] * 2 + [labels[15]] * 2
    dp = [(i, (i + 1) % 30) for i in range(30)] + [(0, 30), (15, 31)]
    return dict(labels=labels, pairs=pairs, diameter=8,
                lines=[(cyc(0), 1), (cyc(5), 1), (cyc(10), 1), (cyc(14), 1), (cyc(0), 1)],
                decoy=(dl, dp), hub=0, hub_leaf=15, hub_valid=8, answer=(16, 32, 1))


def _fan(nleaf, labels):
    pairs = [(0, i) for i in range(1, nleaf + 1)]
    a, b = [1, 0, nleaf], [nleaf, 0, 1]
    tds = [1]
    for i in range(2, nleaf + 1):
        tds += [0, i]
    # decoy: the fan without its last leaf (the leaf that shares t1's label)
    return dict(labels=labels, pairs=pairs, diameter=2, lines=[(a, 0), (b, 0), (a, 0), (b, 0), (tds, 0)],
                decoy=(labels[:nleaf], pairs[:nleaf - 1]), hub=0, hub_leaf=2, hub_valid=8,
                answer=(nleaf + 1, 2 * nleaf, 2))


def _fan7():
    return _fan(7, [1, 3, 5, 7, 9, 11, 13, 3])


def _fan4():
    return _fan(4, [10, 11, 12, 13, 11])


def _star5():
    labels = [1, 3, 3, 3, 3, 3]
    pairs = [(0, i) for i in range(1, 6)]
    tds = [1, 0, 2, 0, 3, 0, 4, 0, 5]
    return dict(labels=labels, pairs=pairs, diameter=2,
                lines=[([1, 0, 2], 0), ([2, 0, 3], 0), ([3, 0, 4], 0), ([4, 0, 5], 0), (tds, 0)],
                decoy=(labels[:5], pairs[:4]), hub=0, hub_leaf=1, hub_valid=4, answer=(6, 10, 120))


FAMILIES = {"chain16_ends": _chain16_ends, "ring15_tail": _ring15_tail, "fan7": _fan7, "fan4": _fan4,
            "star5": _star5}


def family(name):
    return FAMILIES[name]()


# ---------------------------------------------------------------------------------------------------------------
# Seeded random templates

def _tree_path(adj, a, b):
    prev = {a: None}
    todo = [a]
    while todo:
        u = todo.pop()
        for w in adj[u]:
            if w not in prev:
                prev[w] = u
                todo.append(w)
    out = [b]
    while out[-1] != a:
        out.append(prev[out[-1]])
    return out[::-1]


def lines_ok(labels, lines):
    """The rules of the module docstring for lines 0..3 (and the walk length for every line)."""
    for pl, (walk, vc) in enumerate(lines):
        if not 3 <= len(walk) <= MAX_WALK:
            return False
        if pl >= 4:
            continue
        ls = [labels[t] for t in walk]
        if ls[0] != ls[-1] or (vc and walk[0] != walk[-1]) or (not vc and walk[0] == walk[-1]):
            return False
        if any(ls.count(x) != 1 for x in ls[1:-1]):
            return False
    return True


def _diameter(adj, K):
    best = 0
    for s in range(K):
        dist = {s: 0}
        todo = [s]
        for u in todo:
            for w in adj[u]:
                if w not in dist:
                    dist[w] = dist[u] + 1
                    todo.append(w)
        best = max(best, max(dist.values()))
    return best


def random_template(seed):
    """A random tree or unicyclic template of K in [2, 16] vertices with random labels (repetition allowed), four
    path / cycle lines derived from it and one depth-first TDS walk; redrawn (K included) until a legal line 0..3
    of at least three positions exists, so K = 2 never survives.  Same keys as family()."""
    rng = np.random.default_rng(seed)
    while True:
        K = int(rng.integers(2, 17))
        parent = [int(rng.integers(0, t)) for t in range(1, K)]
        pairs = [(parent[t - 1], t) for t in range(1, K)]
        adj = [[] for _ in range(K)]
        for a, b in pairs:
            adj[a].append(b)
            adj[b].append(a)
        cycle = None
        if K >= 3 and rng.integers(0, 2):
            a = int(rng.integers(0, K))
            far = [b for b in range(K) if b != a and b not in adj[a]]
            if far:
                b = far[int(rng.integers(0, len(far)))]
                cycle = _tree_path(adj, a, b)  # closed by the extra edge (b, a)
        nlab = int(rng.integers(max(2, (K + 1) // 2), K + 1))
        alphabet = 1 + 2 * rng.permutation(16)[:nlab]
        labels = [int(alphabet[int(rng.integers(0, nlab))]) for _ in range(K)]
        cand = []
        for a in range(K):  # path lines between equal-label template vertices, both directions
            for b in range(K):
                if a != b and labels[a] == labels[b]:
                    w = _tree_path(adj, a, b)
                    if lines_ok(labels, [(w, 0)]):
                        cand.append((w, 0))
        if cycle is not None and len(cycle) + 1 <= MAX_WALK and len(set(labels[t] for t in cycle)) == len(cycle):
            for s in range(len(cycle)):
                cand.append((cycle[s:] + cycle[:s] + [cycle[s]], 1))
        if not cand:
            continue
        order = rng.permutation(len(cand))
        lines = [cand[int(order[i % len(cand)])] for i in range(4)]
        # line 4: depth-first walk over the tree edges from a random root, cut at 16 positions and back to the last
        # first visit (a walk that ends on a revisit of its source has no legal end)
        root = int(rng.integers(0, K))
        walk, seen = [], set()

        def dfs(u):
            walk.append(u)
            seen.add(u)
            for w in adj[u]:
                if w not in seen:
                    dfs(w)
                    walk.append(u)

        dfs(root)
        walk = walk[:MAX_WALK]
        while walk.index(walk[-1]) != len(walk) - 1:
            walk.pop()
        if len(walk) < 3:
            continue
        if cycle is not None:
            pairs.append((cycle[-1], cycle[0]))
            adj[cycle[-1]].append(cycle[0])
            adj[cycle[0]].append(cycle[-1])
        lines.append((walk, 0))
        # decoy: a copy folded so that LCC keeps it and line 0 does not -- a path line's two end vertices merged into
        # one, or a cycle line's cycle doubled (two copies, the closing edges crossed)
        w0, vc0 = lines[0]
        if vc0:
            u, v = w0[0], w0[1]
            cut = {(u, v), (v, u)}
            dp = [(a, b) for a, b in pairs if (a, b) not in cut]
            dp = dp + [(a + K, b + K) for a, b in dp] + [(u, v + K), (u + K, v)]
            dl = labels + labels
        else:
            a, b = w0[0], w0[-1]
            ren = lambda t: a if t == b else (t if t < b else t - 1)
            dp = sorted({(min(ren(x), ren(y)), max(ren(x), ren(y))) for x, y in pairs})
            dl = [l for t, l in enumerate(labels) if t != b]
        deg = [len(x) for x in adj]
        hub = int(np.argmax(deg))
        return dict(labels=labels, pairs=pairs, diameter=_diameter(adj, K), lines=lines, decoy=(dl, dp), hub=hub,
                    hub_leaf=adj[hub][0], hub_valid=8, answer=None, K=K)


# ---------------------------------------------------------------------------------------------------------------
# Graphs

HUB_EXTRA = 1100  # further neighbours of the hub copy's hub: past the 480-entry light limit, the 512-entry heavy
                  # segment and entry 1024
BACKGROUND_VERTICES = 600
BACKGROUND_EDGES = 2500


def planted_graph(fam, copies, decoys, background, seed, hub=False):
    """`copies` copies of the family's template and `decoys` of its decoy; background: 600 more vertices with labels
    drawn from every value from 0 to the largest pattern label + 1 and 2,500 uniformly random edges over all
    vertices; hub: one more copy whose fam["hub"] vertex gets HUB_EXTRA further neighbours, fam["hub_valid"] with
    fam["hub_leaf"]'s label, the others with labels the template does not put next to the hub (superstep 0 drops
    them).  Vertex ids are shuffled.  Returns (off, col, labels, hub vertex id or None)."""
    rng = np.random.default_rng(seed)
    tl, tp = fam["labels"], fam["pairs"]
    labels, pairs = [], []

    def add(ls, ps):
        base = len(labels)
        labels.extend(int(x) for x in ls)
        pairs.extend((base + a, base + b) for a, b in ps)
        return base

    for _ in range(copies):
        add(tl, tp)
    for _ in range(decoys):
        add(*fam["decoy"])
    top = max(tl) + 1
    hub_v = None
    if hub:
        hub_v = add(tl, tp) + fam["hub"]
        near = {tl[b] if a == fam["hub"] else tl[a] for a, b in tp if fam["hub"] in (a, b)}
        other = np.array([x for x in range(top + 1) if x not in near])
        for i in range(HUB_EXTRA):
            lab = tl[fam["hub_leaf"]] if i < fam["hub_valid"] else int(other[int(rng.integers(0, len(other)))])
            pairs.append((hub_v, add([lab], [])))
    if background:
        labels.extend(int(x) for x in rng.integers(0, top + 1, BACKGROUND_VERTICES))
        n = len(labels)
        for a, b in rng.integers(0, n, (BACKGROUND_EDGES, 2)):
            if a != b:
                pairs.append((int(a), int(b)))
    n = len(labels)
    perm = rng.permutation(n)
    lab = np.zeros(n, np.uint64)
    lab[perm] = np.array(labels, np.uint64)
    off, col = pmtest.symmetric_csr([(int(perm[a]), int(perm[b])) for a, b in pairs], n)
    return off, col, lab, None if hub_v is None else int(perm[hub_v])
