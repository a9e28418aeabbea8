"""Graphs outside the three synthetic families of cg_mrslam_amd/synth.py (tests/test_topology_cpu.py,
tests/test_topology_gpu.py): dense blocks, forests, stars, trees, fixed-fixed edges, one-pose systems, a self edge and a
component without a fixed vertex -- one per shape of the elimination forest the solver has to get right, each with the
predicate on gn_symbolic_info / gn_front_table that pins the shape.  TEST INFRASTRUCTURE ONLY.

Every graph is built the same way: truth = random poses in a 20 m square, the C2 scan-match information (or full 3x3
information where the case says so), measurements = the true relative poses with noise at that information composed on the
right, initial guess = truth + 0.02 noise on every free vertex.  Deterministic: fixed seeds."""
import numpy as np

from cg_mrslam_amd import synth

TOP_MAX_COLS = 128     # kTopMaxCols (gn_symbolic.h): scalar columns of the top block


def _build(V, ef, et, fixed, seed, full_info=False, shuffle=False):
    rng = np.random.default_rng(seed)
    ef = np.asarray(ef, dtype=np.int32)
    et = np.asarray(et, dtype=np.int32)
    E = len(ef)
    truth = np.stack([rng.uniform(0, 20, V), rng.uniform(0, 20, V), rng.uniform(-np.pi, np.pi, V)], axis=1)
    if full_info:                                 # random axes, eigenvalues log-uniform over 1e1 .. 1e4
        O = np.empty((E, 3, 3))
        for k in range(E):
            Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
            O[k] = Q @ np.diag(10.0 ** rng.uniform(1, 4, 3)) @ Q.T
            O[k] = 0.5 * (O[k] + O[k].T)
        info = np.stack([O[:, 0, 0], O[:, 0, 1], O[:, 0, 2], O[:, 1, 1], O[:, 1, 2], O[:, 2, 2]], axis=1)
        noise = np.einsum("eij,ej->ei", np.linalg.cholesky(np.linalg.inv(O)), rng.standard_normal((E, 3)))
    else:
        info = np.zeros((E, 6))
        info[:, 0], info[:, 3], info[:, 5] = synth.SM_INFO
        noise = rng.standard_normal((E, 3)) / np.sqrt(np.asarray(synth.SM_INFO))
    meas = synth.se2_compose(synth.se2_compose(synth.se2_inverse(truth[ef]), truth[et]), noise)
    if shuffle:
        k = rng.permutation(E)
        ef, et, meas, info = ef[k], et[k], meas[k], info[k]
    fx = np.zeros(V, dtype=np.uint8)
    fx[np.asarray(fixed)] = 1
    poses = truth + 0.02 * rng.standard_normal((V, 3)) * (fx == 0)[:, None]
    poses[:, 2] = synth.normalize_theta(poses[:, 2])
    return dict(truth=truth, poses=poses, fixed=fx, edge_from=np.ascontiguousarray(ef, dtype=np.int32),
                edge_to=np.ascontiguousarray(et, dtype=np.int32), meas=np.ascontiguousarray(meas),
                info=np.ascontiguousarray(info))


def _clique_edges(lo, n):
    i, j = np.triu_indices(n, 1)
    return lo + i, lo + j


def clique60():
    return _build(60, *_clique_edges(0, 60), [0], seed=101)


def clique150_rev():
    """Every edge stored (j, i) with j > i, full information, the edge list shuffled, the last vertex fixed."""
    i, j = _clique_edges(0, 150)
    return _build(150, j, i, [149], seed=102, full_info=True, shuffle=True)


def barbell():
    a, b = _clique_edges(0, 40), _clique_edges(40, 40)
    return _build(80, np.r_[a[0], b[0], 39], np.r_[a[1], b[1], 40], [5], seed=103)


def two_components():
    a, b = _clique_edges(0, 40), _clique_edges(40, 40)
    return _build(80, np.r_[a[0], b[0]], np.r_[a[1], b[1]], [0, 40], seed=104)


def free_component():
    g = two_components()
    g["fixed"] = g["fixed"].copy()
    g["fixed"][40] = 0
    return g


THREE_SIZES = (300, 40, 201)          # chain, clique, star (centre + 200 leaves)


def three_components_labels():
    """vertex -> component (0 chain, 1 clique, 2 star) of three_components_mixed: the ids are a fixed shuffle."""
    return np.random.default_rng(1050).permutation(np.repeat(np.arange(3), THREE_SIZES))


def three_components_mixed():
    lab = three_components_labels()
    ids = [np.flatnonzero(lab == c) for c in range(3)]         # ascending ids of each component, interleaved in 0 .. 540
    chain, clique, star = ids
    ci, cj = _clique_edges(0, 40)
    ef = np.r_[chain[:-1], clique[ci], np.full(200, star[0])]
    et = np.r_[chain[1:], clique[cj], star[1:]]
    return _build(len(lab), ef, et, [chain[150], clique[3], star[7]], seed=105, shuffle=True)


def _star(fixed):
    return _build(3001, np.zeros(3000, np.int32), np.arange(1, 3001), [fixed], seed=106)


def star3000():
    return _star(0)


def star3000_free_centre():
    return _star(17)


def bintree():
    k = np.arange(1, 2047)
    return _build(2047, (k - 1) // 2, k, [0], seed=107)


def bipartite():
    a, b = np.meshgrid(np.arange(30), 30 + np.arange(200), indexing="ij")
    return _build(230, a.ravel(), b.ravel(), [0], seed=108)


def fixed_fixed_edge():
    k = np.arange(299)
    return _build(300, np.r_[k, 0, 0], np.r_[k + 1, 299, 299], [0, 299], seed=109)


def all_neighbours_fixed():
    k = np.arange(4)
    return _build(5, k, k + 1, [0, 2, 4], seed=110)


def self_edge():
    """A 50-chain plus the edge (7, 7); its measurement is not the identity, so its (constant) error is not zero."""
    k = np.arange(49)
    g = _build(50, np.r_[k, 7], np.r_[k + 1, 7], [0], seed=111)
    g["meas"][-1] = [0.3, -0.2, 0.4]
    return g


def shape(g):
    """gn_symbolic_info of the graph, plus what the front table of the host analysis shows of the forest (one row per front:
    first column, columns, border rows, parent, level, children): roots, zero_borders (fronts with a border of zero rows),
    root_levels."""
    from cg_mrslam_amd._lib import gn_front_table, gn_symbolic_info
    a = (len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"])
    info = gn_symbolic_info(*a)
    t = gn_front_table(*a)
    info["roots"] = int(np.sum(t[:, 3] < 0))
    info["zero_borders"] = int(np.sum(t[:, 2] == 0))
    info["root_levels"] = sorted(int(x) for x in t[t[:, 3] < 0, 4])
    info["border_1"] = int(np.sum(t[:, 2] == 1))
    return info


def components(g):
    """Component label of every vertex over the edges between free vertices (fixed vertices cut the graph); -1: fixed."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    V = len(g["poses"])
    ef, et = g["edge_from"], g["edge_to"]
    m = (g["fixed"][ef] == 0) & (g["fixed"][et] == 0)
    A = sp.coo_matrix((np.ones(int(m.sum())), (ef[m], et[m])), shape=(V, V))
    lab = connected_components(A, directed=False)[1].copy()
    lab[g["fixed"] != 0] = -1
    return lab


def _n_components(g):
    return len(np.unique(components(g)[g["fixed"] == 0]))


# name -> (builder, the branch it is there for).  PREDICATES (below) pins each branch and records the measured values.
CASES = {
    "clique60": (clique60, "a dense top block of two fronts, two full fronts below it"),
    "clique150_rev": (clique150_rev, "chain of full fronts, borders of > 100 poses in several work items, full update tiles"),
    "barbell": (barbell, "a one-pose separator between dense subtrees"),
    "two_components": (two_components, "forest: two roots"),
    "three_components_mixed": (three_components_mixed, "forest whose trees differ in height; levels on which a tree has no front"),
    "star3000": (star3000, "every leaf a system of its own (the fixed centre cuts every edge)"),
    "star3000_free_centre": (star3000_free_centre, "one front with thousands of children"),
    "bintree": (bintree, "744 fronts on one level, most with one border pose, under a chain of 34 launch levels"),
    "bipartite": (bipartite, "wide border shared by 200 small fronts"),
    "fixed_fixed_edge": (fixed_fixed_edge, "edges that add to chi2 and to no row of H"),
    "all_neighbours_fixed": (all_neighbours_fixed, "one-pose systems, top block only"),
    "self_edge": (self_edge, "the documented self-edge contribution: chi2 only"),
    "free_component": (free_component, "singular system beside a healthy one"),
}

# the cases whose optimum has zero residual (a tree from one fixed vertex): their final chi2 is rounding
ZERO_RESIDUAL = ("star3000", "star3000_free_centre", "bintree")
# the cases with a solution (free_component is singular)
SOLVED = tuple(n for n in CASES if n != "free_component")

_GRAPHS = {}


def graph(name):
    """The case's graph, built once per process and shared: treat it as read-only."""
    if name not in _GRAPHS:
        _GRAPHS[name] = CASES[name][0]()
    return _GRAPHS[name]


# The analysis depends on the edge list only (fixed vertices are masked numerically), so what a fixed vertex cuts shows in
# the numbers, not in the forest: the predicates on the graph itself say so.  Measured by the host analysis
# (fronts / levels / launch_levels / max_border / max_children / top_block_cols / roots):
PREDICATES = {
    # 4 / 4 / 2 / 44 / 1 / 84 / 1: a chain of four full fronts, the upper two (28 poses, all coupled) are the top block
    "clique60": lambda s, g: (s["fronts"] == s["levels"] >= 4 and s["max_children"] == 1 and s["max_border"] >= 40
                              and s["top_block_fronts"] >= 2 and s["fronts"] - s["top_block_fronts"] >= 2 and s["roots"] == 1),
    # 10 / 10 / 7 / 134 / 1 / 114 / 1
    "clique150_rev": lambda s, g: (s["fronts"] == s["levels"] >= 8 and s["max_border"] >= 100 and s["max_children"] == 1
                                   and bool(np.all(g["edge_from"] > g["edge_to"])) and bool(np.all(g["info"][:, [1, 2, 4]] != 0))),
    # 6 / 4 / 3 / 25 / 2 / 24 / 1: the two cliques' chains of fronts meet in one front
    "barbell": lambda s, g: s["max_children"] == 2 and s["roots"] == 1 and s["fronts"] >= 5 and s["max_border"] >= 24,
    # 6 / 3 / 3 / 24 / 1 / 0 / 2: two roots, both with a border of zero rows, and no top block
    "two_components": lambda s, g: (s["roots"] == 2 and s["zero_borders"] == 2 and s["top_block_fronts"] == 0
                                    and _n_components(g) == 2),
    # 217 / 65 / 4 / 25 / 185 / 123 / 2 (roots on levels 3 and 64: amalgamation puts the star's centre into the clique's
    # chain of fronts, so three components make two trees; the top block is within two poses of kTopMaxCols)
    "three_components_mixed": lambda s, g: (s["roots"] >= 2 and s["root_levels"][0] + 10 < s["root_levels"][-1]
                                            and s["max_children"] > 64 and s["top_block_cols"] > TOP_MAX_COLS - 6
                                            and _n_components(g) == 4),
    # 2986 / 996 / 1 / 1 / 2985 / 3 / 1; the fixed centre cuts every edge: 3000 one-pose systems
    "star3000": lambda s, g: s["max_children"] > 2000 and s["max_border"] == 1 and _n_components(g) == 3000,
    "star3000_free_centre": lambda s, g: s["max_children"] > 2000 and s["max_border"] == 1 and _n_components(g) == 1,
    # 771 / 36 / 34 / 256 / 33 / 96 / 1: 744 fronts on the lowest level, 547 of them with one border pose; amalgamation turns
    # the upper tree into a chain of 16-column fronts with borders of up to 256 poses and up to 33 children each
    "bintree": lambda s, g: (s["fronts"] > 500 and s["border_1"] > 500 and s["launch_levels"] >= 30 and s["max_children"] > 8
                             and s["max_border"] >= 100),
    # 15 / 15 / 12 / 214 / 1 / 114 / 1
    "bipartite": lambda s, g: s["max_border"] >= 200 and s["fronts"] == s["levels"] >= 10,
    # 30 / 4 / 3 / 4 / 5 / 15 / 1
    "fixed_fixed_edge": lambda s, g: int(np.sum((g["fixed"][g["edge_from"]] != 0) & (g["fixed"][g["edge_to"]] != 0))) == 2,
    # 1 / 1 / 0 / 0 / 0 / 15 / 1
    "all_neighbours_fixed": lambda s, g: (s["top_block_fronts"] == s["fronts"] == 1 and _n_components(g) == 2
                                          and not np.any((g["fixed"][g["edge_from"]] == 0) & (g["fixed"][g["edge_to"]] == 0))),
    # 5 / 3 / 1 / 2 / 2 / 72 / 1
    "self_edge": lambda s, g: int(np.sum(g["edge_from"] == g["edge_to"])) == 1 and g["fixed"][7] == 0,
    # as two_components
    "free_component": lambda s, g: (s["roots"] == 2 and _n_components(g) == 2
                                    and int(g["fixed"][:40].sum()) == 1 and int(g["fixed"][40:].sum()) == 0),
}


def assert_branch(name, g):
    """The case reaches the branch it is there for; returns the measured values."""
    s = shape(g)
    assert PREDICATES[name](s, g), (name, s)
    return s
