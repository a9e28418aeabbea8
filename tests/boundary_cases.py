"""Sweeps of one integer knob each across the solver's tile, chunk, child-count and list-length constants
(tests/test_boundary_cpu.py, tests/test_boundary_gpu.py).  tests/topology_cases.py samples shapes; these families step a front's
border, the top block's width, a front's child count, one assembly list's length and the number of assembly keys through every
value around the constant, so that a front lands one below, exactly on and one above it.  TEST INFRASTRUCTURE ONLY.

Every graph is built by topology_cases._build (random truth, the C2 scan-match information, noisy true relative poses, a 0.02
perturbation of every free vertex), deterministic by its seed.  The analysis depends on the edge list only (fixed vertices are
masked numerically), so every vertex with an edge has a block column.

The families (front = (own poses nc, border poses ns); measured by the host analysis, pinned by tests/test_boundary_cpu.py):
  clique(n), n = 2 .. 71: up to n = 42 the top block alone (3 n = 6 .. 126 columns: every 16-column tile edge, one pose short of
      kTopMaxCols = 128); from n = 43 a chain of fronts (16, n - 16), (16, n - 32), .. under it, two launch levels from n = 59
  blobs(b, 16, 4), b = 1 .. 54: a separator clique of b poses that carries four 16-pose cliques, each joined to every separator
      pose: four leaves (16, b) up to b = 48 -- the border of a level of leaves across 31 | 32 poses (kLeafChunkRows = 95 rows) and
      from b = 49 the analysis chains the fronts instead, borders of 53 | 54 poses among them (kChunkRows = 159 rows)
  forest(k, n), k in {2, 9}, n = 17 .. 64: k disjoint copies of clique(n), a fixed vertex each: no top block, level 1 holds k
      fronts (16, n - 32): borders of 1 .. 32 poses above the leaves, on a level of two fronts (kTopChunkRows = 31 rows) and of
      nine (kMidChunkRows = 79 rows)
  fan(m) = blobs(6, 20, m), m = 2 .. 10, 31 .. 34, 63 .. 66: the top front has exactly m children; fan2(m), two disjoint copies:
      from m = 8 their roots are amalgamated into one front with 2 m children (below: two roots, no top block);
      fanlow(m) = blobs(44, 16, m), m = 7 .. 10: the separator's lowest front lies below the top block and has the m children
  star(k): a free centre with k leaves, one leaf fixed: the centre's diagonal block has an assembly list of k entries;
      dup(d): one edge repeated d times: three lists of d entries
  chain(V), ring(V) = the chain plus the closure (0, V - 1): 2 V - 1 and 2 V assembly keys, V = 2047 .. 2050 and 32767 .. 32770:
      every residue mod 4 on either side of 4096 (one tile of k_asm_scan) and of 65 536 (one round of its outer loop)

Measured on an MI355X (tests/test_boundary_gpu.py): see MEASURED below; the device-built structure equals the host's on every case."""
import numpy as np

import topology_cases as T

# family -> (largest backward error of a Gauss-Newton step in u = 2^-53 (bar: 120 u), largest error of a marginal block of
# marginals_all / marginals against the dense inverse, of a joint block (bar: 1e-9 both); None: not checked for the family) as
# tests/test_boundary_gpu.py printed them on an MI355X.  "0.0 u" is below the allowance for the rounding of the pose update.
MEASURED = {
    "clique": (0.0, 2.25e-14, 8.25e-15),       # marginals: clique_55, joint: clique_62 with 17 vertices
    "blobs": (0.0, 2.69e-14, 2.32e-14),        # blobs_40, blobs_29 with 17
    "forest2": (0.0, 2.43e-14, 5.48e-15),      # forest2_59, forest2_25 with 17
    "forest9": (0.0, 5.92e-15, 8.67e-15),      # forest9_29 (17 cases of up to 300 vertices), forest9_37 with 17
    "fan": (0.0, 2.33e-14, None),              # fan_7 (15 cases of up to 300 vertices)
    "star": (0.0, None, None),
    "dup": (0.0, None, None),
    "chain": (2.5, None, None),                # chain_32768
}

LEAF_CHUNK, MID_CHUNK, TOP_CHUNK, TOP_CHUNK_FRONTS, CHUNK_ROWS = 95, 79, 31, 8, 159     # gn_symbolic.h
TOP_MAX_COLS = T.TOP_MAX_COLS
WORK_CHILDREN, TOP_PRE, CHILD_ROUND = 8, 32, 64      # gn_symbolic.h kWorkChildren, gn_kernels.hip kTopPre, marginals_kernels.hip
UPDATE_TILE, SELINV_TILE = 32, 64                    # rows of an update tile (gn_kernels.hip), of a selected-inversion row tile
LIST_EDGES = (4, 8, 16, 256, 1024)                   # gn_structure.hip: registers 4 / 8 / 16, a wavefront up to 256, 1024-entry tiles
SCAN_EDGES = (4096, 65536)                           # gn_structure.hip: one tile / one round of k_asm_scan


def _seed(*k):
    return int(np.random.SeedSequence([7919, *k]).generate_state(1)[0])


def _blob_edges(b, c, m, lo=0):
    """Separator lo .. lo + b - 1, blob j at lo + b + j c."""
    i, k = T._clique_edges(lo, b)
    ef, et = [i], [k]
    for j in range(m):
        o = lo + b + j * c
        i, k = T._clique_edges(o, c)
        s, q = np.meshgrid(lo + np.arange(b), o + np.arange(c), indexing="ij")
        ef += [i, s.ravel()]
        et += [k, q.ravel()]
    return np.concatenate(ef), np.concatenate(et)


def clique(n):
    return T._build(n, *T._clique_edges(0, n), [0], seed=_seed(1, n))


def blobs(b, c=16, m=4, copies=1):
    V1 = b + m * c
    parts = [_blob_edges(b, c, m, lo=k * V1) for k in range(copies)]
    return T._build(copies * V1, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
                    [k * V1 for k in range(copies)], seed=_seed(2, b, c, m, copies))


def forest(k, n):
    parts = [T._clique_edges(c * n, n) for c in range(k)]
    return T._build(k * n, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
                    [c * n for c in range(k)], seed=_seed(3, k, n))


def fan(m, copies=1):
    return blobs(6, 20, m, copies)


def star(k):
    return T._build(k + 1, np.zeros(k, np.int32), np.arange(1, k + 1), [1], seed=_seed(4, k))


def dup(d):
    return T._build(2, np.zeros(d, np.int32), np.ones(d, np.int32), [0], seed=_seed(5, d))


def chain(V, closed=False):
    k = np.arange(V - 1)
    ef, et = (np.r_[k, 0], np.r_[k + 1, V - 1]) if closed else (k, k + 1)
    return T._build(V, ef, et, [0], seed=_seed(6, V, int(closed)))


FAN_M = (*range(2, 11), *range(31, 35), *range(63, 67))
FAN2_M = (4, 5, 8, 9, 16, 17, 32, 33, 64, 65)
FANLOW_M = (7, 8, 9, 10)
STAR_K = (*range(1, 21), *range(63, 67), *range(255, 259), *range(1023, 1027))
DUP_D = (3, 4, 5, 8, 9, 16, 17)
CHAIN_V = (2047, 2048, 2049, 2050, 32767, 32768, 32769, 32770)

# family -> {case name: builder}
FAMILIES = {
    "clique": {f"clique_{n}": (lambda n=n: clique(n)) for n in range(2, 72)},
    "blobs": {f"blobs_{b}": (lambda b=b: blobs(b)) for b in range(1, 55)},
    "forest2": {f"forest2_{n}": (lambda n=n: forest(2, n)) for n in range(17, 65)},
    "forest9": {f"forest9_{n}": (lambda n=n: forest(9, n)) for n in range(17, 65)},
    "fan": {**{f"fan_{m}": (lambda m=m: fan(m)) for m in FAN_M}, **{f"fan2_{m}": (lambda m=m: fan(m, 2)) for m in FAN2_M},
            **{f"fanlow_{m}": (lambda m=m: blobs(44, 16, m)) for m in FANLOW_M}},
    "star": {f"star_{k}": (lambda k=k: star(k)) for k in STAR_K},
    "dup": {f"dup_{d}": (lambda d=d: dup(d)) for d in DUP_D},
    "chain": {**{f"chain_{V}": (lambda V=V: chain(V)) for V in CHAIN_V}, **{f"ring_{V}": (lambda V=V: chain(V, True)) for V in CHAIN_V}},
}
CASES = {name: b for fam in FAMILIES.values() for name, b in fam.items()}
FAMILY_OF = {name: fam for fam, cases in FAMILIES.items() for name in cases}
# structure equality plus one Gauss-Newton step is the whole check of these
STRUCTURE_ONLY = ("star", "dup", "chain")
DENSE_UP_TO = 300
# Levenberg-Marquardt and dogleg traces: either side of kTopMaxCols and of the leaf chunk
TRACE_CASES = ("clique_42", "clique_43", "blobs_31", "blobs_32")

# cases on which the C oracle's own step misses reference_cases.OMEGA_MAX (tests/test_boundary_cpu.py re-measures it): no
# valid case for the backward-error check, which they are left out of -- the bar stays
NO_STEP_CHECK = ()

_GRAPHS = {}
_SHAPES = {}


def graph(name):
    """The case's graph, built once per process and shared: treat it as read-only."""
    if name not in _GRAPHS:
        _GRAPHS[name] = CASES[name]()
    return _GRAPHS[name]


def level_chunks(t, top, n_levels):
    """Border rows per work item of every launch level, by the rule of gn_upload (gn_host.cpp): kLeafChunkRows on a level of
    leaves, else kMidChunkRows, kTopChunkRows where the level has at most kTopChunkFronts fronts (the top block's left out)."""
    out = []
    for l in range(n_levels):
        on = [f for f in range(len(t)) if t[f, 4] == l and f not in top]
        leaf = all(t[f, 5] == 0 for f in on)
        out.append(LEAF_CHUNK if leaf else TOP_CHUNK if len(on) <= TOP_CHUNK_FRONTS else MID_CHUNK)
    return out


def shape(name):
    """What the host analysis makes of the case, in the terms the boundaries are stated in:
    info (gn_symbolic_info), table (gn_front_table), top (fronts of the top block), chunk (rows per work item of each launch
    level), role -> set of border rows 3 ns of the fronts in that role ('leaf' / 'mid' / 'upper': factored on a level with that
    chunk length; 'factor': any front outside the top block; 'any': every front), children_factor (child counts of the fronts outside the top
    block), children_top (fronts outside the top block whose parent is inside), children_any, keys (nf + nb), longest_list."""
    if name in _SHAPES:
        return _SHAPES[name]
    from cg_mrslam_amd import load_library
    from cg_mrslam_amd._lib import gn_front_table, gn_symbolic_info
    from test_gn_gpu import _asm_lists
    g = graph(name)
    a = (len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"])
    info = gn_symbolic_info(*a)
    t = gn_front_table(*a)
    top, f = set(), len(t) - 1
    for _ in range(info["top_block_fronts"]):               # the last fronts of the root's chain, consecutive columns
        top.add(f)
        nxt = [c for c in range(len(t)) if t[c, 3] == f and t[c, 0] + t[c, 1] == t[f, 0] and t[c, 4] == t[f, 4] - 1]
        f = nxt[0] if nxt else -1
    chunk = level_chunks(t, top, info["launch_levels"])
    role = {"leaf": set(), "mid": set(), "upper": set(), "factor": set(), "any": {3 * int(x) for x in t[:, 2]}}
    names = {LEAF_CHUNK: "leaf", MID_CHUNK: "mid", TOP_CHUNK: "upper"}
    for f in range(len(t)):
        if f in top:
            continue
        role["factor"].add(3 * int(t[f, 2]))
        role[names[chunk[t[f, 4]]]].add(3 * int(t[f, 2]))
    ptr, _ = _asm_lists(load_library(), None, *a[:1], *a[2:])
    s = dict(info=info, table=t, top=top, chunk=chunk, role=role,
             children_factor={int(t[f, 5]) for f in range(len(t)) if f not in top},
             children_top=sum(1 for f in range(len(t)) if f not in top and t[f, 3] in top) if top else None,
             children_any={int(x) for x in t[:, 5]}, keys=len(ptr) - 1, longest_list=int(np.diff(ptr).max()))
    _SHAPES[name] = s
    return s
