"""The solver away from the information scale and the units of the synthetic recipes (tests/test_scale_cpu.py proves the
references and measures the bars; tests/test_scale_gpu.py runs the device).  TEST INFRASTRUCTURE ONLY.

Every other graph of the suite is weighted with synth.SM_INFO / ODOM_INFO (or eigenvalues over three decades) and lies within a
few tens of metres of the origin.  Here the smallest graphs that still reach every kernel role (CASES) are re-weighted and
re-scaled by ``rescale`` (FAMILIES), and every quantity the device returns is held, per block by the block's own norm, to

    e_dev <= max(the quantity's existing bar, 10 e_ref)

e_dev: the device's error against the truth T (SuperLU, three refinements with the residual in long double; labels and the
       stars' inverses in long double);
e_ref: the error of the plain float64 path (unrefined SuperLU step, np.linalg.inv blocks, the labels computed from them)
against the same T, measured on the CPU and recorded in MEASURED; a (case, family, quantity) is valid only where T's own error
estimate (its last correction, carried through the same formulas) is at most e_ref / 100 (``valid``).

The families:
  identity          the control: the base graph's own arrays
  edge_spread       each edge's Omega times 10^U(-2, 2)
  component_spread  diagonal Omega, each of the three entries 10^U(1, 5)
  full_spread       random axes, eigenvalues 10^U(1, 5)
  heading_stiff     the heading weighted 1e6 times more: Omega_tt x 1e6 and, so that a full Omega stays positive definite, the
                    xy-theta entries x 1e3 (the congruence diag(1, 1, 1e3); on a diagonal Omega exactly Omega_tt x 1e6)
  heading_soft      the same with 1e-3 (the congruence diag(1, 1, 10^-1.5))
  millimetres       positions and translational measurements x 1000, Omega's xy block x 1e-6, its xy-theta entries x 1e-3
  far_origin        every position + 1e6 m; the relative measurements stay, a prior's (absolute) position moves along
  weak, strong      all Omega x 2^-40, x 2^40: H and b scale exactly, dx is unchanged in exact and in float64 arithmetic

The vertex-removal stars take no positions: far_origin leaves their input as it is (the call must give identity's bytes)."""
import numpy as np

import boundary_cases as B
import ref_numpy as R
import ref_robust_marginals as RM
import ref_typed as RT
import remove_nodes_cases as K
import typed_cases as TC
from cg_mrslam_amd import synth

FAMILIES = ("identity", "edge_spread", "component_spread", "full_spread", "heading_stiff", "heading_soft", "millimetres",
            "far_origin", "weak", "strong")
SEED = 20

# name -> (kind, builder).  pose: pose-pose edges only; typed: points and priors; star: one removed vertex
CASES = {
    "clique40": ("pose", lambda: B.clique(40)),                       # the top block alone, 120 columns
    "blobs20": ("pose", lambda: B.blobs(20)),                         # four leaves under a top block: L21, update tiles, Z, the chain
    "forest2_40": ("pose", lambda: B.forest(2, 40)),                  # no top block, two launch levels
    "pg300": ("pose", lambda: synth.make_pose_graph(300, 900, seed=3)),   # a many-level tree
    "leaf_and_hub": ("typed", TC.leaf_and_hub),
    "mixed257": ("typed", lambda: TC.mixed(257, 3)),
    "star5": ("star", lambda: K.star(5, 104)),
    "star16": ("star", lambda: K.star(16, 116)),
}
# the condensed graph fixes the gauge alone: on the forest that leaves a component without a fixed vertex
CONDENSED = ("clique40", "blobs20", "pg300")
PAIRS = [(c, f) for c in CASES for f in FAMILIES]
# where the reference's condensed tree is decided by less than condense_tree_cases.MARGIN_MIN (heading_stiff leaves the cliques'
# pair weights, uniform information throughout, 3e-9 and 5e-8 nats apart): the device's tree is held to the minimum total weight
# on the reference's weights instead of to the reference's edges, as tests/test_condense_tree_gpu.py does at 300 queries
TREE_TIED = (("clique40", "heading_stiff"), ("blobs20", "heading_stiff"))

# (case, family) -> the half-width in decades the family is narrowed to for the case: at the full width the truth's own error
# estimate exceeds e_ref / 100 (tests/test_scale_cpu.py: pg300 under edge_spread over four decades, cond_2(H) 1.2e11, blocks of
# np.linalg.inv off by 1.7e-9, the truth's last correction 3.7e-11)
# star16 under component_spread: cond_2(H) of the local star 2.6e5, the long double truth's two evaluation orders 3.2e-14 apart, the
# float64 reference off by 1.1e-12.
NARROWED = {("pg300", "edge_spread"): 1.5, ("star16", "component_spread"): 1.5}

REFINEMENTS = 3     # of the truth (ref_numpy._refine_solve; the suite's other references take two)

_BASE, _SCALED = {}, {}


def base(name):
    """The base graph as a dict, built once (read-only).  A star: nV, edge_from, edge_to, meas, info, remove."""
    if name not in _BASE:
        kind, mk = CASES[name]
        g = mk()
        if kind == "star":
            g = dict(zip(("nV", "edge_from", "edge_to", "meas", "info", "remove"), g))
        _BASE[name] = g
    return _BASE[name]


def _upper(O):
    return np.stack([O[:, 0, 0], O[:, 0, 1], O[:, 0, 2], O[:, 1, 1], O[:, 1, 2], O[:, 2, 2]], axis=1)


def _heading(info, f):
    """The congruence diag(1, 1, sqrt(f)) of every Omega: Omega_tt x f, the xy-theta entries x sqrt(f)."""
    out = info.copy()
    out[:, [2, 4]] *= np.sqrt(f)
    out[:, 5] *= f
    return out


def rescale(graph, family, seed=SEED, width=2.0):
    """The graph re-weighted / re-scaled by ``family``: a new dict, the arrays that do not change shared with ``graph``.
    Deterministic in (family, seed).  width: the half-width in decades of the three spread families (NARROWED)."""
    g = dict(graph)
    E = len(g["edge_from"])
    rng = np.random.default_rng([seed, FAMILIES.index(family)])
    info = g["info"]
    if family == "identity":
        pass
    elif family == "edge_spread":
        g["info"] = info * (10.0 ** rng.uniform(-width, width, E))[:, None]
    elif family == "component_spread":
        d = 10.0 ** rng.uniform(3 - width, 3 + width, (E, 3))
        g["info"] = np.stack([d[:, 0], 0 * d[:, 0], 0 * d[:, 0], d[:, 1], 0 * d[:, 0], d[:, 2]], axis=1)
    elif family == "full_spread":
        O = np.empty((E, 3, 3))
        for k in range(E):
            Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
            O[k] = Q @ np.diag(10.0 ** rng.uniform(3 - width, 3 + width, 3)) @ Q.T
            O[k] = 0.5 * (O[k] + O[k].T)
        g["info"] = _upper(O)
    elif family == "heading_stiff":
        g["info"] = _heading(info, 1e6)
    elif family == "heading_soft":
        g["info"] = _heading(info, 1e-3)
    elif family == "millimetres":
        g["meas"] = g["meas"] * np.array([1000.0, 1000.0, 1.0])
        g["info"] = info * np.array([1e-6, 1e-6, 1e-3, 1e-6, 1e-3, 1.0])
        if "poses" in g:
            g["poses"] = g["poses"] * np.array([1000.0, 1000.0, 1.0])
    elif family == "far_origin":
        if "poses" in g:
            g["poses"] = g["poses"] + np.array([1e6, 1e6, 0.0])
            if "ek" in g:                                          # a prior measures a position, not a difference
                prior = g["ek"] >= 3
                g["meas"] = g["meas"] + prior[:, None] * np.array([1e6, 1e6, 0.0])
    elif family == "weak":
        g["info"] = info * 2.0 ** -40
    elif family == "strong":
        g["info"] = info * 2.0 ** 40
    else:
        raise KeyError(family)
    return g


def graph(name, family):
    """The rescaled case, built once and shared: read-only."""
    if (name, family) not in _SCALED:
        _SCALED[(name, family)] = rescale(base(name), family, width=NARROWED.get((name, family), 2.0))
    return _SCALED[(name, family)]


def args(g):
    return tuple(g[k] for k in ("poses", "fixed", "edge_from", "edge_to", "meas", "info"))


def kinds(g):
    return g.get("vk"), g.get("ek")


# ------------------------------------------------------------------------------------------------ truth and the plain path
class Solved:
    """H, b and the layout of the system at ``poses`` (ref_typed.build_system: pose graphs and typed ones alike) with
      dx, dx_err    the refined solve of H dx = b and its last correction (the truth T and its own error estimate)
      inv, inv_err  the refined H^-1, every column, and its last correction
      dx_plain      the step the float64 reference takes (ref_typed.gn_optimize: unrefined SuperLU, the poses updated and
                    the step read back off them, as the device's is)
      inv_plain     np.linalg.inv of the dense H."""

    def __init__(self, poses, fixed, ef, et, meas, info, vk=None, ek=None):
        import scipy.sparse.linalg as spla
        self.poses = np.asarray(poses, dtype=np.float64)
        self.a = (fixed, ef, et, meas, info)
        self.vk, self.ek = vk, ek
        fx = R.active_fixed(len(self.poses), fixed, ef, et)
        self.H, self.b, self.lay = RT.build_system(self.poses, fx, ef, et, meas, info, vk, ek)
        lu = spla.splu(self.H, permc_spec="MMD_AT_PLUS_A", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))
        X, D = R._refine_solve(self.H, lu, self.b[:, None], steps=REFINEMENTS)
        self.dx, self.dx_err = X[:, 0], D[:, 0]
        self.inv, self.inv_err = R._refine_solve(self.H, lu, np.eye(self.lay.n), steps=REFINEMENTS)
        self.dx_scale = np.abs(self.inv) @ (abs(self.H) @ np.abs(self.dx) + np.abs(self.b))
        p1 = RT.gn_optimize(self.poses, fixed, ef, et, meas, info, 1, vk, ek)[0]
        self.dx_plain = self.step_of(p1)
        self.inv_plain = np.linalg.inv(self.H.toarray())
        self.live = np.flatnonzero(self.lay.off >= 0)
        self.nd = np.zeros(len(self.poses))
        self.nd[self.live] = [np.linalg.norm(self.block(self.inv, v, v)) for v in self.live]

    def step_of(self, poses1):
        """dx of the step to ``poses1`` in the layout's order (the heading's branch of 2 pi from the truth)."""
        return RT.step_vector(self.poses, np.asarray(poses1, dtype=np.float64), self.lay, self.dx)

    def apply(self, dx):
        return RT.apply_step(self.poses, self.lay, dx)

    def block(self, M, a, b):
        """The block (a, b) of a matrix in the layout's order, padded to 3x3 (a point's third row / column: zeros)."""
        out = np.zeros((3, 3))
        oa, da, ob, db = self.lay.off[a], self.lay.dim[a], self.lay.off[b], self.lay.dim[b]
        if oa >= 0 and ob >= 0:
            out[:da, :db] = M[oa:oa + da, ob:ob + db]
        return out

    def step_error(self, dx, of=None):
        """max over the free vertices of ||dx_v - T_v|| / ||(|H^-1| (|H| |T| + |b|))_v|| (``of``: an error vector in dx's
        place).  The block's own scale is not the step's norm: a vertex that hardly moves has cancelled, and its rounding has
        not (on pg300 the chained odometry guess leaves some vertices within 1e-9 of where they are, and by their own norm the
        unrefined SuperLU step is off by 0.7).  It is the componentwise forward bound of a solve: a step with componentwise
        backward error omega is off by at most omega times this scale, block by block (Oettli-Prager / Skeel), so a
        backward-stable solve's error is a few u here and a weak block is held by its own rows of |H^-1|."""
        d = (np.asarray(dx) - self.dx) if of is None else np.asarray(of)
        return max(np.linalg.norm(d[o:o + n]) / np.linalg.norm(self.dx_scale[o:o + n])
                   for o, n in zip(self.lay.off[self.live], self.lay.dim[self.live]))

    def step_own_error(self, dx, of=None):
        """max over the free vertices of ||dx_v - T_v|| / ||T_v||: the block's own norm (STEP_OWN)."""
        d = (np.asarray(dx) - self.dx) if of is None else np.asarray(of)
        return max(np.linalg.norm(d[o:o + n]) / np.linalg.norm(self.dx[o:o + n])
                   for o, n in zip(self.lay.off[self.live], self.lay.dim[self.live]))

    def pair_error(self, got, pairs, M=None, of=None):
        """max over ``pairs`` (a, b) of ||got_k - T_ab||_F / sqrt(||T_aa|| ||T_bb||); got [k, 3, 3], or the blocks of a
        matrix M in the layout's order, or (``of``) an error matrix.  Blocks of fixed / inactive vertices must be exact zeros."""
        worst = 0.0
        for k, (a, b) in enumerate(pairs):
            if self.lay.off[a] < 0 or self.lay.off[b] < 0:
                assert got is None or not np.any(got[k]), (a, b)
                continue
            if of is not None:
                d = self.block(of, a, b)
            else:
                d = (got[k] if got is not None else self.block(M, a, b)) - self.block(self.inv, a, b)
            worst = max(worst, np.linalg.norm(d) / np.sqrt(self.nd[a] * self.nd[b]))
        return worst


def solved(g):
    return Solved(*args(g), *kinds(g))


def spread(g, nK):
    """nK vertices spread evenly over the elimination order, the first column to the root's last (tests/test_boundary_gpu.py)."""
    from cg_mrslam_amd._lib import gn_symbolic_info
    V = len(g["poses"])
    _, perm = gn_symbolic_info(V, g["fixed"], g["edge_from"], g["edge_to"], want_perm=True)
    order = np.argsort(perm)
    return order[np.unique(np.linspace(0, V - 1, nK).round().astype(int))].astype(np.int32)


def queries(g):
    """q12: the first fixed vertex, the vertex eliminated last and a spread, 12 in all; q5, q17: the joint queries."""
    fixed0 = int(np.flatnonzero(g["fixed"])[0]) if g["fixed"].any() else 0
    q17 = spread(g, 17)
    last = int(q17[-1])
    rest = [int(v) for v in spread(g, 14) if int(v) not in (fixed0, last)]
    q12 = np.array(([fixed0, last] if fixed0 != last else [fixed0]) + rest, dtype=np.int32)[:12]
    return q12, spread(g, 5), q17


def joint_pairs(q):
    return [(int(a), int(b)) for a in q for b in q]


def joint_blocks(S, q):
    n = len(q)
    return np.asarray(S).reshape(n, 3, n, 3).transpose(0, 2, 1, 3).reshape(n * n, 3, 3)


def plain_errors(g, s=None):
    """quantity -> (e_ref, T's own error estimate) of a pose or typed graph: step, diag (every vertex), cross (every
    edge between two vertices), joint (every pair of q5 and of q17)."""
    s = solved(g) if s is None else s
    V = len(g["poses"])
    _, q5, q17 = queries(g)
    diag = [(v, v) for v in range(V)]
    cross = [(int(a), int(b)) for a, b in zip(g["edge_from"], g["edge_to"]) if a != b]
    joint = joint_pairs(q5) + joint_pairs(q17)
    out = {"step": (s.step_error(s.dx_plain), s.step_error(None, of=s.dx_err))}
    for name, pairs in (("diag", diag), ("cross", cross), ("joint", joint)):
        out[name] = (s.pair_error(None, pairs, M=s.inv_plain), s.pair_error(None, pairs, of=s.inv_err))
    return out


# ------------------------------------------------------------------------------------------------ condensed star
COND_QUERIES = 8


def condensed_query(g):
    """(gauge, query): the last vertex and 8 others spread over the indices."""
    V = len(g["poses"])
    return V - 1, np.linspace(0, V - 2, COND_QUERIES).astype(np.int32)


LD = np.longdouble


def _wrap(t):
    return np.arctan2(np.sin(t), np.cos(t))


def _inv_mul(a, b):
    """a^-1 b of two poses (x, y, theta), in the arguments' precision."""
    c, s = np.cos(a[2]), np.sin(a[2])
    dx, dy = b[0] - a[0], b[1] - a[1]
    return np.array([c * dx + s * dy, -s * dx + c * dy, _wrap(b[2] - a[2])], dtype=a.dtype)


def _chol3(A):
    n = A.shape[0]
    L = np.zeros((n, n), dtype=A.dtype)
    for j in range(n):
        d = A[j, j] - (L[j, :j] ** 2).sum()
        if not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    return L


def label_ut_extended(xg, xv, Sigma, alpha=1e-3, beta=2.0, reverse=False):
    """ref_numpy.label_edges_ut for one edge in long double (the 3x3 Cholesky factor and the adjugate inverse written out:
    LAPACK has no long double): (z [3], information [3, 3]) rounded to float64 at the end.  The labelling itself loses digits
    -- the sigma points lie alpha sqrt(3 Sigma) from the mean and their errors are differences of poses --, so the truth of a
    label needs more than float64 even from exact blocks.  reverse: the sums taken in the opposite order (the distance between the two
    is the long double labelling's own error estimate)."""
    from ref_condense_tree import _inv3_adjugate
    xg, xv, S = np.asarray(xg, dtype=LD), np.asarray(xv, dtype=LD), np.asarray(Sigma, dtype=LD)
    n = 3
    lam = LD(alpha) * LD(alpha) * n
    wm = np.full(2 * n + 1, 1 / (2 * (n + lam)), dtype=LD)
    wc = wm.copy()
    wm[0] = lam / (n + lam)
    wc[0] = wm[0] + (1 - LD(alpha) * LD(alpha) + LD(beta))
    z = _inv_mul(xg, xv)
    L = _chol3((n + lam) * S)
    assert L is not None
    pts = [np.zeros(3, dtype=LD)] + [sg * L[:, i] for i in range(n) for sg in (1, -1)]
    if reverse:                                                    # the same sums in the opposite order
        pts, wm, wc = pts[::-1], wm[::-1], wc[::-1]
    e = []
    for p in pts:
        x = xv + p
        x[2] = _wrap(x[2])
        e.append(_inv_mul(z, _inv_mul(xg, x)))
    e = np.array(e, dtype=LD)
    dev = e - wm @ e
    C = (wc[:, None, None] * dev[:, :, None] * dev[:, None, :]).sum(axis=0)
    return z.astype(np.float64), _inv3_adjugate(C).astype(np.float64)


def _labels(s, dx, inv, gauge, to, extended=False):
    p1 = s.apply(dx)
    cov = np.stack([s.block(inv, v, v) for v in to])
    if extended:
        out = [label_ut_extended(p1[gauge], p1[v], c) for v, c in zip(to, cov)]
        return np.array([o[0] for o in out]), np.array([o[1] for o in out]), cov, np.zeros(len(to), bool)
    est, iu, bad = R.label_edges_ut(p1[gauge], p1[to], cov)
    return est, R.info_full(iu), cov, bad


def est_error(a, b):
    d = np.asarray(a) - np.asarray(b)
    d[:, 2] = R.normalize_theta(d[:, 2])
    return float(np.abs(d).max())


def info_error(a, b):
    """max over the edges of ||a - b||_F / ||b||_F, full 3x3."""
    return max(np.linalg.norm(x - y) / np.linalg.norm(y) for x, y in zip(a, b))


def labels_extended(xg, xv, cov, reverse=False):
    """(est [n, 3], information [n, 3, 3]) of the edges gauge -> v by label_ut_extended."""
    out = [label_ut_extended(xg, x, c, reverse=reverse) for x, c in zip(xv, cov)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def T_nodes(gauge, query):
    import ref_condense_tree as T
    return T.nodes_of(gauge, query)


def joint_of(s, M, verts):
    """The joint matrix [3 n, 3 n] of the vertices' blocks of M (a Solved's layout)."""
    n = len(verts)
    out = np.zeros((3 * n, 3 * n))
    for a, u in enumerate(verts):
        for b, v in enumerate(verts):
            out[3 * a:3 * a + 3, 3 * b:3 * b + 3] = s.block(M, int(u), int(v))
    return out


def label_ut13_extended(xp, xc, S6, alpha=1e-3, beta=2.0, reverse=False):
    """ref_condense_tree.label_ut13 in long double, as label_ut_extended: (z [3], information [3, 3]) rounded at the end."""
    from ref_condense_tree import _inv3_adjugate
    xp, xc, S6 = np.asarray(xp, dtype=LD), np.asarray(xc, dtype=LD), np.asarray(S6, dtype=LD)
    n = 6
    lam = LD(alpha) * LD(alpha) * n
    wm = np.full(2 * n + 1, 1 / (2 * (n + lam)), dtype=LD)
    wc = wm.copy()
    wm[0] = lam / (n + lam)
    wc[0] = wm[0] + (1 - LD(alpha) * LD(alpha) + LD(beta))
    z = _inv_mul(xp, xc)
    L = _chol3((n + lam) * (S6 + S6.T) / 2)
    assert L is not None
    pts = [np.zeros(6, dtype=LD)] + [sg * L[:, i] for i in range(n) for sg in (1, -1)]
    if reverse:
        pts, wm, wc = pts[::-1], wm[::-1], wc[::-1]
    e = []
    for p in pts:
        a, b = xp + p[:3], xc + p[3:]
        a[2], b[2] = _wrap(a[2]), _wrap(b[2])
        e.append(_inv_mul(z, _inv_mul(a, b)))
    e = np.array(e, dtype=LD)
    dev = e - wm @ e
    C = (wc[:, None, None] * dev[:, :, None] * dev[:, None, :]).sum(axis=0)
    return z.astype(np.float64), _inv3_adjugate(C).astype(np.float64)


def _relative_cov_ld(xa, xb, Saa, Sab, Sbb):
    xa, xb = np.asarray(xa, dtype=LD), np.asarray(xb, dtype=LD)
    Saa, Sab, Sbb = (np.asarray(M, dtype=LD) for M in (Saa, Sab, Sbb))
    c, sn = np.cos(xa[2]), np.sin(xa[2])
    dx, dy = xb[0] - xa[0], xb[1] - xa[1]
    Ja = np.array([[-c, -sn, -sn * dx + c * dy], [sn, -c, -c * dx - sn * dy], [0, 0, -1]], dtype=LD)
    Jb = np.array([[c, sn, 0], [-sn, c, 0], [0, 0, 1]], dtype=LD)
    return Ja @ Saa @ Ja.T + Ja @ Sab @ Jb.T + Jb @ Sab.T @ Ja.T + Jb @ Sbb @ Jb.T


def tree_labels(poses, nodes, parent, Sigma, extended, reverse=False):
    """The edges parent[k] -> k of the nodes k = 1 .. nq at ``poses`` under the joint covariance Sigma of nodes 1 .. nq: a dict
    of est [nq, 3], info [nq, 3, 3], w [nq] (log det of the relative pose's covariance) and scale [nq] (the size of the terms
    the weight's covariance is the sum of, times ||Sz^-1||: tests/test_condense_tree_gpu.py's measure).  extended False:
    ref_condense_tree's float64 labels and weights; True: long double (7 points on the gauge, 13 otherwise; reverse: the sums
    in the opposite order, the log det by the determinant's expansion instead of the Cholesky factor)."""
    import ref_condense_tree as T
    import ref_joint_marginals as J
    nq = len(nodes) - 1
    est, info, w, scale = np.zeros((nq, 3)), np.zeros((nq, 3, 3)), np.zeros(nq), np.zeros(nq)
    if not extended:
        ed = T.edges_of(dict(nodes=nodes, Sigma=Sigma, poses1=poses), parent)
        assert not ed["flags"].any()
        est, info = ed["est"], R.info_full(ed["iu"])
    for k in range(1, nq + 1):
        p = int(parent[k])
        a, b = min(p, k), max(p, k)
        xa, xb = poses[nodes[a]], poses[nodes[b]]
        Saa, Sab, Sbb = T.node_block(Sigma, a, a), T.node_block(Sigma, a, b), T.node_block(Sigma, b, b)
        Sz = J.relative_cov(xa, xb, Saa, Sab, Sbb)
        scale[k - 1] = J.relative_cov_scale(xa, xb, Saa, Sab, Sbb) * np.linalg.norm(np.linalg.inv(Sz))
        if not extended:
            w[k - 1] = T.logdet_chol(Sz)
            continue
        Sz = _relative_cov_ld(xa, xb, Saa, Sab, Sbb)
        Sz = (Sz + Sz.T) / 2
        if reverse:
            m = Sz
            det = (m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0])
                   + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))
            w[k - 1] = float(np.log(det))
        else:
            w[k - 1] = float(2 * np.log(np.diag(_chol3(Sz))).sum())
        xp, xc = poses[nodes[p]], poses[nodes[k]]
        if p == 0:
            est[k - 1], info[k - 1] = label_ut_extended(xp, xc, T.node_block(Sigma, k, k), reverse=reverse)
        else:
            Spp, Spc, Scc = T.node_block(Sigma, p, p), T.node_block(Sigma, p, k), T.node_block(Sigma, k, k)
            est[k - 1], info[k - 1] = label_ut13_extended(xp, xc, np.block([[Spp, Spc], [Spc.T, Scc]]), reverse=reverse)
    return dict(est=est, info=info, w=w, scale=scale)


def weight_error(w, truth):
    """max over the edges of |w - w_T| / scale."""
    return float(np.max(np.abs(np.asarray(w) - truth["w"]) / truth["scale"]))


def condensed_reference(g):
    """CondensedGraphCreator::compute restated as ref_numpy.condense_ref does, with the step refined as well: the gauge alone
    fixed, the breadth-first guess, one step, the blocks of H^-1 at the guess, the unscented labels at the stepped poses.
    Returns dict(gauge, query, to, guess, fixed, est, cov -- the truth --, info, solved, errors) with errors: quantity ->
    (e_ref, T's own estimate) for
      cond_cov   the blocks, by their own norm
      cond_est   the measurements (absolute, the largest component); T's own estimate: the labels of the step moved by its
                 last correction
      cond_info  the labelling alone, per edge by its own norm: float64 labels (ref_numpy.label_edges_ut) against long double
                 ones on the same poses and blocks; T's own estimate: the long double sums taken in the opposite order.
    The information of the whole path (``info``: long double labels of the truth's blocks) is a block's error times the
    block's condition number; the truth's blocks are not known a hundred times better than np.linalg.inv's on every family
    (pg300 under heading_soft: their last correction moves the information by 9.4e-9, np.linalg.inv's blocks by 3.0e-7), so
    the path is held in its two halves: the blocks against the truth, the labels on the device's own blocks against long double."""
    gauge, query = condensed_query(g)
    p, _, ef, et, meas, info = args(g)
    fixed = np.zeros(len(p), np.uint8)
    fixed[gauge] = 1
    guess = RM.guess_bfs(p, fixed, ef, et, meas)
    s = Solved(guess, fixed, ef, et, meas, info)
    to = np.array([q for q in query if q != gauge], dtype=np.int32)
    cov, cov_p, cov_t = (np.stack([s.block(M, v, v) for v in to]) for M in (s.inv, s.inv_plain, s.inv + s.inv_err))
    p1, p1_p, p1_t = s.apply(s.dx), s.apply(s.dx_plain), s.apply(s.dx + s.dx_err)
    est, I = labels_extended(p1[gauge], p1[to], cov)
    _, I_rev = labels_extended(p1[gauge], p1[to], cov, reverse=True)
    est_t, _ = labels_extended(p1_t[gauge], p1_t[to], cov)
    est_p, _, _ = R.label_edges_ut(p1_p[gauge], p1_p[to], cov_p)
    _, iu64, bad = R.label_edges_ut(p1[gauge], p1[to], cov)
    assert not bad.any()
    errors = {"cond_cov": (info_error(cov_p, cov), info_error(cov_t, cov)),
              "cond_est": (est_error(est_p, est), est_error(est_t, est)),
              "cond_info": (info_error(R.info_full(iu64), I), info_error(I_rev, I))}
    # the whole path's information: valid where the truth's blocks are known well enough (PATH_INVALID otherwise)
    _, iu_p, _ = R.label_edges_ut(p1_p[gauge], p1_p[to], cov_p)
    _, I_t = labels_extended(p1_t[gauge], p1_t[to], cov_t)
    errors["cond_path_info"] = (info_error(R.info_full(iu_p), I), info_error(I_t, I))
    # the tree over the gauge and the requested vertices
    nodes = T_nodes(gauge, query)
    Sig, Sig_p, Sig_t = (joint_of(s, M, nodes[1:]) for M in (s.inv, s.inv_plain, s.inv + s.inv_err))
    import ref_condense_tree as T
    W, _ = T.weights(p1, nodes, Sig)
    parent = T.kruskal(W)
    tr = tree_labels(p1, nodes, parent, Sig, extended=True)
    tr_rev = tree_labels(p1, nodes, parent, Sig, extended=True, reverse=True)
    tr_64 = tree_labels(p1, nodes, parent, Sig, extended=False)
    tr_p = tree_labels(p1_p, nodes, parent, Sig_p, extended=False)
    tr_t = tree_labels(p1_t, nodes, parent, Sig_t, extended=True)
    errors.update({"tree_est": (est_error(tr_p["est"], tr["est"]), est_error(tr_t["est"], tr["est"])),
                   "tree_info": (info_error(tr_64["info"], tr["info"]), info_error(tr_rev["info"], tr["info"])),
                   "tree_w": (weight_error(tr_64["w"], tr), weight_error(tr_rev["w"], tr)),
                   "tree_path_info": (info_error(tr_p["info"], tr["info"]), info_error(tr_t["info"], tr["info"]))})
    return dict(gauge=gauge, query=query, to=to, guess=guess, fixed=fixed, est=est, info=I, cov=cov, solved=s, errors=errors,
                nodes=nodes, parent=parent, W=W, tree_margin=T.decision_margin(W, parent), p1=p1, Sigma=Sig)


# ------------------------------------------------------------------------------------------------ vertex removal
def _inverse_extended(A):
    """The inverse of a positive definite matrix in its own precision: A = L L^T by columns, L^-1 by forward substitution,
    A^-1 = L^-T L^-1."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - (L[j, :j] ** 2).sum())
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Z = np.zeros_like(A)
    for j in range(n):
        Z[j, :] = ((np.arange(n) == j) - L[j, :j] @ Z[:j, :]) / L[j, j]
    return Z.T @ Z


def _relative_cov_extended(xa, xb, Saa, Sab, Sbb):
    """ref_joint_marginals.relative_cov and ref_condense_tree.label_first_order in long double: (z, information)."""
    from ref_condense_tree import _inv3_adjugate
    xa, xb = np.asarray(xa, dtype=LD), np.asarray(xb, dtype=LD)
    c, sn = np.cos(xa[2]), np.sin(xa[2])
    dx, dy = xb[0] - xa[0], xb[1] - xa[1]
    Ja = np.array([[-c, -sn, -sn * dx + c * dy], [sn, -c, -c * dx - sn * dy], [0, 0, -1]], dtype=LD)
    Jb = np.array([[c, sn, 0], [-sn, c, 0], [0, 0, 1]], dtype=LD)
    Sz = Ja @ Saa @ Ja.T + Ja @ Sab @ Jb.T + Jb @ Sab.T @ Ja.T + Jb @ Sbb @ Jb.T
    z = _inv_mul(xa, xb)
    cz, sz = np.cos(z[2]), np.sin(z[2])
    Je = np.array([[cz, sz, 0], [-sz, cz, 0], [0, 0, 1]], dtype=LD)
    I = _inv3_adjugate(Je @ Sz @ Je.T)
    return z.astype(np.float64), (0.5 * (I + I.T)).astype(np.float64)


def star_args(g):
    return g["nV"], g["edge_from"], g["edge_to"], g["meas"], g["info"], g["remove"]


def star_reference(g):
    """ref_remove_nodes.remove_nodes on the star (``plain``: float64 throughout) and the truth of its numbers: the same local
    configuration, H and tree, then in long double the inverse of H (from its Cholesky factor), the relative-pose covariance of every tree
    edge and its first-order label.  T's own estimate: the same from H inverted in the reversed order of its columns.
    Returns dict(plain, est, info [n, 3, 3], margin, errors: rm_est (absolute), rm_info (per edge by its own norm))."""
    import ref_remove_nodes as RN
    plain = RN.remove_nodes(*star_args(g))
    per = plain["per"][0]
    assert plain["flags"].tolist() == [0] and per["fix"] == 0
    x, parent, m = per["x"], per["parent"], len(per["nbrs"])
    H = per["H"].astype(LD)
    H = 0.5 * (H + H.T)                     # (the diagonal blocks J^T Omega J are symmetric to rounding only)
    rev = np.arange(H.shape[0])[::-1]
    out = []
    for Hinv in (_inverse_extended(H), _inverse_extended(H[np.ix_(rev, rev)])[np.ix_(rev, rev)]):
        Hinv = 0.5 * (Hinv + Hinv.T)
        blk = lambda a, b: Hinv[3 * a:3 * a + 3, 3 * b:3 * b + 3] if a and b else np.zeros((3, 3), dtype=LD)   # noqa: E731
        lab = [_relative_cov_extended(x[parent[k]], x[k], blk(parent[k], parent[k]), blk(parent[k], k), blk(k, k)) for k in range(1, m)]
        out.append((np.array([l[0] for l in lab]), np.array([l[1] for l in lab])))
    (est, I), (est_r, I_r) = out
    I_p = np.array([R.info_full(u[None])[0] for u in plain["iu"]])
    errors = {"rm_est": (est_error(plain["est"], est), est_error(est_r, est)), "rm_info": (info_error(I_p, I), info_error(I_r, I))}
    return dict(plain=plain, est=est, info=I, margin=plain["margin"], errors=errors)


# ------------------------------------------------------------------------------------------------ Levenberg-Marquardt
RHO_MARGIN = 1e-6


def lm_decided(ref, family):
    """The leading iterations of a ref_lm trace whose every trial is decided by more than RHO_MARGIN: |rho| > RHO_MARGIN.
    Under ``weak`` that cannot be asked: g2o's rho = (currentChi - tempChi) / (dx^T (lambda dx + b) + 1e-3) carries an absolute
    1e-3, so with chi2 of 1e-9 every rho is a few 1e-9 whatever the step is worth (and lambda falls by 2/3 per iteration, the
    clip of 1 - (2 rho - 1)^3).  The decision there is the sign of currentChi - tempChi, asked to be a hundred times what
    test_lm_gpu.compared_iterations takes for rounding (1e3 u of currentChi): ten times the agreement test_lm_gpu.CHI_AGREE
    assumes of two chi2 sums.  (The graphs converge in three or four iterations; after that no gain is.)"""
    for t in ref["trace"]:
        if t["failed"]:
            continue
        if family == "weak":
            ok = abs(t["current"] - t["temp"]) > 1e5 * R.U * abs(t["current"])
        else:
            ok = abs(t["rho"]) > RHO_MARGIN
        if not ok:
            return t["iteration"]
    return ref["iters_done"]


def lm_truncated(ref, k):
    """A ref_lm result cut to its first k iterations."""
    return dict(ref, trace=[t for t in ref["trace"] if t["iteration"] < k], iters_done=min(ref["iters_done"], k),
                trials=ref["trials"][:k], lambdas=ref["lambdas"][:k], chi2=ref["chi2"][:k + 1])


# ------------------------------------------------------------------------------------------------ the bars
def bar(existing, e_ref):
    return max(existing, 10.0 * e_ref)


def valid(existing, e_ref, t_err):
    """T's own error estimate is at most e_ref / 100 -- where e_ref is so small that the existing bar is the one asserted
    (e_ref < existing / 10), at most a thousandth of that bar: a truth stored in float64 is itself rounded to 1.1e-16, and a
    hundredth of an e_ref of a few u is below that."""
    return t_err <= max(e_ref, existing / 10.0) / 100.0


# The step error below which nothing can be told: a few u.  The truth is stored in float64 (u of |dx|, at most u in either
# measure), the device's step is read back as a difference of rounded poses (u again), and ten times an e_ref of less than
# that would ask the device to beat the truth's own storage.  Above it the rule is 10 e_ref.
STEP_FLOOR = 4 * R.U
# the cases whose step is also held by the blocks' own norms ||dx_v - T_v|| / ||T_v|| (on pg300 and the typed graphs some
# vertices hardly move, and by their own norm the truth is not a hundred times better than the reference)
STEP_OWN = ("clique40", "blobs20", "forest2_40")

# quantity -> the existing bar it is held to where 10 e_ref is smaller (tests/test_reference_gpu.py MARG_TAU, reference_cases
# EST_ATOL and INFO_RTOL, remove_nodes_cases MEAS_ATOL and INFO_GAP x INFO_MARGIN)
EXISTING = {"step": STEP_FLOOR, "diag": 1e-9, "cross": 1e-9, "joint": 1e-9, "cond_cov": 1e-9, "cond_est": 3e-7, "cond_info": 1e-8,
            "cond_path_info": 1e-8, "tree_est": 3e-7, "tree_info": 1e-12, "tree_w": 1e-12, "tree_path_info": 1e-9, "step_own": STEP_FLOOR,
            "rm_est": K.MEAS_ATOL, "rm_info": K.INFO_GAP * K.INFO_MARGIN}


def reference_errors(name, family):
    """quantity -> (e_ref, T's own error estimate) of a (case, family), every quantity the case has."""
    g = graph(name, family)
    if CASES[name][0] == "star":
        return star_reference(g)["errors"]
    s = solved(g)
    out = plain_errors(g, s)
    if name in STEP_OWN:
        out["step_own"] = (s.step_own_error(s.dx_plain), s.step_own_error(None, of=s.dx_err))
    if name in CONDENSED:
        out.update(condensed_reference(g)["errors"])
    return out


# The information of a condensed edge over the whole path (blocks and labelling together) is a block's error times the block's
# condition number.  Where the truth's blocks are not known a hundred times better than np.linalg.inv's in that sense the
# whole-path quantity is not asserted (its two halves are: the blocks against the truth, the labelling on the device's own
# blocks against long double).  (case, family, quantity); tests/test_scale_cpu.py holds every entry that is not listed to the validity rule and every listed
# one to being invalid or valid by less than a factor 3.
PATH_INVALID = (
    ("clique40", "heading_soft", "cond_path_info"), ("clique40", "heading_soft", "tree_path_info"),
    ("blobs20", "heading_soft", "cond_path_info"), ("blobs20", "heading_soft", "tree_path_info"),
    ("pg300", "identity", "tree_path_info"), ("pg300", "edge_spread", "cond_path_info"), ("pg300", "edge_spread", "tree_path_info"),
    ("pg300", "component_spread", "cond_path_info"), ("pg300", "component_spread", "tree_path_info"),
    ("pg300", "full_spread", "cond_path_info"), ("pg300", "full_spread", "tree_path_info"),
    ("pg300", "heading_soft", "cond_path_info"), ("pg300", "heading_soft", "tree_path_info"),
    ("pg300", "far_origin", "tree_path_info"), ("pg300", "weak", "tree_path_info"),
    ("pg300", "weak", "cond_path_info"), ("blobs20", "weak", "tree_path_info"))       # (valid by a factor 1.0 and 1.1 only)

# case -> whether the device's weak / strong results are identity's bytes (times the power of two); where they are not, the
# measured rule above is what holds ("Input scale")
BYTE_IDENTICAL = {name: True for name in CASES}

# (case, family) -> {quantity: (e_ref, T's own error estimate, e_dev)}: e_ref and T's estimate as tests/test_scale_cpu.py
# measures them (it fails where an e_ref here is off by more than a factor 2), e_dev as tests/test_scale_gpu.py printed it on
# an MI355X (a record only: no bar is derived from it; None: the typed entry points return no edge blocks, the joint blocks
# cover them).
MEASURED = {
    ("clique40", "identity"): {"step": (9.80e-17, 1.9e-19, 1.03e-16), "diag": (2.93e-15, 7.0e-17, 7.19e-15), "cross": (3.18e-15, 4.8e-17, 6.31e-15), "joint": (1.96e-15, 6.2e-17, 5.08e-15), "step_own": (9.36e-14, 7.7e-17, 9.36e-14), "cond_cov": (1.95e-14, 1.5e-18, 1.06e-13), "cond_est": (6.22e-15, 0.0e+00, 2.67e-15), "cond_info": (2.69e-13, 0.0e+00, 2.67e-13), "cond_path_info": (2.66e-13, 0.0e+00, 2.68e-13), "tree_est": (3.55e-15, 0.0e+00, 3.55e-15), "tree_info": (4.12e-13, 1.2e-20, 3.36e-13), "tree_w": (9.87e-20, 0.0e+00, 2.27e-19), "tree_path_info": (2.24e-13, 2.6e-17, 3.36e-13)},
    ("clique40", "edge_spread"): {"step": (5.32e-17, 1.5e-19, 5.65e-17), "diag": (1.85e-15, 8.0e-17, 3.65e-15), "cross": (1.81e-15, 4.8e-17, 3.29e-15), "joint": (1.55e-15, 7.2e-17, 3.30e-15), "step_own": (8.06e-14, 8.2e-17, 9.00e-14), "cond_cov": (2.13e-14, 9.6e-18, 1.78e-13), "cond_est": (3.55e-15, 0.0e+00, 1.51e-14), "cond_info": (9.88e-13, 0.0e+00, 9.97e-13), "cond_path_info": (9.90e-13, 0.0e+00, 9.87e-13), "tree_est": (7.66e-15, 0.0e+00, 8.88e-15), "tree_info": (1.02e-12, 0.0e+00, 1.30e-12), "tree_w": (2.34e-19, 0.0e+00, 9.51e-20), "tree_path_info": (1.04e-12, 6.6e-17, 1.31e-12)},
    ("clique40", "component_spread"): {"step": (7.70e-17, 1.8e-19, 8.65e-17), "diag": (1.73e-15, 8.7e-17, 3.71e-15), "cross": (2.90e-15, 5.9e-17, 3.71e-15), "joint": (1.81e-15, 8.7e-17, 3.73e-15), "step_own": (1.21e-13, 9.2e-17, 2.43e-13), "cond_cov": (2.19e-13, 1.8e-16, 3.14e-13), "cond_est": (4.44e-14, 4.4e-16, 1.57e-13), "cond_info": (5.99e-13, 2.4e-18, 5.68e-13), "cond_path_info": (6.02e-13, 1.4e-14, 6.02e-13), "tree_est": (6.88e-15, 4.4e-16, 2.13e-14), "tree_info": (7.47e-13, 0.0e+00, 7.53e-13), "tree_w": (9.37e-19, 0.0e+00, 2.45e-20), "tree_path_info": (9.33e-13, 1.0e-14, 7.44e-13)},
    ("clique40", "full_spread"): {"step": (5.09e-17, 1.8e-19, 5.43e-17), "diag": (2.49e-15, 9.0e-17, 7.40e-15), "cross": (2.37e-15, 5.8e-17, 6.71e-15), "joint": (2.49e-15, 8.4e-17, 7.74e-15), "step_own": (9.23e-14, 7.8e-17, 1.63e-13), "cond_cov": (1.00e-13, 2.6e-16, 4.10e-13), "cond_est": (4.44e-15, 0.0e+00, 9.77e-14), "cond_info": (4.41e-13, 5.3e-18, 4.31e-13), "cond_path_info": (4.43e-13, 1.8e-14, 4.33e-13), "tree_est": (6.22e-15, 0.0e+00, 5.68e-14), "tree_info": (8.51e-13, 2.1e-20, 1.43e-12), "tree_w": (4.81e-19, 0.0e+00, 4.81e-19), "tree_path_info": (1.23e-12, 5.3e-15, 1.44e-12)},
    ("clique40", "heading_stiff"): {"step": (6.91e-17, 2.7e-19, 7.41e-17), "diag": (1.73e-15, 5.6e-17, 3.67e-15), "cross": (4.24e-15, 3.3e-17, 3.54e-15), "joint": (2.32e-15, 5.4e-17, 3.65e-15), "step_own": (1.19e-13, 8.5e-17, 1.20e-13), "cond_cov": (4.25e-15, 0.0e+00, 2.95e-15), "cond_est": (3.55e-15, 0.0e+00, 3.55e-15), "cond_info": (1.13e-10, 1.7e-27, 1.13e-10), "cond_path_info": (1.13e-10, 0.0e+00, 1.13e-10), "tree_est": (4.44e-15, 0.0e+00, 2.47e-15), "tree_info": (2.87e-10, 8.3e-27, 2.87e-10), "tree_w": (3.16e-24, 0.0e+00, 1.67e-22), "tree_path_info": (2.87e-10, 0.0e+00, 2.87e-10)},
    ("clique40", "heading_soft"): {"step": (9.10e-17, 3.1e-19, 1.13e-16), "diag": (2.56e-15, 6.6e-17, 4.95e-15), "cross": (3.39e-15, 4.9e-17, 4.40e-15), "joint": (1.86e-15, 6.6e-17, 4.31e-15), "step_own": (1.21e-13, 8.4e-17, 1.78e-13), "cond_cov": (1.25e-11, 1.7e-14, 1.24e-11), "cond_est": (4.49e-12, 3.6e-15, 9.29e-12), "cond_info": (2.31e-12, 5.7e-13, 4.54e-10), "cond_path_info": (7.39e-11, 1.0e-10, None), "tree_est": (6.49e-13, 3.6e-15, 1.34e-12), "tree_info": (1.18e-12, 2.1e-16, 7.16e-13), "tree_w": (6.89e-18, 0.0e+00, 9.19e-18), "tree_path_info": (6.88e-11, 8.5e-11, None)},
    ("clique40", "millimetres"): {"step": (6.84e-17, 1.8e-19, 7.07e-17), "diag": (1.25e-13, 8.3e-17, 6.28e-15), "cross": (4.03e-13, 4.5e-17, 5.88e-15), "joint": (3.60e-13, 7.7e-17, 4.90e-15), "step_own": (4.08e-13, 8.7e-17, 4.51e-13), "cond_cov": (4.40e-13, 9.0e-25, 9.45e-14), "cond_est": (3.64e-12, 0.0e+00, 3.64e-12), "cond_info": (2.82e-13, 0.0e+00, 2.74e-13), "cond_path_info": (5.21e-12, 6.5e-16, 2.81e-13), "tree_est": (3.64e-12, 0.0e+00, 1.82e-12), "tree_info": (5.00e-13, 0.0e+00, 3.42e-13), "tree_w": (7.44e-24, 0.0e+00, 1.49e-23), "tree_path_info": (2.21e-12, 5.4e-16, 3.41e-13)},
    ("clique40", "far_origin"): {"step": (4.56e-12, 1.9e-19, 4.56e-12), "diag": (3.03e-15, 7.6e-17, 6.16e-15), "cross": (4.78e-15, 4.6e-17, 6.64e-15), "joint": (2.94e-15, 7.6e-17, 6.33e-15), "step_own": (2.62e-08, 8.6e-17, 2.62e-08), "cond_cov": (3.38e-14, 1.6e-17, 3.76e-15), "cond_est": (1.95e-10, 0.0e+00, 1.78e-15), "cond_info": (5.91e-10, 0.0e+00, 5.91e-10), "cond_path_info": (5.91e-10, 2.8e-15, 5.91e-10), "tree_est": (1.61e-10, 0.0e+00, 1.16e-14), "tree_info": (2.99e-09, 0.0e+00, 2.99e-09), "tree_w": (3.29e-18, 0.0e+00, 3.29e-18), "tree_path_info": (2.99e-09, 1.3e-15, 2.99e-09)},
    ("clique40", "weak"): {"step": (9.80e-17, 1.9e-19, 1.03e-16), "diag": (2.93e-15, 7.0e-17, 7.19e-15), "cross": (3.18e-15, 4.8e-17, 6.31e-15), "joint": (1.96e-15, 6.2e-17, 5.08e-15), "step_own": (9.36e-14, 7.7e-17, 9.36e-14), "cond_cov": (1.95e-14, 1.5e-18, 1.06e-13), "cond_est": (6.22e-15, 0.0e+00, 2.67e-15), "cond_info": (2.31e-12, 0.0e+00, 5.63e-12), "cond_path_info": (2.22e-11, 1.4e-15, 1.09e-10), "tree_est": (3.55e-15, 0.0e+00, 3.55e-15), "tree_info": (5.58e-13, 0.0e+00, 4.86e-13), "tree_w": (1.20e-19, 0.0e+00, 1.20e-19), "tree_path_info": (3.06e-11, 6.5e-14, 1.85e-10)},
    ("clique40", "strong"): {"step": (9.80e-17, 1.9e-19, 1.03e-16), "diag": (2.93e-15, 7.0e-17, 7.19e-15), "cross": (3.18e-15, 4.8e-17, 6.31e-15), "joint": (1.96e-15, 6.2e-17, 5.08e-15), "step_own": (9.36e-14, 7.7e-17, 9.36e-14), "cond_cov": (1.95e-14, 1.5e-18, 1.06e-13), "cond_est": (6.22e-15, 0.0e+00, 2.67e-15), "cond_info": (4.10e-07, 2.3e-18, 4.10e-07), "cond_path_info": (4.10e-07, 0.0e+00, 4.10e-07), "tree_est": (3.55e-15, 0.0e+00, 3.55e-15), "tree_info": (2.92e-07, 1.2e-21, 2.94e-07), "tree_w": (1.17e-16, 0.0e+00, 4.54e-19), "tree_path_info": (3.13e-07, 0.0e+00, 2.94e-07)},
    ("blobs20", "identity"): {"step": (6.34e-17, 2.1e-19, 9.04e-17), "diag": (1.08e-14, 7.4e-17, 3.55e-15), "cross": (8.25e-15, 4.3e-17, 2.91e-15), "joint": (3.88e-15, 6.0e-17, 3.45e-15), "step_own": (1.36e-13, 9.5e-17, 1.81e-13), "cond_cov": (1.09e-14, 1.4e-16, 5.82e-14), "cond_est": (2.04e-14, 0.0e+00, 2.04e-14), "cond_info": (2.07e-13, 5.5e-19, 2.36e-13), "cond_path_info": (2.15e-13, 3.9e-15, 2.22e-13), "tree_est": (5.11e-15, 0.0e+00, 5.99e-15), "tree_info": (3.04e-13, 0.0e+00, 2.82e-13), "tree_w": (5.24e-19, 0.0e+00, 5.24e-19), "tree_path_info": (7.20e-13, 2.6e-15, 2.82e-13)},
    ("blobs20", "edge_spread"): {"step": (6.00e-17, 1.6e-19, 7.88e-17), "diag": (4.43e-15, 9.4e-17, 6.00e-15), "cross": (3.05e-15, 4.8e-17, 4.82e-15), "joint": (1.52e-15, 9.4e-17, 6.22e-15), "step_own": (1.05e-13, 9.7e-17, 1.35e-13), "cond_cov": (5.23e-14, 2.0e-17, 1.68e-13), "cond_est": (9.94e-15, 0.0e+00, 4.26e-14), "cond_info": (8.39e-13, 0.0e+00, 8.22e-13), "cond_path_info": (8.40e-13, 1.8e-15, 8.40e-13), "tree_est": (3.11e-15, 0.0e+00, 1.20e-14), "tree_info": (7.70e-13, 0.0e+00, 7.58e-13), "tree_w": (1.03e-19, 0.0e+00, 1.57e-19), "tree_path_info": (7.81e-13, 2.1e-15, 7.57e-13)},
    ("blobs20", "component_spread"): {"step": (3.88e-17, 1.3e-19, 9.20e-17), "diag": (3.64e-15, 9.0e-17, 8.17e-15), "cross": (5.33e-15, 5.0e-17, 5.34e-15), "joint": (1.93e-15, 9.0e-17, 5.23e-15), "step_own": (1.55e-13, 8.9e-17, 5.68e-13), "cond_cov": (7.26e-14, 4.4e-16, 7.76e-13), "cond_est": (4.97e-14, 1.4e-17, 1.60e-13), "cond_info": (5.02e-13, 7.1e-18, 5.20e-13), "cond_path_info": (5.01e-13, 1.5e-14, 5.09e-13), "tree_est": (1.29e-14, 0.0e+00, 4.29e-14), "tree_info": (7.76e-13, 2.0e-18, 1.07e-12), "tree_w": (3.98e-19, 0.0e+00, 3.98e-19), "tree_path_info": (6.10e-13, 1.3e-14, 1.06e-12)},
    ("blobs20", "full_spread"): {"step": (4.44e-17, 9.0e-20, 7.70e-17), "diag": (1.62e-15, 7.6e-17, 5.00e-15), "cross": (4.06e-15, 4.3e-17, 2.85e-15), "joint": (1.62e-15, 7.6e-17, 3.31e-15), "step_own": (1.30e-13, 9.5e-17, 2.24e-13), "cond_cov": (1.76e-14, 4.3e-16, 2.34e-14), "cond_est": (5.06e-14, 0.0e+00, 7.73e-14), "cond_info": (9.41e-13, 1.4e-16, 8.92e-13), "cond_path_info": (9.41e-13, 1.3e-14, 9.49e-13), "tree_est": (1.40e-14, 0.0e+00, 1.95e-14), "tree_info": (8.59e-13, 0.0e+00, 8.50e-13), "tree_w": (1.04e-17, 0.0e+00, 9.73e-19), "tree_path_info": (9.00e-13, 2.2e-14, 8.55e-13)},
    ("blobs20", "heading_stiff"): {"step": (7.21e-17, 2.3e-19, 9.52e-17), "diag": (3.30e-15, 8.1e-17, 2.85e-15), "cross": (7.50e-15, 3.4e-17, 2.38e-15), "joint": (5.46e-15, 7.8e-17, 2.38e-15), "step_own": (1.59e-13, 1.0e-16, 1.66e-13), "cond_cov": (7.65e-15, 3.1e-22, 4.41e-15), "cond_est": (2.66e-15, 0.0e+00, 1.78e-15), "cond_info": (6.57e-11, 2.0e-27, 6.57e-11), "cond_path_info": (6.57e-11, 0.0e+00, 6.57e-11), "tree_est": (3.55e-15, 0.0e+00, 3.55e-15), "tree_info": (8.85e-11, 6.0e-27, 8.85e-11), "tree_w": (7.78e-24, 0.0e+00, 1.67e-22), "tree_path_info": (8.85e-11, 0.0e+00, 8.85e-11)},
    ("blobs20", "heading_soft"): {"step": (7.77e-17, 1.9e-19, 1.25e-16), "diag": (1.67e-14, 7.1e-17, 2.46e-15), "cross": (1.03e-14, 3.6e-17, 2.58e-15), "joint": (2.34e-15, 6.8e-17, 2.51e-15), "step_own": (1.61e-13, 9.1e-17, 3.13e-13), "cond_cov": (2.87e-11, 3.3e-13, 7.05e-11), "cond_est": (2.45e-12, 1.8e-15, 1.93e-11), "cond_info": (1.01e-11, 2.2e-12, 1.31e-09), "cond_path_info": (7.38e-10, 4.3e-09, None), "tree_est": (6.38e-13, 1.8e-15, 5.03e-12), "tree_info": (4.29e-12, 1.7e-15, 4.07e-12), "tree_w": (2.47e-18, 1.3e-19, 2.80e-19), "tree_path_info": (3.74e-10, 6.4e-10, None)},
    ("blobs20", "millimetres"): {"step": (6.19e-17, 2.2e-19, 7.87e-17), "diag": (5.38e-13, 6.9e-17, 2.56e-15), "cross": (1.18e-12, 3.8e-17, 2.41e-15), "joint": (1.02e-12, 6.9e-17, 2.47e-15), "step_own": (2.01e-13, 9.7e-17, 2.24e-13), "cond_cov": (8.00e-12, 1.2e-16, 8.03e-14), "cond_est": (1.55e-11, 0.0e+00, 5.46e-12), "cond_info": (2.06e-13, 0.0e+00, 2.46e-13), "cond_path_info": (5.08e-12, 7.0e-16, 2.14e-13), "tree_est": (3.64e-12, 0.0e+00, 5.00e-12), "tree_info": (2.54e-13, 0.0e+00, 2.64e-13), "tree_w": (3.85e-24, 6.6e-33, 3.85e-24), "tree_path_info": (4.02e-12, 1.5e-15, 2.66e-13)},
    ("blobs20", "far_origin"): {"step": (4.27e-12, 2.0e-19, 4.27e-12), "diag": (4.48e-15, 7.3e-17, 2.13e-15), "cross": (1.12e-14, 3.9e-17, 1.58e-15), "joint": (2.48e-15, 6.4e-17, 2.13e-15), "step_own": (6.86e-09, 7.7e-17, 6.86e-09), "cond_cov": (3.51e-14, 1.6e-16, 6.10e-14), "cond_est": (2.04e-10, 0.0e+00, 1.78e-15), "cond_info": (4.61e-10, 0.0e+00, 4.61e-10), "cond_path_info": (4.61e-10, 5.6e-16, 4.61e-10), "tree_est": (1.72e-10, 0.0e+00, 3.09e-14), "tree_info": (2.98e-09, 2.6e-21, 2.98e-09), "tree_w": (4.88e-20, 0.0e+00, 4.26e-20), "tree_path_info": (2.98e-09, 6.1e-16, 2.98e-09)},
    ("blobs20", "weak"): {"step": (6.34e-17, 2.1e-19, 9.04e-17), "diag": (1.08e-14, 7.4e-17, 3.55e-15), "cross": (8.25e-15, 4.3e-17, 2.91e-15), "joint": (3.88e-15, 6.0e-17, 3.45e-15), "step_own": (1.36e-13, 9.5e-17, 1.81e-13), "cond_cov": (1.09e-14, 1.4e-16, 5.82e-14), "cond_est": (2.04e-14, 0.0e+00, 2.04e-14), "cond_info": (2.12e-12, 0.0e+00, 3.59e-12), "cond_path_info": (5.20e-11, 2.7e-12, 2.31e-10), "tree_est": (5.11e-15, 0.0e+00, 5.99e-15), "tree_info": (1.08e-12, 0.0e+00, 2.20e-12), "tree_w": (4.28e-19, 0.0e+00, 2.99e-17), "tree_path_info": (5.20e-11, 9.0e-13, 2.31e-10)},
    ("blobs20", "strong"): {"step": (6.34e-17, 2.1e-19, 9.04e-17), "diag": (1.08e-14, 7.4e-17, 3.55e-15), "cross": (8.25e-15, 4.3e-17, 2.91e-15), "joint": (3.88e-15, 6.0e-17, 3.45e-15), "step_own": (1.36e-13, 9.5e-17, 1.81e-13), "cond_cov": (1.09e-14, 1.4e-16, 5.82e-14), "cond_est": (2.04e-14, 0.0e+00, 2.04e-14), "cond_info": (4.98e-07, 0.0e+00, 4.98e-07), "cond_path_info": (4.98e-07, 0.0e+00, 4.98e-07), "tree_est": (5.11e-15, 0.0e+00, 5.99e-15), "tree_info": (3.42e-07, 1.9e-21, 3.42e-07), "tree_w": (1.05e-18, 0.0e+00, 8.52e-20), "tree_path_info": (3.44e-07, 0.0e+00, 3.42e-07)},
    ("forest2_40", "identity"): {"step": (9.61e-17, 1.7e-19, 1.12e-16), "diag": (2.20e-15, 8.3e-17, 2.31e-15), "cross": (3.39e-15, 4.8e-17, 1.70e-15), "joint": (2.01e-15, 8.0e-17, 1.55e-15), "step_own": (1.24e-13, 8.0e-17, 1.36e-13)},
    ("forest2_40", "edge_spread"): {"step": (4.94e-17, 1.6e-19, 5.70e-17), "diag": (2.44e-15, 8.6e-17, 8.75e-15), "cross": (2.74e-15, 6.2e-17, 8.31e-15), "joint": (2.44e-15, 7.3e-17, 9.21e-15), "step_own": (1.15e-13, 9.2e-17, 1.15e-13)},
    ("forest2_40", "component_spread"): {"step": (6.06e-17, 1.3e-19, 7.81e-17), "diag": (3.07e-15, 8.6e-17, 7.63e-15), "cross": (3.97e-15, 5.3e-17, 6.81e-15), "joint": (1.98e-15, 8.6e-17, 6.23e-15), "step_own": (1.22e-13, 8.7e-17, 2.23e-13)},
    ("forest2_40", "full_spread"): {"step": (3.92e-17, 1.2e-19, 8.04e-17), "diag": (2.21e-15, 7.2e-17, 6.72e-15), "cross": (4.13e-15, 6.5e-17, 6.57e-15), "joint": (1.56e-15, 7.0e-17, 5.56e-15), "step_own": (1.12e-13, 8.5e-17, 2.03e-13)},
    ("forest2_40", "heading_stiff"): {"step": (7.87e-17, 2.6e-19, 8.36e-17), "diag": (3.32e-15, 6.4e-17, 1.43e-15), "cross": (5.77e-15, 3.4e-17, 1.25e-15), "joint": (2.25e-15, 5.3e-17, 1.51e-15), "step_own": (5.86e-14, 8.7e-17, 6.29e-14)},
    ("forest2_40", "heading_soft"): {"step": (7.56e-17, 1.5e-19, 7.66e-17), "diag": (3.33e-15, 9.4e-17, 4.29e-15), "cross": (3.10e-15, 4.6e-17, 3.48e-15), "joint": (2.62e-15, 7.1e-17, 2.79e-15), "step_own": (1.21e-13, 8.3e-17, 1.10e-13)},
    ("forest2_40", "millimetres"): {"step": (7.07e-17, 1.6e-19, 8.28e-17), "diag": (3.31e-13, 7.6e-17, 5.89e-15), "cross": (7.15e-13, 4.7e-17, 5.08e-15), "joint": (2.57e-13, 7.6e-17, 5.95e-15), "step_own": (1.96e-13, 1.0e-16, 1.96e-13)},
    ("forest2_40", "far_origin"): {"step": (5.04e-12, 1.7e-19, 5.04e-12), "diag": (2.86e-15, 9.1e-17, 2.55e-15), "cross": (3.32e-15, 6.3e-17, 2.24e-15), "joint": (2.26e-15, 9.1e-17, 1.78e-15), "step_own": (8.26e-09, 9.6e-17, 8.26e-09)},
    ("forest2_40", "weak"): {"step": (9.61e-17, 1.7e-19, 1.12e-16), "diag": (2.20e-15, 8.3e-17, 2.31e-15), "cross": (3.39e-15, 4.8e-17, 1.70e-15), "joint": (2.01e-15, 8.0e-17, 1.55e-15), "step_own": (1.24e-13, 8.0e-17, 1.36e-13)},
    ("forest2_40", "strong"): {"step": (9.61e-17, 1.7e-19, 1.12e-16), "diag": (2.20e-15, 8.3e-17, 2.31e-15), "cross": (3.39e-15, 4.8e-17, 1.70e-15), "joint": (2.01e-15, 8.0e-17, 1.55e-15), "step_own": (1.24e-13, 8.0e-17, 1.36e-13)},
    ("pg300", "identity"): {"step": (2.23e-18, 2.5e-21, 4.93e-18), "diag": (7.23e-11, 1.4e-13, 1.05e-10), "cross": (7.23e-11, 1.4e-13, 1.05e-10), "joint": (7.23e-11, 8.8e-14, 1.04e-10), "cond_cov": (8.94e-11, 5.3e-14, 1.30e-11), "cond_est": (3.65e-11, 2.8e-14, 7.27e-11), "cond_info": (4.51e-15, 0.0e+00, 5.91e-15), "cond_path_info": (3.60e-11, 1.3e-13, 6.95e-12), "tree_est": (7.37e-12, 5.3e-15, 1.59e-11), "tree_info": (3.35e-14, 0.0e+00, 7.65e-15), "tree_w": (3.06e-19, 0.0e+00, 2.78e-19), "tree_path_info": (4.34e-11, 6.8e-12, None)},
    ("pg300", "edge_spread"): {"step": (4.76e-18, 9.0e-22, 1.50e-17), "diag": (9.34e-10, 5.5e-12, 6.18e-09), "cross": (9.34e-10, 5.5e-12, 6.18e-09), "joint": (9.40e-10, 3.7e-12, 6.18e-09), "cond_cov": (1.97e-09, 7.9e-13, 1.71e-09), "cond_est": (7.00e-10, 1.2e-12, 1.87e-09), "cond_info": (1.34e-14, 2.5e-19, 1.45e-14), "cond_path_info": (1.39e-09, 1.6e-11, None), "tree_est": (9.13e-11, 2.0e-13, 2.99e-10), "tree_info": (3.06e-13, 0.0e+00, 9.97e-14), "tree_w": (7.89e-19, 0.0e+00, 3.02e-20), "tree_path_info": (1.16e-08, 6.6e-10, None)},
    ("pg300", "component_spread"): {"step": (4.51e-18, 2.8e-21, 4.91e-18), "diag": (3.29e-08, 5.6e-11, 2.01e-08), "cross": (3.29e-08, 5.6e-11, 2.01e-08), "joint": (3.28e-08, 4.1e-11, 2.01e-08), "cond_cov": (4.13e-09, 2.2e-12, 4.63e-09), "cond_est": (3.28e-09, 6.3e-12, 1.02e-08), "cond_info": (5.76e-14, 1.4e-17, 3.95e-14), "cond_path_info": (1.30e-09, 1.2e-10, None), "tree_est": (9.32e-10, 1.3e-12, 3.13e-09), "tree_info": (1.62e-13, 4.8e-20, 5.72e-14), "tree_w": (2.87e-19, 0.0e+00, 7.61e-19), "tree_path_info": (2.08e-09, 1.3e-09, None)},
    ("pg300", "full_spread"): {"step": (1.19e-17, 6.6e-21, 7.36e-18), "diag": (1.65e-08, 4.4e-11, 2.22e-08), "cross": (1.64e-08, 4.4e-11, 2.22e-08), "joint": (1.62e-08, 3.6e-11, 2.24e-08), "cond_cov": (3.32e-09, 6.3e-12, 9.00e-09), "cond_est": (1.61e-08, 1.3e-11, 1.25e-08), "cond_info": (1.42e-14, 1.8e-16, 6.71e-14), "cond_path_info": (7.01e-09, 7.4e-10, None), "tree_est": (4.10e-09, 3.3e-12, 3.46e-09), "tree_info": (9.52e-13, 1.3e-17, 4.01e-13), "tree_w": (4.97e-19, 0.0e+00, 6.09e-19), "tree_path_info": (3.45e-08, 2.1e-08, None)},
    ("pg300", "heading_stiff"): {"step": (5.04e-18, 3.2e-21, 7.72e-18), "diag": (9.24e-12, 1.6e-15, 1.71e-12), "cross": (9.25e-12, 1.6e-15, 1.71e-12), "joint": (1.23e-11, 1.2e-15, 1.71e-12), "cond_cov": (5.53e-12, 5.5e-16, 1.32e-12), "cond_est": (6.82e-13, 3.6e-15, 5.14e-12), "cond_info": (1.91e-12, 1.5e-22, 1.91e-12), "cond_path_info": (4.71e-12, 2.0e-15, 2.81e-12), "tree_est": (5.56e-13, 1.8e-15, 1.17e-12), "tree_info": (1.91e-12, 2.9e-27, 1.91e-12), "tree_w": (4.58e-25, 0.0e+00, 3.45e-25), "tree_path_info": (5.46e-12, 1.6e-14, 1.91e-12)},
    ("pg300", "heading_soft"): {"step": (3.12e-18, 2.3e-21, 6.05e-18), "diag": (1.68e-07, 1.1e-10, 1.05e-07), "cross": (1.68e-07, 1.1e-10, 1.05e-07), "joint": (1.68e-07, 1.0e-10, 1.05e-07), "cond_cov": (9.20e-08, 5.0e-11, 7.45e-08), "cond_est": (2.67e-07, 1.6e-10, 5.86e-07), "cond_info": (4.26e-14, 1.2e-18, 6.72e-14), "cond_path_info": (3.00e-07, 9.4e-09, None), "tree_est": (7.75e-08, 4.8e-11, 2.07e-07), "tree_info": (7.28e-14, 1.8e-17, 1.23e-13), "tree_w": (1.72e-17, 0.0e+00, 2.58e-17), "tree_path_info": (2.02e-06, 4.9e-08, None)},
    ("pg300", "millimetres"): {"step": (6.02e-18, 6.4e-21, 1.26e-17), "diag": (2.66e-09, 1.9e-13, 1.33e-10), "cross": (2.70e-09, 1.9e-13, 1.33e-10), "joint": (2.43e-09, 1.6e-13, 1.32e-10), "cond_cov": (2.22e-09, 7.8e-14, 1.45e-10), "cond_est": (6.34e-08, 7.3e-12, 1.04e-07), "cond_info": (5.44e-15, 0.0e+00, 8.80e-15), "cond_path_info": (4.16e-09, 1.9e-13, 2.43e-11), "tree_est": (1.40e-08, 1.8e-12, 2.11e-08), "tree_info": (9.83e-14, 0.0e+00, 2.52e-14), "tree_w": (1.65e-30, 0.0e+00, 4.70e-31), "tree_path_info": (3.39e-09, 4.3e-12, 6.50e-11)},
    ("pg300", "far_origin"): {"step": (1.06e-16, 2.1e-21, 1.06e-16), "diag": (2.67e-11, 1.1e-13, 2.57e-10), "cross": (2.67e-11, 1.1e-13, 2.57e-10), "joint": (2.68e-11, 7.7e-14, 2.56e-10), "cond_cov": (9.14e-11, 2.3e-14, 3.78e-11), "cond_est": (2.52e-10, 4.4e-16, 9.23e-11), "cond_info": (1.31e-10, 0.0e+00, 1.31e-10), "cond_path_info": (1.31e-10, 2.8e-13, 1.31e-10), "tree_est": (1.11e-10, 7.1e-15, 1.13e-10), "tree_info": (1.31e-10, 0.0e+00, 1.31e-10), "tree_w": (2.64e-19, 0.0e+00, 7.39e-17), "tree_path_info": (1.31e-10, 6.4e-12, None)},
    ("pg300", "weak"): {"step": (2.23e-18, 2.5e-21, 4.93e-18), "diag": (7.23e-11, 1.4e-13, 1.05e-10), "cross": (7.23e-11, 1.4e-13, 1.05e-10), "joint": (7.23e-11, 8.8e-14, 1.04e-10), "cond_cov": (8.94e-11, 5.3e-14, 1.30e-11), "cond_est": (3.65e-11, 2.8e-14, 7.27e-11), "cond_info": (7.19e-10, 1.2e-15, 2.50e-09), "cond_path_info": (3.07e-05, 3.1e-07, 2.24e-05), "tree_est": (7.37e-12, 5.3e-15, 1.59e-11), "tree_info": (3.19e-10, 0.0e+00, 3.75e-10), "tree_w": (8.43e-18, 0.0e+00, 1.48e-16), "tree_path_info": (5.67e-06, 8.3e-08, None)},
    ("pg300", "strong"): {"step": (2.23e-18, 2.5e-21, 4.93e-18), "diag": (7.23e-11, 1.4e-13, 1.05e-10), "cross": (7.23e-11, 1.4e-13, 1.05e-10), "joint": (7.23e-11, 8.8e-14, 1.04e-10), "cond_cov": (8.94e-11, 5.3e-14, 1.30e-11), "cond_est": (3.65e-11, 2.8e-14, 7.27e-11), "cond_info": (2.95e-09, 0.0e+00, 2.83e-09), "cond_path_info": (3.33e-09, 2.0e-12, 2.82e-09), "tree_est": (7.37e-12, 5.3e-15, 1.59e-11), "tree_info": (5.48e-09, 0.0e+00, 4.99e-09), "tree_w": (3.34e-19, 0.0e+00, 2.78e-19), "tree_path_info": (5.55e-09, 9.8e-12, 4.98e-09)},
    ("leaf_and_hub", "identity"): {"step": (4.02e-18, 9.6e-21, 6.64e-18), "diag": (2.30e-13, 3.8e-16, 4.50e-13), "cross": (2.31e-13, 3.4e-16, None), "joint": (2.32e-13, 2.7e-16, 4.48e-13)},
    ("leaf_and_hub", "edge_spread"): {"step": (1.12e-17, 3.0e-21, 1.20e-17), "diag": (9.24e-12, 2.1e-14, 6.49e-12), "cross": (9.24e-12, 2.1e-14, None), "joint": (9.22e-12, 2.1e-14, 6.49e-12)},
    ("leaf_and_hub", "component_spread"): {"step": (2.26e-18, 1.9e-21, 8.63e-18), "diag": (3.09e-11, 4.0e-14, 3.27e-11), "cross": (3.09e-11, 4.0e-14, None), "joint": (3.07e-11, 2.0e-14, 3.27e-11)},
    ("leaf_and_hub", "full_spread"): {"step": (1.99e-17, 7.5e-21, 8.64e-18), "diag": (2.68e-12, 8.7e-15, 7.82e-12), "cross": (2.67e-12, 8.8e-15, None), "joint": (2.67e-12, 8.7e-15, 7.82e-12)},
    ("leaf_and_hub", "heading_stiff"): {"step": (8.17e-18, 1.9e-20, 1.38e-17), "diag": (8.07e-14, 8.7e-17, 2.68e-15), "cross": (6.02e-14, 6.0e-17, None), "joint": (6.79e-14, 8.6e-17, 1.94e-15)},
    ("leaf_and_hub", "heading_soft"): {"step": (4.10e-18, 1.9e-21, 8.12e-18), "diag": (8.14e-13, 4.0e-16, 6.29e-13), "cross": (8.14e-13, 3.8e-16, None), "joint": (8.14e-13, 3.6e-16, 4.44e-14)},
    ("leaf_and_hub", "millimetres"): {"step": (5.65e-19, 9.5e-21, 2.32e-18), "diag": (3.33e-10, 2.7e-16, 5.05e-14), "cross": (3.35e-10, 2.6e-16, None), "joint": (3.31e-10, 2.1e-16, 4.40e-14)},
    ("leaf_and_hub", "far_origin"): {"step": (5.99e-14, 3.5e-21, 5.99e-14), "diag": (1.59e-13, 2.5e-16, 5.27e-13), "cross": (1.59e-13, 2.9e-16, None), "joint": (1.58e-13, 3.0e-16, 5.24e-13)},
    ("leaf_and_hub", "weak"): {"step": (4.02e-18, 9.6e-21, 6.64e-18), "diag": (2.30e-13, 3.8e-16, 4.50e-13), "cross": (2.31e-13, 3.4e-16, None), "joint": (2.32e-13, 2.7e-16, 4.48e-13)},
    ("leaf_and_hub", "strong"): {"step": (4.02e-18, 9.6e-21, 6.64e-18), "diag": (2.30e-13, 3.8e-16, 4.50e-13), "cross": (2.31e-13, 3.4e-16, None), "joint": (2.32e-13, 2.7e-16, 4.48e-13)},
    ("mixed257", "identity"): {"step": (1.80e-17, 4.8e-20, 2.38e-17), "diag": (1.35e-14, 9.7e-17, 2.14e-14), "cross": (1.32e-14, 8.3e-17, None), "joint": (1.35e-14, 7.5e-17, 2.13e-14)},
    ("mixed257", "edge_spread"): {"step": (9.24e-18, 8.7e-21, 3.56e-17), "diag": (8.84e-13, 5.6e-16, 5.55e-13), "cross": (8.84e-13, 5.9e-16, None), "joint": (8.76e-13, 5.7e-16, 5.38e-13)},
    ("mixed257", "component_spread"): {"step": (1.13e-17, 2.0e-20, 2.25e-17), "diag": (2.51e-14, 9.6e-17, 4.81e-14), "cross": (2.43e-14, 7.5e-17, None), "joint": (2.51e-14, 7.7e-17, 2.03e-14)},
    ("mixed257", "full_spread"): {"step": (1.57e-17, 2.2e-20, 2.52e-17), "diag": (1.54e-14, 7.6e-17, 1.99e-14), "cross": (1.16e-14, 6.7e-17, None), "joint": (1.07e-14, 7.5e-17, 9.90e-15)},
    ("mixed257", "heading_stiff"): {"step": (1.31e-17, 2.7e-20, 1.63e-17), "diag": (4.96e-14, 7.6e-17, 1.36e-14), "cross": (6.22e-14, 7.7e-17, None), "joint": (4.27e-14, 6.9e-17, 1.27e-14)},
    ("mixed257", "heading_soft"): {"step": (1.21e-17, 3.9e-20, 4.94e-17), "diag": (2.51e-15, 8.2e-17, 1.22e-14), "cross": (4.65e-15, 6.5e-17, None), "joint": (3.74e-15, 7.5e-17, 1.07e-14)},
    ("mixed257", "millimetres"): {"step": (1.42e-17, 4.5e-20, 2.32e-17), "diag": (1.70e-11, 7.9e-17, 2.05e-14), "cross": (1.66e-11, 7.5e-17, None), "joint": (1.71e-11, 7.9e-17, 1.95e-14)},
    ("mixed257", "far_origin"): {"step": (3.04e-13, 3.6e-20, 3.04e-13), "diag": (3.48e-15, 8.2e-17, 1.97e-14), "cross": (4.31e-15, 6.8e-17, None), "joint": (3.52e-15, 7.2e-17, 1.93e-14)},
    ("mixed257", "weak"): {"step": (1.80e-17, 4.8e-20, 2.38e-17), "diag": (1.35e-14, 9.7e-17, 2.14e-14), "cross": (1.32e-14, 8.3e-17, None), "joint": (1.35e-14, 7.5e-17, 2.13e-14)},
    ("mixed257", "strong"): {"step": (1.80e-17, 4.8e-20, 2.38e-17), "diag": (1.35e-14, 9.7e-17, 2.14e-14), "cross": (1.32e-14, 8.3e-17, None), "joint": (1.35e-14, 7.5e-17, 2.13e-14)},
    ("star5", "identity"): {"rm_est": (4.44e-16, 0.0e+00, 4.44e-16), "rm_info": (8.14e-15, 4.8e-17, 7.76e-15)},
    ("star5", "edge_spread"): {"rm_est": (4.44e-16, 0.0e+00, 4.44e-16), "rm_info": (3.26e-16, 0.0e+00, 1.05e-15)},
    ("star5", "component_spread"): {"rm_est": (4.44e-16, 0.0e+00, 4.44e-16), "rm_info": (8.09e-14, 5.7e-19, 2.09e-14)},
    ("star5", "full_spread"): {"rm_est": (4.44e-16, 0.0e+00, 4.44e-16), "rm_info": (1.21e-14, 5.2e-17, 2.72e-14)},
    ("star5", "heading_stiff"): {"rm_est": (4.44e-16, 0.0e+00, 4.44e-16), "rm_info": (3.36e-14, 1.1e-24, 1.82e-15)},
    ("star5", "heading_soft"): {"rm_est": (4.44e-16, 0.0e+00, 4.44e-16), "rm_info": (2.58e-12, 3.5e-15, 4.05e-13)},
    ("star5", "millimetres"): {"rm_est": (2.27e-13, 0.0e+00, 2.27e-13), "rm_info": (8.30e-15, 4.1e-24, 6.19e-15)},
    ("star5", "far_origin"): {"rm_est": (4.44e-16, 0.0e+00, 4.44e-16), "rm_info": (8.14e-15, 4.8e-17, 7.76e-15)},
    ("star5", "weak"): {"rm_est": (4.44e-16, 0.0e+00, 4.44e-16), "rm_info": (8.14e-15, 4.8e-17, 7.76e-15)},
    ("star5", "strong"): {"rm_est": (4.44e-16, 0.0e+00, 4.44e-16), "rm_info": (8.14e-15, 4.8e-17, 7.76e-15)},
    ("star16", "identity"): {"rm_est": (4.44e-16, 0.0e+00, 4.44e-16), "rm_info": (2.84e-14, 1.1e-16, 7.12e-14)},
    ("star16", "edge_spread"): {"rm_est": (4.44e-16, 0.0e+00, 4.44e-16), "rm_info": (1.68e-13, 1.4e-16, 5.72e-14)},
    ("star16", "component_spread"): {"rm_est": (6.66e-16, 0.0e+00, 6.66e-16), "rm_info": (2.89e-14, 3.5e-16, 3.36e-13)},
    ("star16", "full_spread"): {"rm_est": (4.44e-16, 0.0e+00, 4.44e-16), "rm_info": (3.32e-13, 7.1e-17, 1.04e-13)},
    ("star16", "heading_stiff"): {"rm_est": (4.44e-16, 0.0e+00, 4.44e-16), "rm_info": (7.60e-14, 3.8e-21, 6.78e-14)},
    ("star16", "heading_soft"): {"rm_est": (4.44e-16, 0.0e+00, 4.44e-16), "rm_info": (9.85e-12, 5.9e-14, 9.43e-12)},
    ("star16", "millimetres"): {"rm_est": (4.55e-13, 0.0e+00, 4.55e-13), "rm_info": (1.48e-13, 1.6e-16, 2.57e-14)},
    ("star16", "far_origin"): {"rm_est": (4.44e-16, 0.0e+00, 4.44e-16), "rm_info": (2.84e-14, 1.1e-16, 7.12e-14)},
    ("star16", "weak"): {"rm_est": (4.44e-16, 0.0e+00, 4.44e-16), "rm_info": (2.84e-14, 1.1e-16, 7.12e-14)},
    ("star16", "strong"): {"rm_est": (4.44e-16, 0.0e+00, 4.44e-16), "rm_info": (2.84e-14, 1.1e-16, 7.12e-14)},
}
