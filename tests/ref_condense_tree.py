"""Float64 numpy reference of the condensed graph as a spanning tree of relative poses (include/cgmr.h: cgmr_condense_tree,
cgmr_min_spanning_tree).  TEST INFRASTRUCTURE ONLY, written from the definitions:

  the gauge alone fixed, the spanning-tree guess (ref_robust_marginals.guess_bfs) and one Gauss-Newton step
  (ref_numpy.gn_optimize), as ref_numpy.condense_ref takes them;
  the blocks of H^-1 at the guess from ref_joint_marginals.joint_dense / joint_refined;
  the weight of a pair of nodes w(a, b) = log det of ref_joint_marginals.relative_cov at the stepped poses, a < b;
  the tree by Kruskal with union-find over the edges sorted by (w, max(a, b), min(a, b)) -- not the device's Prim;
  the labels: ref_numpy.label_edges_ut (7 points) where the parent is the gauge, `label_ut13` below otherwise, and a
  first-order labelling (the relative-pose covariance rotated into the edge's error frame) for the cases that have a closed form.

The nodes are the gauge (node 0) and the unique requested vertices other than it (nodes 1 .. nq, in order of first appearance)."""
import numpy as np

import ref_joint_marginals as J
import ref_numpy as R
import ref_robust_marginals as RM


# ------------------------------------------------------------------------------------------- the tree
def kruskal(W, root=0, enumeration=None):
    """parent [n] (parent[root] = -1) of the minimum spanning tree of the dense symmetric W under the total order
    (w, max(a, b), min(a, b)); only the lower triangle is read, a NaN counts as +inf.  enumeration: a permutation of the
    n (n - 1) / 2 candidate edges, the order they are listed in before they are sorted (the keys are distinct: no effect)."""
    W = np.asarray(W, dtype=np.float64)
    n = W.shape[0]
    a, b = np.tril_indices(n, -1)                                  # a > b
    if enumeration is not None:
        a, b = a[enumeration], b[enumeration]
    w = W[a, b].copy()
    w[np.isnan(w)] = np.inf
    order = np.lexsort((b, a, w))                                  # by w, then max = a, then min = b
    comp = list(range(n))

    def find(x):
        while comp[x] != x:
            comp[x] = comp[comp[x]]
            x = comp[x]
        return x

    adj = [[] for _ in range(n)]
    left = n - 1
    for k in order:
        if left == 0:
            break
        ra, rb = find(int(a[k])), find(int(b[k]))
        if ra != rb:
            comp[ra] = rb
            adj[int(a[k])].append(int(b[k]))
            adj[int(b[k])].append(int(a[k]))
            left -= 1
    parent = np.full(n, -1, dtype=np.int32)
    seen = np.zeros(n, dtype=bool)
    seen[root] = True
    stack = [int(root)]
    while stack:
        u = stack.pop()
        for v in adj[u]:
            if not seen[v]:
                seen[v] = True
                parent[v] = u
                stack.append(v)
    assert seen.all()
    return parent


def tree_path_max(W, parent, a, b):
    """The largest weight on the tree path between nodes a and b."""
    def up(x):
        out = [x]
        while parent[out[-1]] >= 0:
            out.append(int(parent[out[-1]]))
        return out
    pa, pb = up(a), up(b)
    while len(pa) > 1 and len(pb) > 1 and pa[-2] == pb[-2]:        # drop the shared part above the meeting node
        pa.pop(); pb.pop()
    m = -np.inf
    for path in (pa, pb):
        for x, y in zip(path[:-1], path[1:]):
            m = max(m, W[x, y])
    return m


def decision_margin(W, parent):
    """min over the pairs not in the tree of w(pair) - the largest weight on the tree path between its ends: how far the
    weights may move before another tree is the minimum one."""
    n = W.shape[0]
    best = np.inf
    for a in range(n):
        for b in range(a):
            if parent[a] == b or parent[b] == a:
                continue
            best = min(best, W[a, b] - tree_path_max(W, parent, a, b))
    return best


# ------------------------------------------------------------------------------------------- the numeric half
def nodes_of(gauge, query):
    nodes = [int(gauge)]
    for v in query:
        if int(v) not in nodes:
            nodes.append(int(v))
    return np.array(nodes, dtype=np.int32)


def node_block(Sigma, a, b):
    """The 3x3 block of nodes (a, b) of the joint covariance [3 nq, 3 nq] of nodes 1 .. nq; node 0 (the gauge): zeros."""
    if a == 0 or b == 0:
        return np.zeros((3, 3))
    return Sigma[3 * (a - 1):3 * a, 3 * (b - 1):3 * b]


def logdet_chol(S):
    """log det S from the Cholesky factor; +inf without one."""
    S = 0.5 * (S + S.T)
    if not np.all(np.isfinite(S)):
        return np.inf
    try:
        L = np.linalg.cholesky(S)
    except np.linalg.LinAlgError:
        return np.inf
    return float(2.0 * np.log(np.diag(L)).sum())


def weights(poses, nodes, Sigma):
    """W [n, n]: w(a, b) = log det of the first-order covariance of x_a^-1 x_b, a < b; +inf on the diagonal and for every pair
    of a node other than the gauge whose covariance is zero.  Returns (W, Sz)
    with Sz[a, b] = Sz[b, a] the covariance itself (of x_a^-1 x_b, a < b)."""
    n = len(nodes)
    full = np.zeros((3 * n, 3 * n), dtype=np.asarray(Sigma).dtype)  # node 0, the gauge: zero rows and columns
    full[3:, 3:] = Sigma
    B = full.reshape(n, 3, n, 3).transpose(0, 2, 1, 3)             # B[a, b] = the block of nodes (a, b)
    a, b = np.triu_indices(n, 1)                                   # a < b
    x = np.asarray(poses, dtype=np.float64)[np.asarray(nodes)]
    S = J.relative_cov(x[a], x[b], B[a, a], B[a, b], B[b, b])
    W = np.full((n, n), np.inf)
    Sz = np.zeros((n, n, 3, 3))
    Sz[a, b] = Sz[b, a] = S
    W[a, b] = W[b, a] = [logdet_chol(np.asarray(Sk, dtype=np.float64)) for Sk in S]
    # a requested vertex without a covariance (no edge touches it: zero rows of H^-1) has no finite weight
    dead = np.array([k > 0 and not B[k, k].any() for k in range(n)])
    W[dead, :] = np.inf
    W[:, dead] = np.inf
    return W, Sz


def label_ut13(xp, xc, S6, alpha=1e-3, beta=2.0):
    """g2o's EdgeLabeler on an edge xp -> xc with two free ends: z := xp^-1 xc; sampleUnscented at dimension 6 (lambda = alpha^2 6):
    L = chol((6 + lambda) S6), S6 the joint covariance of (xp, xc), the 13 points 0, +-L[:, i], each applied to both vertices
    by the additive (x, y, theta) update with normalised theta; the edge error e = z^-1 (xp'^-1 xc'), its weighted mean and
    covariance, information = covariance^-1.  Returns (z [3], info_upper [6], not_pd)."""
    xp, xc = np.asarray(xp, dtype=np.float64), np.asarray(xc, dtype=np.float64)
    n = 6
    lam = alpha * alpha * n
    wm = np.full(2 * n + 1, 1.0 / (2 * (n + lam)))
    wc = wm.copy()
    wm[0] = lam / (n + lam)
    wc[0] = wm[0] + (1 - alpha * alpha + beta)
    z = R._se2_mul(R._se2_inv(xp), xc)
    try:
        L = np.linalg.cholesky((n + lam) * 0.5 * (S6 + S6.T))
    except np.linalg.LinAlgError:
        return z, np.array([1.0, 0, 0, 1, 0, 1]), True
    pts = np.concatenate([np.zeros((1, 6)), np.stack([s * L[:, i] for i in range(n) for s in (1.0, -1.0)])])
    P = np.concatenate([xp + pts[:, :3], xc + pts[:, 3:]])
    P[:, 2] = R.normalize_theta(P[:, 2])
    e = R.edge_errors(P, np.arange(13), 13 + np.arange(13), np.tile(z, (13, 1)))
    mean = wm @ e
    dev = e - mean
    C = (wc[:, None, None] * dev[:, :, None] * dev[:, None, :]).sum(axis=0)
    I = np.linalg.inv(C)
    return z, np.array([I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]]), False


def _inv3_adjugate(C):
    """The inverse of a 3x3 by its adjugate, in C's own precision (np.linalg.inv has no long double)."""
    a, b, c, d, e, f, g, h, i = C.ravel()
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    return np.array([[e * i - f * h, c * h - b * i, b * f - c * e], [f * g - d * i, a * i - c * g, c * d - a * f],
                     [d * h - e * g, b * g - a * h, a * e - b * d]], dtype=C.dtype) / det


def joint_extended(poses, fixed, ef, et, meas, info, query):
    """ref_joint_marginals.joint_dense with the inverse of H taken in long double (Gauss-Jordan on the dense matrix; H is
    positive definite: no pivoting): the joint covariance [3 nK, 3 nK] as a long double array.  For the cases whose closed form
    is known to more digits than a float64 inverse of H leaves."""
    H, hidx = J._system(poses, fixed, ef, et, meas, info)
    A = H.toarray().astype(np.longdouble)
    n = A.shape[0]
    X = np.eye(n, dtype=np.longdouble)
    for k in range(n):
        piv = A[k, k]
        A[k], X[k] = A[k] / piv, X[k] / piv
        col = A[:, k].copy()
        col[k] = 0
        A -= col[:, None] * A[k][None, :]
        X -= col[:, None] * X[k][None, :]
    nK = len(query)
    out = np.zeros((3 * nK, 3 * nK), dtype=np.longdouble)
    for k, vk in enumerate(query):
        for l, vl in enumerate(query):
            if hidx[vk] >= 0 and hidx[vl] >= 0:
                out[3 * k:3 * k + 3, 3 * l:3 * l + 3] = X[3 * hidx[vk]:3 * hidx[vk] + 3, 3 * hidx[vl]:3 * hidx[vl] + 3]
    return out


def label_first_order(xp, xc, Sz):
    """The first-order label: z := xp^-1 xc, information = (J_e Sigma_z J_e^T)^-1 with J_e = R(z.theta)^T (+) 1 the rotation of
    the relative pose's covariance into the edge's error frame."""
    z = J.relative_pose(xp, xc)
    _, Je = J.hypothesis_error(z, z)
    C = Je @ Sz @ Je.T
    I = _inv3_adjugate(C) if C.dtype == np.longdouble else np.linalg.inv(C)
    I = np.asarray(0.5 * (I + I.T), dtype=np.float64)
    return z, np.array([I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]])


def prepare(poses, ef, et, meas, info, gauge, query, refined=False):
    """The numeric front half: nodes, the spanning-tree guess from the gauge, the poses after one step from it, the joint
    covariance of nodes 1 .. nq at the guess (refined: True, refined columns of H^-1 with their own error estimate; False, the
    dense inverse; "extended", the dense inverse in long double, which the first-order labels then keep up to their 3x3 inverse)."""
    nV = len(poses)
    fixed = np.zeros(nV, np.uint8)
    fixed[gauge] = 1
    nodes = nodes_of(gauge, query)
    guess = RM.guess_bfs(poses, fixed, ef, et, meas)
    fx = R.active_fixed(nV, fixed, ef, et)
    poses1, _ = R.gn_optimize(guess, fx, ef, et, meas, info, 1)
    a = (guess, fixed, ef, et, meas, info, nodes[1:])
    if refined == "extended":
        Sigma, err = joint_extended(*a), None
    else:
        Sigma, err = J.joint_refined(*a) if refined else (J.joint_dense(*a), None)
    return dict(nodes=nodes, gauge=int(gauge), guess=guess, poses1=poses1, Sigma=Sigma, Sigma_err=err)


def edges_of(ref, parent, Sigma=None, poses=None, labels="ut", weight=None):
    """The labelled edges parent[k] -> k of nodes k = 1 .. nq at `poses` (default: the reference's stepped poses) under the
    joint covariance `Sigma` (default: the reference's): a dict of from, to (vertex indices), est, iu, flags (1: unlabelled,
    identity information; 2: the chosen weight, `weight` [nq] where given, is +inf, identity information).  labels: "ut" (7
    points from the gauge, 13 otherwise) or "first" (first order)."""
    nodes = ref["nodes"]
    Sigma = ref["Sigma"] if Sigma is None else Sigma
    poses = ref["poses1"] if poses is None else poses
    nq = len(nodes) - 1
    fr, to = np.zeros(nq, np.int32), np.zeros(nq, np.int32)
    est, iu, fl = np.zeros((nq, 3)), np.zeros((nq, 6)), np.zeros(nq, np.int32)
    for k in range(1, nq + 1):
        p = int(parent[k])
        xp, xc = poses[nodes[p]], poses[nodes[k]]
        fr[k - 1], to[k - 1] = nodes[p], nodes[k]
        Spp, Spc, Scc = node_block(Sigma, p, p), node_block(Sigma, p, k), node_block(Sigma, k, k)
        if weight is not None and not np.isfinite(weight[k - 1]):  # hung on the tree by no finite weight: unlabelled
            est[k - 1], iu[k - 1], fl[k - 1] = J.relative_pose(xp, xc), [1.0, 0, 0, 1, 0, 1], 2
        elif labels == "first":
            est[k - 1], iu[k - 1] = label_first_order(xp, xc, J.relative_cov(xp, xc, Spp, Spc, Scc))
        elif p == 0:
            z, i7, bad = R.label_edges_ut(xp, xc[None], Scc[None])
            est[k - 1], iu[k - 1], fl[k - 1] = z[0], i7[0], int(bad[0])
        else:
            est[k - 1], iu[k - 1], bad = label_ut13(xp, xc, np.block([[Spp, Spc], [Spc.T, Scc]]))
            fl[k - 1] = int(bad)
    return dict(fr=fr, to=to, est=est, iu=iu, flags=fl)


def condense_tree(poses, ef, et, meas, info, gauge, query, refined=False, labels="ut"):
    """cgmr_condense_tree restated.  Returns prepare()'s dict plus W, parent, weight (the chosen edges' w) and the edges of
    the tree (`tree`) and of the star on the gauge (`star`), both labelled the same way."""
    ref = prepare(poses, ef, et, meas, info, gauge, query, refined)
    n = len(ref["nodes"])
    ref["W"], ref["Sz"] = weights(ref["poses1"], ref["nodes"], ref["Sigma"])
    ref["parent"] = kruskal(ref["W"])
    ref["weight"] = np.array([ref["W"][k, ref["parent"][k]] for k in range(1, n)])
    ref["tree"] = edges_of(ref, ref["parent"], labels=labels, weight=ref["weight"])
    ref["star"] = edges_of(ref, np.r_[-1, np.zeros(n - 1, np.int32)], labels=labels)
    return ref


# ------------------------------------------------------------------------------------------- how good a condensed graph is
def implied_information(poses, nodes, fr, to, est, iu):
    """The information [3 nq, 3 nq], in node order, of the Gaussian the condensed edges imply over nodes 1 .. nq with the
    gauge fixed: ref_numpy.build_system on the graph of the nodes alone, linearised at `poses` (where the edges' errors are
    zero when est was read off them)."""
    nodes = np.asarray(nodes)
    idx = {int(v): k for k, v in enumerate(nodes)}
    ef = np.array([idx[int(v)] for v in fr], dtype=np.int32)
    et = np.array([idx[int(v)] for v in to], dtype=np.int32)
    fixed = np.zeros(len(nodes), np.uint8)
    fixed[0] = 1
    H, _, hidx = R.build_system(np.asarray(poses, dtype=np.float64)[nodes], fixed, ef, et, np.asarray(est, dtype=np.float64),
                                np.asarray(iu, dtype=np.float64))
    assert np.array_equal(hidx[1:], np.arange(len(nodes) - 1))
    return H.toarray()


def kl(Sigma, Lam):
    """KL( N(0, Sigma) || N(0, Lam^-1) ) in nats: (tr(Lam Sigma) - k - log det(Lam Sigma)) / 2."""
    k = Sigma.shape[0]
    s1, l1 = np.linalg.slogdet(Sigma)
    s2, l2 = np.linalg.slogdet(Lam)
    assert s1 > 0 and s2 > 0
    return 0.5 * (np.trace(Lam @ Sigma) - k - (l1 + l2))


def kl_of_edges(ref, edges, Sigma=None, poses=None):
    """KL( the joint marginal of the requested vertices given the gauge || the Gaussian the edges imply )."""
    poses = ref["poses1"] if poses is None else poses
    Lam = implied_information(poses, ref["nodes"], edges["fr"], edges["to"], edges["est"], edges["iu"])
    return kl(np.asarray(ref["Sigma"] if Sigma is None else Sigma, dtype=np.float64), Lam)
