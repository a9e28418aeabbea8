"""Float64 numpy reference for the pairwise consistency maximisation of closure candidates (cgmr_closure_consistency,
cgmr_max_clique_greedy).  TEST INFRASTRUCTURE ONLY; shares no code with the device.

A candidate k = (a_k, b_k, z_k, Omega_k) measures x_a^-1 x_b.  For l < k the loop residual is

    eps_kl = z_k (+) (x_bk^-1 (+) x_bl) (+) z_l^-1 (+) (x_al^-1 (+) x_ak)

and S_kl = J_x Sigma J_x^T + J_zk Omega_k^-1 J_zk^T + J_zl Omega_l^-1 J_zl^T, d2 = eps^T S^-1 eps.  The Jacobians are carried
through the expression by forward accumulation: every intermediate pose holds its derivatives with respect to the six inputs,
and compose / inverse push them on with their own analytic derivatives (the chain rule, node by node)."""
import numpy as np

import ref_joint_marginals as J

GAMMA_99 = 11.344866730144373          # chi2.ppf(0.99, 3)
INPUTS = ("ak", "bk", "al", "bl", "zk", "zl")


# ------------------------------------------------------------------------------------------- SE(2)
def norm_theta(t):
    """theta into (-pi, pi]."""
    t = float(t)
    if -np.pi < t <= np.pi:
        return t
    return t - 2 * np.pi * np.ceil((t - np.pi) / (2 * np.pi))


def compose(a, b):
    c, s = np.cos(a[2]), np.sin(a[2])
    return np.array([a[0] + c * b[0] - s * b[1], a[1] + s * b[0] + c * b[1], norm_theta(a[2] + b[2])])


def inverse(a):
    c, s = np.cos(a[2]), np.sin(a[2])
    return np.array([-(c * a[0] + s * a[1]), -(-s * a[0] + c * a[1]), norm_theta(-a[2])])


def d_compose(a, b):
    """(d(a (+) b) / da, d(a (+) b) / db) for additive (x, y, theta) updates."""
    c, s = np.cos(a[2]), np.sin(a[2])
    da = np.array([[1.0, 0.0, -s * b[0] - c * b[1]], [0.0, 1.0, c * b[0] - s * b[1]], [0.0, 0.0, 1.0]])
    db = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return da, db


def d_inverse(a):
    c, s = np.cos(a[2]), np.sin(a[2])
    # x' = -c x - s y,  y' = s x - c y,  theta' = -theta
    return np.array([[-c, -s, s * a[0] - c * a[1]], [s, -c, c * a[0] + s * a[1]], [0.0, 0.0, -1.0]])


# ------------------------------------------------------------------------------------------- the loop
def loop_residual(xak, xbk, xal, xbl, zk, zl):
    t2 = compose(inverse(xbk), xbl)
    t4 = compose(inverse(xal), xak)
    return compose(compose(compose(zk, t2), inverse(zl)), t4)


class _Node:
    def __init__(self, val, jac):
        self.val, self.jac = np.asarray(val, dtype=np.float64), jac


def _mul(A, B):
    da, db = d_compose(A.val, B.val)
    jac = {}
    for n in set(A.jac) | set(B.jac):
        jac[n] = (da @ A.jac[n] if n in A.jac else 0.0) + (db @ B.jac[n] if n in B.jac else 0.0)
    return _Node(compose(A.val, B.val), jac)


def _inv(A):
    d = d_inverse(A.val)
    return _Node(inverse(A.val), {n: d @ j for n, j in A.jac.items()})


def loop_jacobians(xak, xbk, xal, xbl, zk, zl):
    """(eps, {name: d eps / d input}) for the inputs ``INPUTS``, each taken as a variable of its own (a vertex that two roles
    share gets the sum of its roles' Jacobians from the caller -- or, equivalently, identical rows in Sigma)."""
    leaf = {n: _Node(v, {n: np.eye(3)}) for n, v in zip(INPUTS, (xak, xbk, xal, xbl, zk, zl))}
    t2 = _mul(_inv(leaf["bk"]), leaf["bl"])
    t4 = _mul(_inv(leaf["al"]), leaf["ak"])
    e = _mul(_mul(_mul(leaf["zk"], t2), _inv(leaf["zl"])), t4)
    return e.val, e.jac


def info_full(u):
    return np.array([[u[0], u[1], u[2]], [u[1], u[3], u[4]], [u[2], u[4], u[5]]], dtype=np.float64)


def pair_terms(Sigma12, xak, xbk, xal, xbl, zk, zl, info_k, info_l):
    """(eps, S, scale): Sigma12 the joint covariance of (x_ak, x_bk, x_al, x_bl) in that order; scale = the sum over the 16
    block terms of ||J_i|| ||J_j|| ||Sigma_ij|| (Frobenius), the size of what S is added up from."""
    eps, jac = loop_jacobians(xak, xbk, xal, xbl, zk, zl)
    Jx = np.hstack([jac[n] for n in INPUTS[:4]])
    with np.errstate(all="ignore"):
        S = Jx @ Sigma12 @ Jx.T + jac["zk"] @ np.linalg.inv(info_full(info_k)) @ jac["zk"].T \
            + jac["zl"] @ np.linalg.inv(info_full(info_l)) @ jac["zl"].T
    scale = 0.0
    for i in range(4):
        for j in range(4):
            scale += np.linalg.norm(jac[INPUTS[i]]) * np.linalg.norm(jac[INPUTS[j]]) * np.linalg.norm(Sigma12[3 * i:3 * i + 3, 3 * j:3 * j + 3])
    return eps, S, scale


def pair_d2(Sigma12, xak, xbk, xal, xbl, zk, zl, info_k, info_l):
    """eps^T S^-1 eps; NaN where S is not finite or not positive definite."""
    eps, S, _ = pair_terms(Sigma12, xak, xbk, xal, xbl, zk, zl, info_k, info_l)
    S = 0.5 * (S + S.T)
    if not np.all(np.isfinite(S)) or np.linalg.eigvalsh(S).min() <= 0:
        return np.nan
    return float(eps @ np.linalg.solve(S, eps))


def gather12(Sq, idx):
    """The 12x12 joint covariance of the four query positions ``idx`` out of a joint matrix in query order."""
    rows = np.concatenate([np.arange(3 * i, 3 * i + 3) for i in idx])
    return Sq[np.ix_(rows, rows)]


def consistency_from_joint(Sq, pos_a, pos_b, poses, ca, cb, cmeas, cinfo):
    """d2 [N, N] from a joint covariance ``Sq`` of some query list in which closure k's ends sit at pos_a[k], pos_b[k]."""
    N = len(ca)
    d2 = np.zeros((N, N))
    for k in range(N):
        for l in range(k):
            S12 = gather12(Sq, (pos_a[k], pos_b[k], pos_a[l], pos_b[l]))
            d2[k, l] = d2[l, k] = pair_d2(S12, poses[ca[k]], poses[cb[k]], poses[ca[l]], poses[cb[l]], cmeas[k], cmeas[l],
                                          cinfo[k], cinfo[l])
    return d2


def unique_endpoints(ca, cb):
    """(unique vertices in order of first appearance, position of every a, of every b)."""
    uq, where = [], {}
    for v in np.stack([ca, cb], axis=1).reshape(-1):
        if int(v) not in where:
            where[int(v)] = len(uq)
            uq.append(int(v))
    return np.array(uq, dtype=np.int32), [where[int(v)] for v in ca], [where[int(v)] for v in cb]


def consistency_dense(poses, fixed, ef, et, meas, info, ca, cb, cmeas, cinfo):
    """d2 [N, N] on the dense inverse of H (ref_joint_marginals.joint_dense over the unique endpoints)."""
    uq, pa, pb = unique_endpoints(ca, cb)
    Sq = J.joint_dense(poses, fixed, ef, et, meas, info, uq)
    return consistency_from_joint(Sq, pa, pb, np.asarray(poses, dtype=np.float64), ca, cb, np.asarray(cmeas, dtype=np.float64),
                                  np.asarray(cinfo, dtype=np.float64))


def adjacency(d2, gamma=GAMMA_99):
    with np.errstate(invalid="ignore"):
        A = d2 < gamma
    A = A & ~np.eye(len(d2), dtype=bool)
    return A


# ------------------------------------------------------------------------------------------- cliques
def greedy_clique(A):
    """(members ascending, size, seed): from every seed s, C = {s}, P = A[s]; while P is not empty the u in P with the largest
    |A[u] & P| (ties: lowest index) joins C and P &= A[u].  The largest C over the seeds, ties to the lowest seed."""
    A = np.asarray(A, dtype=bool)
    n = len(A)
    best, best_seed = [], -1
    for s in range(n):
        C, P = [s], A[s].copy()
        while P.any():
            idx = np.flatnonzero(P)
            u = int(idx[np.argmax((A[idx] & P).sum(axis=1))])      # (argmax: the first of equals, idx ascending)
            C.append(u)
            P &= A[u]
        if len(C) > len(best):
            best, best_seed = C, s
    return sorted(best), len(best), best_seed


def max_clique_exact(A):
    """A maximum clique (members ascending) by Bron-Kerbosch with pivoting; for n <= 20."""
    A = np.asarray(A, dtype=bool)
    n = len(A)
    assert n <= 20
    nb = [set(np.flatnonzero(A[v]).tolist()) - {v} for v in range(n)]
    best = []

    def rec(Rs, P, X):
        nonlocal best
        if not P and not X:
            if len(Rs) > len(best):
                best = sorted(Rs)
            return
        if len(Rs) + len(P) <= len(best):
            return
        piv = max(P | X, key=lambda v: len(P & nb[v]))
        for v in sorted(P - nb[piv]):
            rec(Rs + [v], P & nb[v], X & nb[v])
            P = P - {v}
            X = X | {v}

    rec([], set(range(n)), set())
    return best


def random_graph(n, p, rng):
    U = np.triu(rng.random((n, n)) < p, 1)
    return U | U.T


def planted_clique(n, p, members, rng):
    A = random_graph(n, p, rng)
    m = np.asarray(members)
    A[np.ix_(m, m)] = True
    A[np.arange(n), np.arange(n)] = False
    return A


def two_triangles():
    """Triangles {0, 2, 4} and {1, 3, 5}: every seed finds its own triangle, the tie goes to seed 0."""
    A = np.zeros((6, 6), dtype=bool)
    for t in ((0, 2, 4), (1, 3, 5)):
        for i in t:
            for j in t:
                A[i, j] = i != j
    return A
