"""The cases of the vertex-removal tests (tests/test_remove_nodes_cpu.py proves the reference on them and checks their
preconditions; tests/test_remove_nodes_gpu.py runs the device on them).  TEST INFRASTRUCTURE ONLY.

Every case is (nV, ef, et, meas, info, remove): random measurements with headings over the full circle and random positive
definite informations from a fixed seed -- uniform informations tie the weights exactly and are not used."""
import numpy as np

import ref_numpy as R
import ref_remove_nodes as RN

MARGIN_MIN = 1e-6               # nats: every case's decision margin in the reference (no tie decides a tree)
MEAS_ATOL = 1e-12               # the new edges' measurements: the bar of the condensed-tree tests for the same arithmetic

# ||I_device - I_reference||_F / ||I_reference||_F, the largest over every new edge of every case, as first measured on an
# MI355X against this reference; the device is held to INFO_MARGIN times it (the different summation order of a 48x48 Cholesky).
INFO_GAP = 3.556e-13             # (the 300-vertex lattice; 8.4e-14 at 16 neighbours, 1.4e-15 or less at two)
INFO_MARGIN = 10.0

# The ring of 12 with one closure, its five alternate interior vertices removed (ring_case): how far the pruned graph's
# optimum lies from the full graph's at the kept vertices (the largest absolute pose component) and the KL in nats of the kept
# vertices' marginal under the full graph from the Gaussian the pruned graph implies.  Measured in the float64 reference on the
# CPU (tests/test_remove_nodes_cpu.py re-measures them); the reference is held to RING_MARGIN times each.
RING_GAP = 4.098e-4
RING_KL = 2.396e-4
RING_MARGIN = 2.0


def random_info(rng, n):
    """n random positive definite informations, upper triangles [n, 6]: A A^T + I, scaled by up to two orders of magnitude."""
    A = rng.normal(size=(n, 3, 3))
    O = (A @ A.transpose(0, 2, 1) + np.eye(3)) * (10.0 ** rng.uniform(0, 2, size=n))[:, None, None]
    return np.stack([O[:, 0, 0], O[:, 0, 1], O[:, 0, 2], O[:, 1, 1], O[:, 1, 2], O[:, 2, 2]], axis=1)


def random_meas(rng, n):
    return np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(-np.pi, np.pi, n)], axis=1)


def star(degree, seed, forward=None, parallel=0):
    """Vertex v = 20 among 40 with ``degree`` neighbours drawn on both sides of it, its edges in a shuffled (unsorted) order;
    forward [degree] (default random): edge k stored v -> n.  parallel: that many more edges to neighbours already joined, each
    stored n -> v in FRONT of the list, so that the lower-index copy points n -> v."""
    rng = np.random.default_rng(seed)
    nV, v = 40, 20
    nb = rng.permutation(np.delete(np.arange(nV), v))[:degree]
    fw = rng.integers(0, 2, degree).astype(bool) if forward is None else np.asarray(forward, dtype=bool)
    ef, et = np.where(fw, v, nb), np.where(fw, nb, v)
    if parallel:
        dup = nb[:parallel]
        ef, et = np.concatenate([dup, ef]), np.concatenate([np.full(parallel, v), et])
    n = len(ef)
    return nV, ef.astype(np.int32), et.astype(np.int32), random_meas(rng, n), random_info(rng, n), np.array([v], dtype=np.int32)


def lattice(rows=36, cols=36, n_remove=300, seed=7, drop=0.2):
    """A 2-D lattice with both diagonals, a fifth of the edges dropped at random (degrees 0 to 8), edges in random direction;
    removed: the first n_remove vertices with even row and column -- no two of them adjacent."""
    rng = np.random.default_rng(seed)
    idx = np.arange(rows * cols).reshape(rows, cols)
    pairs = np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], 1), np.stack([idx[:-1].ravel(), idx[1:].ravel()], 1),
                            np.stack([idx[:-1, :-1].ravel(), idx[1:, 1:].ravel()], 1), np.stack([idx[:-1, 1:].ravel(), idx[1:, :-1].ravel()], 1)])
    pairs = pairs[rng.permutation(len(pairs))]
    pairs = pairs[rng.uniform(size=len(pairs)) >= drop]
    flip = rng.integers(0, 2, len(pairs)).astype(bool)
    ef, et = np.where(flip, pairs[:, 1], pairs[:, 0]), np.where(flip, pairs[:, 0], pairs[:, 1])
    remove = idx[::2, ::2].ravel()[:n_remove]
    n = len(ef)
    return rows * cols, ef.astype(np.int32), et.astype(np.int32), random_meas(rng, n), random_info(rng, n), remove.astype(np.int32)


def singular():
    """Degree 4; the edge to one neighbour that is not the lowest is stored v -> n with information diag(a, b, 0): the heading
    of that neighbour is not observed, its row of H is exactly zero and the factorisation stops at a zero pivot."""
    nV, ef, et, meas, info, remove = star(4, 105, forward=[True] * 4)
    k = int(np.argmax(et))
    info[k] = [3.0, 0.0, 0.0, 5.0, 0.0, 0.0]
    return nV, ef, et, meas, info, remove


def not_independent():
    """Two removed vertices joined by an edge: refused."""
    nV, ef, et, meas, info, remove = star(3, 106)
    return nV, ef, et, meas, info, np.array([remove[0], et[0] if ef[0] == remove[0] else ef[0]], dtype=np.int32)


# name -> builder.  The four direction combinations of degree 2; the degrees at which the kernel takes another path (one
# round of pair weights up to 11 neighbours, two from 12; the limit and one past it); a parallel edge whose lower copy points
# n -> v; 300 workgroups in one call.
CASES = {
    "deg0": lambda: (40, np.array([1], np.int32), np.array([2], np.int32), random_meas(np.random.default_rng(1), 1),
                     random_info(np.random.default_rng(1), 1), np.array([20], np.int32)),
    "deg1": lambda: star(1, 101),
    "deg2_ff": lambda: star(2, 110, forward=[True, True]),
    "deg2_fb": lambda: star(2, 111, forward=[True, False]),
    "deg2_bf": lambda: star(2, 112, forward=[False, True]),
    "deg2_bb": lambda: star(2, 113, forward=[False, False]),
    "deg3": lambda: star(3, 103),
    "deg5": lambda: star(5, 104),
    "deg12": lambda: star(12, 120),
    "deg15": lambda: star(15, 115),
    "deg16": lambda: star(16, 116),
    "deg17": lambda: star(17, 117),
    "unsorted": lambda: star(6, 140),
    "parallel": lambda: star(4, 130, parallel=2),
    "lattice300": lambda: lattice(),
    "singular": singular,
}
FLAGS = {"deg17": 2, "singular": 1}       # every other case: flag 0 throughout

_CASE, _REF = {}, {}


def case(name):
    if name not in _CASE:
        _CASE[name] = CASES[name]()
    return _CASE[name]


def reference(name):
    """ref_remove_nodes.remove_nodes on a case, computed once and shared (never modified)."""
    if name not in _REF:
        _REF[name] = RN.remove_nodes(*case(name))
    return _REF[name]


# ------------------------------------------------------------------------------------------- chain and ring
def noisy_walk(n, seed, closure=False):
    """n poses on a regular n-gon walked with unit-ish steps, odometry k -> k + 1 (and the closure n - 1 -> 0) measured with
    noise, random informations: (poses [n, 3] the noisy start, fixed, ef, et, meas, info)."""
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(n) / n
    truth = np.stack([2 * np.cos(ang), 2 * np.sin(ang), R.normalize_theta(ang + np.pi / 2)], axis=1)
    ef = np.arange(n - 1 + int(closure), dtype=np.int32)
    et = ((ef + 1) % n).astype(np.int32)
    meas = R._se2_mul(R._se2_inv(truth[ef]), truth[et]) + rng.normal(scale=[0.05, 0.05, 0.02], size=(len(ef), 3))
    meas[:, 2] = R.normalize_theta(meas[:, 2])
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    poses = truth + rng.normal(scale=0.02, size=truth.shape)
    poses[0] = truth[0]
    return poses, fixed, ef, et, meas, random_info(rng, len(ef))


def chain_case():
    """A chain of 12, every second interior vertex removed."""
    return noisy_walk(12, 201), np.array([1, 3, 5, 7, 9], dtype=np.int32)


def ring_case():
    """A ring of 12 (the chain and the closure 11 -> 0), its five alternate interior vertices removed."""
    return noisy_walk(12, 202, closure=True), np.array([1, 3, 5, 7, 9], dtype=np.int32)


def optimum(poses, fixed, ef, et, meas, info, iters=30):
    """The float64 Gauss-Newton optimum (ref_numpy.gn_optimize, far past convergence; a vertex without an edge stays)."""
    return R.gn_optimize(poses, R.active_fixed(len(poses), fixed, ef, et), ef, et, meas, info, iters)[0]
