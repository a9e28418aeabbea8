"""Float64 reference of the robust marginals and condensed graphs (include/cgmr.h: cgmr_marginals_robust,
cgmr_marginals_all_robust, cgmr_covariance_estimate_robust, cgmr_condense_robust; the robot graph's
cgmr_graph_set_condensed_robust).

g2o's computeMarginals inverts the H of the last buildSystem, robust weights included [g2o-recalled]: the H here is
ref_numpy.build_system with every edge's information scaled by rho1 (ref_robust.scaled_info) at the linearisation point of
the H that is inverted --
  marginals / marginals_all             the poses given;
  covariance_estimate / condense        the spanning-tree initial guess the one Gauss-Newton iteration starts from (the
                                        gauge alone fixed); the same scaled H drives that iteration's step.
The condensed labelling is ref_numpy.condense_ref's on the scaled information.  ``initial_guess`` is a callable with
oracle.initial_guess's signature (poses, fixed, ef, et, meas) -> poses, as ref_numpy.condense_ref takes it; ``guess_bfs`` below
is a numpy one for tests that do not load the oracle."""
import numpy as np

import ref_numpy as R
import ref_robust as RR


def guess_bfs(poses, fixed, ef, et, meas):
    """SparseOptimizer::computeInitialGuess with unit edge cost: breadth-first from the fixed vertices over the edges, each
    vertex's incident edges in list order, x_to = x_from z or x_from = x_to z^-1 (libm arithmetic)."""
    x = np.array(poses, dtype=np.float64, copy=True)
    nV = len(x)
    inc = [[] for _ in range(nV)]
    for k in range(len(ef)):
        inc[int(ef[k])].append(k)
        inc[int(et[k])].append(k)
    seen = np.zeros(nV, dtype=bool)
    queue = [v for v in range(nV) if fixed[v] and inc[v]]
    seen[queue] = True
    qh = 0
    while qh < len(queue):
        u = queue[qh]
        qh += 1
        for k in inc[u]:
            w = int(et[k]) if int(ef[k]) == u else int(ef[k])
            if seen[w]:
                continue
            seen[w] = True
            z = np.asarray(meas[k], dtype=np.float64)
            if int(ef[k]) != u:
                z = R._se2_inv(z)
            x[w] = R._se2_mul(x[u], z)
            queue.append(w)
    return x


def spanning_tree_edges(nV, fixed, ef, et):
    """The edges guess_bfs (and the library's spanning-tree guess) walks: the breadth-first tree from the fixed vertices."""
    inc = [[] for _ in range(nV)]
    for k in range(len(ef)):
        inc[int(ef[k])].append(k)
        inc[int(et[k])].append(k)
    seen = np.zeros(nV, dtype=bool)
    queue = [v for v in range(nV) if fixed[v] and inc[v]]
    seen[queue] = True
    tree, qh = [], 0
    while qh < len(queue):
        u = queue[qh]
        qh += 1
        for k in inc[u]:
            w = int(et[k]) if int(ef[k]) == u else int(ef[k])
            if not seen[w]:
                seen[w] = True
                tree.append(k)
                queue.append(w)
    return np.array(tree, dtype=np.int64)


def _guess(poses, gauge, ef, et, meas, initial_guess):
    fixed = np.zeros(len(poses), np.uint8)
    fixed[gauge] = 1
    return np.asarray(initial_guess(poses, fixed, ef, et, meas), dtype=np.float64), fixed


def marginals(poses, fixed, ef, et, meas, info, kind, delta, query):
    """cgmr_marginals_robust: the 3x3 blocks of H^-1 for ``query`` (ref_numpy.marginal_blocks_ref, refined), H at ``poses``
    with the information scaled by rho1 there.  Returns (blocks [nq,3,3], their error estimates [nq], weights [nE])."""
    p = np.asarray(poses, dtype=np.float64)
    w = RR.weights(p, ef, et, meas, info, kind, delta)
    fx = R.active_fixed(len(p), fixed, ef, et)
    H, _, hidx = R.build_system(p, fx, ef, et, meas, np.asarray(info, dtype=np.float64) * w[:, None])
    blocks, err = R.marginal_blocks_ref(H, hidx, np.asarray(query))
    return blocks, err, w


def covariance_estimate(poses, ef, et, meas, info, kind, delta, gauge, query, initial_guess):
    """cgmr_covariance_estimate_robust: the gauge alone fixed, H at the spanning-tree guess with rho1 taken there.  Returns
    (blocks [nq,3,3], error estimates [nq], weights [nE], the guess)."""
    guess, fixed = _guess(poses, gauge, ef, et, meas, initial_guess)
    blocks, err, w = marginals(guess, fixed, ef, et, meas, info, kind, delta, query)
    return blocks, err, w, guess


def condense(poses, ef, et, meas, info, kind, delta, gauge, query, initial_guess):
    """cgmr_condense_robust: ref_numpy.condense_ref on the information scaled by rho1 at the spanning-tree guess (which does
    not depend on the information).  Returns condense_ref's dict plus ``weights`` [nE]."""
    guess, _ = _guess(poses, gauge, ef, et, meas, initial_guess)
    w = RR.weights(guess, ef, et, meas, info, kind, delta)
    ref = R.condense_ref(poses, ef, et, meas, np.asarray(info, dtype=np.float64) * w[:, None], gauge, query, initial_guess)
    ref["weights"] = w
    return ref
