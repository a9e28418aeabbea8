"""The reference of vertex removal (tests/ref_remove_nodes.py) proved on the CPU, and the preconditions of the cases
(tests/remove_nodes_cases.py) the device is then held to (tests/test_remove_nodes_gpu.py):

  two neighbours give exactly the composed edge z_1 (+) z_2 with the first-order composed covariance;
  weights and edges do not depend on which neighbour is fixed, nor on where v is put;
  every new edge's covariance is the exact relative covariance of its two ends under the dense local marginal;
  no tie decides a tree: every case's decision margin is at least MARGIN_MIN;
  on a chain the pruned graph's optimum is the full graph's at the kept vertices; on a ring it is not, by RING_GAP, and the
  kept vertices' marginal is RING_KL nats from what the pruned graph implies (both measured here, held to RING_MARGIN times).

Measured: degree two against z_1 (+) z_2 4.4e-16 and against the composed covariance 3.6e-10 (the finite differences' own error);
the chain 8.9e-16; the ring 4.098e-4 and 2.396e-4 nats (remove_nodes_cases.RING_GAP / RING_KL)."""
import numpy as np
import pytest

import ref_condense_tree as T
import ref_joint_marginals as J
import ref_numpy as R
import ref_remove_nodes as RN
import remove_nodes_cases as K
from condense_tree_cases import info_full as _full


def _compose_cov(z1, O1, z2, O2, h=1e-6):
    """The first-order covariance of z_1 (+) z_2 for independent z_1, z_2 with informations O1, O2, in the error frame of the
    composed edge: central differences of e(d1, d2) = z^-1 ((z_1 + d1) (+) (z_2 + d2)) -- the error's own frame -- where each
    measurement is moved in ITS error frame, e_k = z_k^-1 (z_k'), as its information is stated."""
    z = R._se2_mul(z1, z2)

    def err(d1, d2):
        a = R._se2_mul(z1, d1)                                     # z_1 moved by d1 in its own frame
        b = R._se2_mul(z2, d2)
        return R._se2_mul(R._se2_inv(z), R._se2_mul(a, b))

    Jm = np.zeros((3, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        Jm[:, k] = (err(d[:3], d[3:]) - err(-d[:3], -d[3:])) / (2 * h)
    S = np.zeros((6, 6))
    S[:3, :3], S[3:, 3:] = np.linalg.inv(O1), np.linalg.inv(O2)
    return z, Jm @ S @ Jm.T


@pytest.mark.parametrize("name", ["deg2_ff", "deg2_fb", "deg2_bf", "deg2_bb"])
def test_degree_two_is_the_composed_edge(name):
    nV, ef, et, meas, info, remove = K.case(name)
    v = int(remove[0])
    r = K.reference(name)
    assert r["flags"].tolist() == [0] and len(r["to"]) == 1
    lo, hi = int(r["fr"][0]), int(r["to"][0])
    assert lo < hi
    # z_(lo -> v) and z_(v -> hi) with their informations as stored, the stored direction turned where needed
    def toward(n, out):                                            # the edge between v and n as v -> n (out) or n -> v
        e = int(np.flatnonzero(((ef == v) & (et == n)) | ((ef == n) & (et == v)))[0])
        z, O = meas[e], _full(info[e])
        if (ef[e] == v) == out:
            return z, O
        # the inverse edge: e' = -Ad e to first order, so the information turns with the adjoint of z^-1 at the error's frame;
        # taken numerically here, from the definition, not from the code under test
        zi = R._se2_inv(z)
        h = 1e-6
        Jn = np.zeros((3, 3))
        for k in range(3):
            d = np.zeros(3)
            d[k] = h
            f = lambda dd: R._se2_mul(R._se2_inv(zi), R._se2_inv(R._se2_mul(z, dd)))   # noqa: E731
            Jn[:, k] = (f(d) - f(-d)) / (2 * h)
        S = Jn @ np.linalg.inv(O) @ Jn.T
        return zi, np.linalg.inv(S)
    z1, O1 = toward(lo, False)
    z2, O2 = toward(hi, True)
    z, S = _compose_cov(z1, O1, z2, O2)
    d = r["est"][0] - z
    d[2] = R.normalize_theta(d[2])
    print(f"{name}: est against z1 (+) z2 {np.abs(d).max():.1e}")
    assert np.abs(d).max() <= 1e-14
    C = np.linalg.inv(_full(r["iu"][0]))
    gap = np.linalg.norm(C - S) / np.linalg.norm(S)
    print(f"{name}: covariance against the first-order composition {gap:.1e}")
    assert gap <= 1e-8                                             # central differences at h = 1e-6: h^2 and eps / h, both ~1e-10


@pytest.mark.parametrize("name", ["deg3", "deg5", "deg16", "parallel"])
def test_invariant_under_the_gauge_and_the_placement_of_v(name):
    nV, ef, et, meas, info, remove = K.case(name)
    v = int(remove[0])
    base = RN.remove_one(ef, et, meas, info, v)
    m = len(base["nbrs"])
    for fix, xv in ((m - 1, (0, 0, 0)), (m // 2, (0, 0, 0)), (0, (3.0, -1.5, 2.5)), (1, (-0.7, 4.0, -3.0))):
        o = RN.remove_one(ef, et, meas, info, v, fix=fix, xv=xv)
        assert np.array_equal(o["parent"], base["parent"])
        assert np.abs(o["W"][np.isfinite(base["W"])] - base["W"][np.isfinite(base["W"])]).max() <= 1e-9
        d = o["est"] - base["est"]
        d[:, 2] = R.normalize_theta(d[:, 2])
        assert np.abs(d).max() <= 1e-12
        assert max(np.linalg.norm(a - b) / np.linalg.norm(b) for a, b in zip(o["iu"], base["iu"])) <= 1e-9


@pytest.mark.parametrize("name", ["deg3", "deg5", "deg15", "parallel", "unsorted"])
def test_edge_covariance_is_the_pairwise_relative_covariance_of_the_dense_marginal(name):
    """Independently of local_star's own inverse: the star's full H with only the gauge deleted, v's rows and columns dropped
    from a pseudo-solve through the Schur complement -- (H_nn - H_nv H_vv^-1 H_vn)^-1 -- then J Sigma J^T for the tree's pairs."""
    nV, ef, et, meas, info, remove = K.case(name)
    r = RN.remove_one(ef, et, meas, info, int(remove[0]))
    H = r["H"]                                                     # v first, then n_2 .. n_m
    Hvv, Hvn, Hnn = H[:3, :3], H[:3, 3:], H[3:, 3:]
    Sm = np.linalg.inv(Hnn - Hvn.T @ np.linalg.solve(Hvv, Hvn))    # the marginal of n_2 .. n_m
    m = len(r["nbrs"])
    full = np.zeros((3 * m, 3 * m))
    full[3:, 3:] = Sm
    for k in range(1, m):
        p = int(r["parent"][k])
        b = lambda a, c: full[3 * a:3 * a + 3, 3 * c:3 * c + 3]   # noqa: E731
        Sz = J.relative_cov(r["x"][p], r["x"][k], b(p, p), b(p, k), b(k, k))
        z = J.relative_pose(r["x"][p], r["x"][k])
        _, Je = J.hypothesis_error(z, z)
        C = np.linalg.inv(_full(r["iu"][k - 1]))
        want = Je @ Sz @ Je.T
        assert np.linalg.norm(C - want) / np.linalg.norm(want) <= 1e-9


@pytest.mark.parametrize("name", list(K.CASES))
def test_no_tie_decides_a_case(name):
    r = K.reference(name)
    print(f"{name}: decision margin {r['margin']:.3e} nats, {len(r['to'])} edges")
    assert r["margin"] >= K.MARGIN_MIN
    want = K.FLAGS.get(name, 0)
    assert np.all(r["flags"] == want)
    if name == "lattice300":
        deg = np.array([len(p["nbrs"]) for p in r["per"]])
        assert len(deg) == 300 and deg.min() <= 2 and deg.max() == 8 and len(np.unique(deg)) >= 5


def test_refusals_of_the_reference():
    with pytest.raises(ValueError, match="not independent"):
        RN.remove_nodes(*K.not_independent())
    nV, ef, et, meas, info, remove = K.case("deg3")
    with pytest.raises(ValueError, match="repeated"):
        RN.remove_nodes(nV, ef, et, meas, info, np.r_[remove, remove])


def _pruned(case_fn):
    (poses, fixed, ef, et, meas, info), remove = case_fn()
    pe, pt, pm, pi, skipped = RN.remove_vertices(len(poses), ef, et, meas, info, remove)
    assert not skipped
    full = K.optimum(poses, fixed, ef, et, meas, info)
    pruned = K.optimum(poses, fixed, pe, pt, pm, pi)
    keep = np.setdiff1d(np.arange(len(poses)), remove)
    d = pruned[keep] - full[keep]
    d[:, 2] = R.normalize_theta(d[:, 2])
    return dict(poses=poses, fixed=fixed, full=full, pruned=pruned, keep=keep, gap=np.abs(d).max(), graph=(ef, et, meas, info),
                pruned_graph=(pe, pt, pm, pi), remove=remove)


def test_chain_pruned_optimum_is_the_full_optimum():
    r = _pruned(K.chain_case)
    print(f"chain of 12: pruned against full optimum at the kept vertices {r['gap']:.2e}")
    assert len(r["pruned_graph"][0]) == 11 - 5
    assert r["gap"] <= 1e-10                                       # both are the composed odometry: rounding only


def ring_figures():
    """(gap, KL) of the ring case: the gap of the optima at the kept vertices, and KL( the kept free vertices' marginal under
    the full graph at its optimum || the Gaussian of the pruned graph at its optimum )."""
    r = _pruned(K.ring_case)
    free = r["keep"][r["fixed"][r["keep"]] == 0]
    Sigma = J.joint_dense(r["full"], r["fixed"], *r["graph"], free)
    pe, pt, pm, pi = r["pruned_graph"]
    fx = R.active_fixed(len(r["poses"]), r["fixed"], pe, pt)
    H, _, hidx = R.build_system(r["pruned"], fx, pe, pt, pm, pi)
    assert np.array_equal(np.flatnonzero(hidx >= 0), free)
    return r["gap"], T.kl(Sigma, H.toarray())


def test_ring_pruned_optimum_and_marginal_are_close_as_measured():
    gap, kl = ring_figures()
    print(f"ring of 12: pruned against full optimum at the kept vertices {gap:.3e}, KL of the kept marginal {kl:.3e} nats")
    assert gap <= K.RING_MARGIN * K.RING_GAP
    assert 0 <= kl <= K.RING_MARGIN * K.RING_KL


def test_entry_point_is_declared_and_exported():
    from cg_mrslam_amd import _lib
    lib = _lib.load_library()
    assert "cgmr_remove_nodes" in _lib.declared_symbols() and "cgmr_remove_nodes" in _lib._SYMBOLS and hasattr(lib, "cgmr_remove_nodes")
    assert lib.cgmr_version() == 105
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "cgmr.h")).read()
    assert f"#define CGMR_REMOVE_MAX_DEGREE {_lib.REMOVE_MAX_DEGREE}\n" in hdr and RN.MAX_DEGREE == _lib.REMOVE_MAX_DEGREE


def test_python_faces_exist():
    from cg_mrslam_amd import Context
    from cg_mrslam_amd.graph import GraphSLAM
    assert callable(getattr(Context, "remove_nodes", None)) and callable(getattr(GraphSLAM, "removeVertices", None))


class _ReferenceContext:
    """The reference in the device's place behind GraphSLAM: removeVertices' own bookkeeping, checked without a GPU."""
    def remove_nodes(self, ef, et, meas, info, remove, num_vertices=None):
        r = RN.remove_nodes(num_vertices, ef, et, meas, info, np.asarray(remove, dtype=np.int32))
        return r["off"], r["fr"], r["to"], r["est"], r["iu"], r["weight"], r["flags"]


def test_remove_vertices_bookkeeping_in_two_rounds():
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
    (poses, fixed, ef, et, meas, info), _ = K.ring_case()
    n, request = len(poses), [9, 2, 1, 3, 5, 7]
    g = PoseGraph(100 + np.arange(n), poses, fixed, ef, et, meas, info)
    g.lasers = {3: "three", 4: "four", 11: "eleven"}
    slam = GraphSLAM(g, _ReferenceContext())
    index_map, new_edges, skipped = slam.removeVertices(request)
    pe, pt, pm, pi, _ = RN.remove_vertices(n, ef, et, meas, info, request)
    want = RN.compact(n, request)
    assert skipped == [] and np.array_equal(index_map, want)
    assert np.array_equal(g.edge_from, want[pe]) and np.array_equal(g.edge_to, want[pt])
    assert np.array_equal(g.meas, pm) and np.array_equal(g.info, pi) and g.n_edges == 6 and new_edges.tolist() == [2, 3, 4, 5]
    assert g.lasers == {1: "four", 5: "eleven"} and np.array_equal(g.ids, 100 + np.flatnonzero(want >= 0))
    assert np.array_equal(g.poses, poses[want >= 0]) and len(g.edge_level) == 6 and not g.edge_level.any()
