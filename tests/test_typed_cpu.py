"""Typed factors (point landmarks, pose and position priors) without a GPU: the float64 reference itself (tests/ref_typed.py),
the cases' predicates, the .g2o reader / writer, the header, and the measurement the GPU's backward-error bar rests on."""
import os
import re

import numpy as np
import pytest

import ref_numpy as R
import ref_typed as T
import typed_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _a(g):
    return TC.args(g)


@pytest.mark.parametrize("name", ["mixed257", "leaf_and_hub", "wrap_prior"])
def test_reference_jacobians_against_central_differences(name):
    """J_i, J_j of every factor against central differences of its error, to 1e-7."""
    g = TC.case(name)
    p, ef, et, meas, ek = g["poses"], g["edge_from"], g["edge_to"], g["meas"], g["ek"]
    Ji, Jj = T.jacobians(p, ef, et, meas, ek)
    h = 1e-6
    worst = 0.0
    for k in range(len(ef)):
        for J, v, unary in ((Ji[k], ef[k], False), (Jj[k], et[k], ef[k] == et[k])):
            if unary:
                continue                                        # (a prior is carried by Ji alone)
            for c in range(3 if g["vk"][v] == 0 else 2):
                pp, pm = p.copy(), p.copy()
                pp[v, c] += h
                pm[v, c] -= h
                d = T.edge_errors(pp, ef[k:k + 1], et[k:k + 1], meas[k:k + 1], ek[k:k + 1])[0] - \
                    T.edge_errors(pm, ef[k:k + 1], et[k:k + 1], meas[k:k + 1], ek[k:k + 1])[0]
                d[2] = R.normalize_theta(d[2])
                worst = max(worst, float(np.abs(d / (2 * h) - J[:, c]).max()))
            if g["vk"][v] == 1:
                assert np.all(J[:, 2] == 0)
    assert worst <= 1e-7, worst


def test_known_answer_landmark():
    g = TC.landmark_answer()
    p, _, _ = T.gn_optimize(*_a(g), 1, g["vk"], g["ek"])
    assert np.abs(p[1, :2] - g["answer"]).max() <= 1e-12 and p[1, 2] == 0.0
    assert np.array_equal(p[0], g["poses"][0])


@pytest.mark.parametrize("wrap", [False, True])
def test_known_answer_prior(wrap):
    g = TC.prior_answer(wrap)
    p, chi, _ = T.gn_optimize(*_a(g), 1, g["vk"], g["ek"])
    assert np.abs(p[0, :2] - g["answer"][:2]).max() <= 1e-12
    assert abs(float(R.normalize_theta(p[0, 2] - g["answer"][2]))) <= 1e-12
    assert chi[1] <= 1e-20
    if wrap:                                                    # the heading error was taken across +-pi, not around the circle
        x, z = g["poses"][0], g["answer"]
        assert abs(float(R.normalize_theta(x[2] - z[2]))) < 1e-3 and abs(x[2] - z[2]) > 6.0
        c, s = np.cos(z[2]), np.sin(z[2])
        e = np.array([c * (x[0] - z[0]) + s * (x[1] - z[1]), -s * (x[0] - z[0]) + c * (x[1] - z[1]), x[2] - z[2] + 2 * np.pi])
        assert chi[0] == pytest.approx(float(e @ R.info_full(g["info"])[0] @ e), rel=1e-9)


def test_true_dimension_system_equals_padded_system():
    """The padded 3-per-vertex system -- a point's dummy unknown decoupled by a copy of its H_xx, right-hand side 0 -- gives
    the true-dimension system's iterates (the claim the device path rests on), and the same max |H_jj|."""
    g = TC.case("mixed257")
    vk, ek = TC.kinds(g)
    x = xp = g["poses"].copy()
    fx = T.active_fixed(len(x), g["fixed"], g["edge_from"], g["edge_to"])
    for _ in range(4):
        H, b, lay = T.build_system(x, fx, *_a(g)[2:], vk, ek)
        x = T.apply_step(x, lay, T.splu_solve(H, b))
        Hp, bp, layp = T.build_system(xp, fx, *_a(g)[2:], np.zeros_like(vk), ek)     # every vertex 3 wide: zero dummy rows
        Hp = Hp.tolil()
        for v in np.flatnonzero((vk == 1) & (layp.off >= 0)):
            o = layp.off[v]
            assert Hp[o + 2, o + 2] == 0 and bp[o + 2] == 0
            Hp[o + 2, o + 2] = Hp[o, o]
        assert Hp.diagonal().max() == pytest.approx(H.diagonal().max(), rel=8 * T.U)     # (two summation orders of one diagonal)
        dxp = T.splu_solve(Hp.tocsc(), bp)
        assert all(dxp[layp.off[v] + 2] == 0 for v in np.flatnonzero(vk == 1))
        xp = T.apply_step(xp, layp, dxp)
        assert np.abs(x - xp).max() <= 1e-13


def test_g2o_hand_written_file_with_all_line_types(tmp_path):
    from cg_mrslam_amd.graph import PoseGraph
    txt = ("VERTEX_SE2 0 0 0 0\nVERTEX_SE2 1 1 0 0.1\nVERTEX_XY 7 2 3\nFIX 0\n"
           "EDGE_SE2 0 1 1 0 0.1 100 0 0 100 0 1000\nEDGE_SE2_XY 1 7 1 3 10 1 20\n"
           "EDGE_PRIOR_SE2 0 0.5 0.25 0.125 5 0 0 5 0 50\nEDGE_PRIOR_SE2_XY 1 1.5 0.5 4 0.5 4\nUNKNOWN_TAG 3 4\n")
    f = tmp_path / "a.g2o"
    f.write_text(txt)
    g = PoseGraph.load_g2o(str(f))
    assert g.n_vertices == 3 and g.n_edges == 4 and g.typed
    assert g.vertex_kind.tolist() == [0, 0, 1] and g.edge_kind.tolist() == [0, 1, 3, 4]
    assert g.edge_from.tolist() == [0, 1, 0, 1] and g.edge_to.tolist() == [1, 2, 0, 1]
    assert g.poses[2].tolist() == [2.0, 3.0, 0.0]
    assert g.meas.tolist() == [[1, 0, 0.1], [1, 3, 0], [0.5, 0.25, 0.125], [1.5, 0.5, 0]]
    assert g.info[1].tolist() == [10, 1, 0, 20, 0, 0] and g.info[2].tolist() == [5, 0, 0, 5, 0, 50]
    assert g.info[3].tolist() == [4, 0.5, 0, 4, 0, 0]


def test_g2o_round_trip(tmp_path):
    from cg_mrslam_amd.graph import PoseGraph
    c = TC.case("mixed255")
    ids = 100 + 3 * np.arange(len(c["poses"]))
    g = PoseGraph(ids, c["poses"], c["fixed"], c["edge_from"], c["edge_to"], c["meas"], c["info"], vertex_kind=c["vk"],
                  edge_kind=c["ek"])
    g.save_g2o(str(tmp_path / "a.g2o"), precision=17)
    h = PoseGraph.load_g2o(str(tmp_path / "a.g2o"))
    h.save_g2o(str(tmp_path / "b.g2o"), precision=17)
    assert (tmp_path / "a.g2o").read_text() == (tmp_path / "b.g2o").read_text()
    assert np.array_equal(h.vertex_kind, c["vk"]) and np.array_equal(h.edge_kind, c["ek"])
    assert np.array_equal(h.poses, c["poses"]) and np.array_equal(h.edge_from, c["edge_from"]) and np.array_equal(h.edge_to, c["edge_to"])
    two = (c["ek"] == 1) | (c["ek"] == 4)
    assert np.array_equal(h.meas[~two], c["meas"][~two]) and np.array_equal(h.meas[two, :2], c["meas"][two, :2])
    assert np.array_equal(h.info[~two], c["info"][~two]) and np.array_equal(h.info[two][:, [0, 1, 3]], c["info"][two][:, [0, 1, 3]])
    assert np.all(h.meas[two, 2] == 0) and np.all(h.info[two][:, [2, 4, 5]] == 0)      # what a 2-dimensional factor ignores is not written
    # a pure pose graph is written and read as ever: no kinds appear
    p = PoseGraph(ids[:2], c["poses"][:2], c["fixed"][:2], [0], [1], c["meas"][:1], c["info"][:1])
    p.save_g2o(str(tmp_path / "p.g2o"))
    q = PoseGraph.load_g2o(str(tmp_path / "p.g2o"))
    assert q.vertex_kind is None and q.edge_kind is None and not q.typed


def test_graph_slam_appenders():
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
    g = PoseGraph([0, 1], [[0, 0, 0], [1, 0, 0]], [1, 0], [0], [1], [[1, 0, 0]], [[1, 0, 0, 1, 0, 1]])
    s = GraphSLAM.__new__(GraphSLAM)                              # (the appenders need no device)
    s.graph = g
    assert s._typed_level0() is None
    l = s.addLandmark(50, (2.0, 1.0))
    e1 = s.addObservation(1, l, (1.0, 1.0), (10.0, 0.5, 20.0))
    e2 = s.addPrior(0, (0.0, 0.0, 0.0), (5, 0, 0, 5, 0, 5))
    e3 = s.addPositionPrior(1, (1.0, 0.1), (4.0, 0.0, 4.0))
    assert (l, e1, e2, e3) == (2, 1, 2, 3)
    assert g.vertex_kind.tolist() == [0, 0, 1] and g.edge_kind.tolist() == [0, 1, 3, 4]
    assert g.edge_from.tolist() == [0, 1, 0, 1] and g.edge_to.tolist() == [1, 2, 0, 1]
    assert g.poses[2].tolist() == [2.0, 1.0, 0.0] and g.info[1].tolist() == [10, 0.5, 0, 20, 0, 0]
    vk, ek = s._typed_level0()
    assert vk.tolist() == [0, 0, 1] and ek.tolist() == [0, 1, 3, 4]


def test_header_declares_the_typed_entry_points():
    txt = open(os.path.join(ROOT, "include", "cgmr.h")).read()
    for name in ("cgmr_gn_optimize_typed", "cgmr_gn_optimize_typed_dev", "cgmr_lm_optimize_typed", "cgmr_lm_optimize_typed_dev",
                 "cgmr_dl_optimize_typed", "cgmr_dl_optimize_typed_dev", "cgmr_marginals_typed", "cgmr_marginals_all_typed"):
        assert re.search(r"\bint " + name + r"\s*\(", txt), name
    assert re.search(r"typedef struct cgmr_factor_types\s*\{\s*const uint8_t\* vertex_kind;[^}]*const uint8_t\* edge_kind;", txt)
    from cg_mrslam_amd import _lib
    assert "cgmr_marginals_all_typed" in _lib.declared_symbols()
    assert re.search(r"int cgmr_version\(void\) \{ return 105; \}", open(os.path.join(ROOT, "cg_mrslam_amd", "csrc", "cgmr_api.cpp")).read())


@pytest.mark.parametrize("name", list(TC.CASES))
def test_cases_reach_their_gap(name):
    _, why, reach = TC.CASES[name]
    g = TC.case(name)
    assert reach(g), (name, why)
    assert np.all(g["poses"][g["vk"] == 1, 2] == 0.0)
    pri = g["ek"] >= 3
    assert np.array_equal(g["edge_from"][pri], g["edge_to"][pri])
    assert np.all(g["vk"][g["edge_to"][g["ek"] == 1]] == 1) and np.all(g["vk"][g["edge_from"]] == 0)


def _dense_solve(H, b):
    return np.linalg.solve(H.toarray(), b)


def test_reference_backward_error():
    """The componentwise backward error of the reference's own steps -- SuperLU and a dense LAPACK solve -- on every case, from
    the initial guess and from the reference's 3rd iterate: the measurement typed_cases.OMEGA_MAX rests on (ten times the
    largest must not exceed it; REF_OMEGA_MEASURED records it)."""
    worst = 0.0
    for name in TC.CASES:
        g = TC.case(name)
        vk, ek = TC.kinds(g)
        p3, _, _ = T.gn_optimize(*_a(g), 3, vk, ek)
        for start in (g["poses"], p3):
            for solve in (T.splu_solve, _dense_solve):
                p1, _, _ = T.gn_optimize(start, *_a(g)[1:], 1, vk, ek, solve=solve)
                w = T.step_backward_error(start, p1, *_a(g)[1:], vk, ek)
                print(f"{name}: omega {w / T.U:.2f} u ({solve.__name__})")
                worst = max(worst, w)
    print(f"largest omega of the reference solves: {worst / T.U:.2f} u")
    assert 10 * worst <= TC.OMEGA_MAX, worst / T.U              # the bar holds: ten times the reference's own error lies below it
    assert worst <= 1.05 * TC.REF_OMEGA_MEASURED * T.U, worst / T.U     # ... and the recorded measurement is this one


def test_backward_error_catches_a_wrong_term():
    """A 1e-9 relative error in one landmark block of the step shows far above the bar."""
    g = TC.case("mixed257")
    vk, ek = TC.kinds(g)
    p1, _, _ = T.gn_optimize(*_a(g), 1, vk, ek)
    l = int(np.flatnonzero(vk == 1)[3])
    bad = p1.copy()
    bad[l, 0] += 1e-9 * max(1.0, abs(p1[l, 0] - g["poses"][l, 0])) + 1e-9
    assert T.step_backward_error(g["poses"], p1, *_a(g)[1:], vk, ek) <= TC.OMEGA_MAX
    assert T.step_backward_error(g["poses"], bad, *_a(g)[1:], vk, ek) > 100 * TC.OMEGA_MAX


def test_reference_marginals_match_dense_inverse():
    g = TC.case("leaf_and_hub")
    vk, ek = TC.kinds(g)
    p, _, _ = T.gn_optimize(*_a(g), 3, vk, ek)
    pairs = list(zip(g["edge_from"][:20], g["edge_to"][:20]))
    diag, cross, err = T.marginal_blocks(p, *_a(g)[1:], vk, ek, pairs=pairs)
    assert err <= TC.REF_ERR_MAX
    fx = T.active_fixed(len(p), g["fixed"], g["edge_from"], g["edge_to"])
    H, _, lay = T.build_system(p, fx, *_a(g)[2:], vk, ek)
    Hi = np.linalg.inv(H.toarray())
    for v in range(len(p)):
        if lay.off[v] < 0:
            assert np.all(diag[v] == 0)
            continue
        o, d = lay.off[v], lay.dim[v]
        assert np.linalg.norm(diag[v, :d, :d] - Hi[o:o + d, o:o + d]) <= 1e-9 * np.linalg.norm(diag[v])
        assert np.all(diag[v, d:, :] == 0) and np.all(diag[v, :, d:] == 0)
    assert np.all(diag[g["lone"]] == 0) and np.all(diag[g["fixed_point"]] == 0)
