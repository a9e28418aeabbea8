"""Bearing-only observations and landmark data association without a GPU: the float64 reference itself (tests/ref_assoc.py),
the cases' predicates, the .g2o reader / writer, the header, and the measurement the GPU's backward-error bar rests on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import assoc_cases as AC
import ref_assoc as A
import ref_numpy as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cgmr_marginals_joint_typed", "cgmr_marginals_pairs_typed", "cgmr_observation_covariance")


def _a(g):
    return AC.args(g)


@pytest.mark.parametrize("name", ["mixed5_257", "bearing_wrap", "bearing_answer", "bearing_axis"])
def test_reference_jacobians_against_central_differences(name):
    """J_i, J_j of every factor against central differences of its error, to 1e-7 (a bearing's difference taken across +-pi)."""
    g = AC.case(name)
    p, ef, et, meas, ek = g["poses"], g["edge_from"], g["edge_to"], g["meas"], g["ek"]
    Ji, Jj = A.jacobians(p, ef, et, meas, ek)
    h = 1e-6
    worst = 0.0
    for k in range(len(ef)):
        for J, v, unary in ((Ji[k], ef[k], False), (Jj[k], et[k], ef[k] == et[k])):
            if unary:
                continue
            for c in range(3 if g["vk"][v] == 0 else 2):
                pp, pm = p.copy(), p.copy()
                pp[v, c] += h
                pm[v, c] -= h
                d = A.edge_errors(pp, ef[k:k + 1], et[k:k + 1], meas[k:k + 1], ek[k:k + 1])[0] - \
                    A.edge_errors(pm, ef[k:k + 1], et[k:k + 1], meas[k:k + 1], ek[k:k + 1])[0]
                d[2] = R.normalize_theta(d[2])
                if ek[k] == 2:
                    d[0] = R.normalize_theta(d[0])
                worst = max(worst, float(np.abs(d / (2 * h) - J[:, c]).max()))
            if ek[k] == 2:
                assert np.all(J[1:] == 0) and np.all(J[:, 2] == (-1.0 if v == ef[k] else 0.0) * np.array([1, 0, 0]))
    assert worst <= 1e-7, worst


def test_known_answer_bearing():
    g = AC.case("bearing_answer")
    p, ef, et, meas, ek = g["poses"], g["edge_from"], g["edge_to"], g["meas"], g["ek"]
    e = A.edge_errors(p, ef, et, meas, ek)
    Ji, Jj = A.jacobians(p, ef, et, meas, ek)
    assert abs(e[0, 0] + 0.1) <= 1e-15 and e[0, 1] == 0 and e[0, 2] == 0
    assert np.abs(Ji[0, 0] - [0.5, -0.5, -1.0]).max() <= 1e-15 and np.abs(Jj[0, 0] - [-0.5, 0.5, 0.0]).max() <= 1e-15
    assert A.edge_chi2(p, ef, et, meas, g["info"], ek)[0] == pytest.approx(0.04, rel=1e-13)
    O = A.info_typed(g["info"], ek)[0]
    assert O[0, 0] == 4.0 and np.count_nonzero(O) == 1          # (the junk around info[0] is ignored)


def test_known_answer_bearing_wrap():
    g = AC.case("bearing_wrap")
    e = A.edge_errors(g["poses"], g["edge_from"], g["edge_to"], g["meas"], g["ek"])
    z, _ = A.predict(g["poses"], 0, 1, 2)
    assert abs(z[0] - g["meas"][0, 0]) > 6.0 and abs(e[0, 0] - 0.02) <= 1e-12
    assert A.edge_chi2(*_a(g)[:1], *_a(g)[2:], g["ek"])[0] == pytest.approx(50.0 * 0.02 ** 2, rel=1e-9)


def test_bearing_on_the_pose_has_no_nans():
    p = np.array([[1.0, 2.0, 0.7], [1.0, 2.0, 0.0]])
    ef, et, meas, ek = np.array([0]), np.array([1]), np.array([[0.3, 0, 0]]), np.array([2], np.uint8)
    e = A.edge_errors(p, ef, et, meas, ek)
    Ji, Jj = A.jacobians(p, ef, et, meas, ek)
    assert e[0].tolist() == [-0.3, 0.0, 0.0] and np.all(Ji == 0) and np.all(Jj == 0)


@pytest.mark.parametrize("name", ["bearing_axis", "mixed5_257"])
def test_true_dimension_system_equals_padded_system(name):
    """The padded 3-per-vertex system -- a point's dummy decoupled by the sum of its edges' H_jj(0,0), a bearing's with no
    fall-back -- gives the true-dimension system's iterates to 1e-13 (tests/test_typed_cpu.py's bar) and the same max |H_jj|:
    exactly on bearing_axis, where the point is the only free vertex and one bearing's H_jj(0,0) is exactly 0."""
    g = AC.case(name)
    vk, ek = AC.kinds(g)
    x = xp = g["poses"].copy()
    fx = A.active_fixed(len(x), g["fixed"], g["edge_from"], g["edge_to"])
    for it in range(4):
        H, b, lay = A.build_system(x, fx, *_a(g)[2:], vk, ek)
        x = A.apply_step(x, lay, A.splu_solve(H, b))
        Hp, bp, layp = A.padded_system(xp, fx, *_a(g)[2:], vk, ek)
        if name == "bearing_axis":
            assert Hp.diagonal().max() == H.diagonal().max() and H.diagonal().max() < 1.0
            o = layp.off[g["point"]]
            assert Hp[o + 2, o + 2] == Hp[o, o] > 0
        else:
            assert Hp.diagonal().max() == pytest.approx(H.diagonal().max(), rel=8 * A.U)
        dxp = A.splu_solve(Hp, bp)
        assert all(dxp[layp.off[v] + 2] == 0 for v in np.flatnonzero((vk == 1) & (layp.off >= 0)))
        xp = A.apply_step(xp, layp, dxp)
        assert np.abs(x - xp).max() <= 1e-13


def test_bearing_axis_levenberg_first_lambda():
    """Levenberg's first lambda is tau * max |H_jj| of the true system; kind 1's fall-back (1.0 for an H_jj(0,0) that is not
    positive) on the axis bearing would have made it tau * 1.0."""
    g = AC.case("bearing_axis")
    vk, ek = AC.kinds(g)
    H, _, _ = A.build_system(*_a(g), vk, ek)
    ref = A.lm_optimize(*_a(g), 3, vk, ek)
    lam0 = ref["trace"][0]["lambda"]
    assert lam0 == 1e-5 * H.diagonal().max() and lam0 < 1e-5
    Jj = A.jacobians(g["poses"], g["edge_from"], g["edge_to"], g["meas"], ek)[1]
    assert Jj[g["axis_edge"], 0, 0] == 0.0                      # ... which is where the 1.0 would have come from


def test_g2o_hand_written_file_with_a_bearing(tmp_path):
    from cg_mrslam_amd.graph import PoseGraph
    txt = ("VERTEX_SE2 0 0 0 0\nVERTEX_SE2 1 1 0 0.1\nVERTEX_XY 7 2 3\nFIX 0\n"
           "EDGE_SE2 0 1 1 0 0.1 100 0 0 100 0 1000\nEDGE_BEARING_SE2_XY 1 7 0.75 250\nEDGE_SE2_XY 0 7 2 3 10 1 20\n")
    f = tmp_path / "a.g2o"
    f.write_text(txt)
    g = PoseGraph.load_g2o(str(f))
    assert g.n_vertices == 3 and g.n_edges == 3 and g.typed
    assert g.edge_kind.tolist() == [0, 2, 1] and g.edge_from.tolist() == [0, 1, 0] and g.edge_to.tolist() == [1, 2, 2]
    assert g.meas[1].tolist() == [0.75, 0, 0] and g.info[1].tolist() == [250, 0, 0, 0, 0, 0]
    g.save_g2o(str(tmp_path / "b.g2o"))
    assert "EDGE_BEARING_SE2_XY 1 7 0.75 250\n" in (tmp_path / "b.g2o").read_text()


def test_g2o_round_trip(tmp_path):
    from cg_mrslam_amd.graph import PoseGraph
    c = AC.case("mixed5_255")
    ids = 100 + 3 * np.arange(len(c["poses"]))
    g = PoseGraph(ids, c["poses"], c["fixed"], c["edge_from"], c["edge_to"], c["meas"], c["info"], vertex_kind=c["vk"],
                  edge_kind=c["ek"])
    g.save_g2o(str(tmp_path / "a.g2o"), precision=17)
    h = PoseGraph.load_g2o(str(tmp_path / "a.g2o"))
    h.save_g2o(str(tmp_path / "b.g2o"), precision=17)
    assert (tmp_path / "a.g2o").read_bytes() == (tmp_path / "b.g2o").read_bytes()
    assert np.array_equal(h.vertex_kind, c["vk"]) and np.array_equal(h.edge_kind, c["ek"])
    assert np.array_equal(h.poses, c["poses"]) and np.array_equal(h.edge_from, c["edge_from"]) and np.array_equal(h.edge_to, c["edge_to"])
    one = c["ek"] == 2
    assert one.sum() >= 20 and np.array_equal(h.meas[one, 0], c["meas"][one, 0]) and np.array_equal(h.info[one, 0], c["info"][one, 0])
    assert np.all(h.meas[one, 1:] == 0) and np.all(h.info[one, 1:] == 0)     # what a 1-dimensional factor ignores is not written
    assert A.chi2(h.poses, h.edge_from, h.edge_to, h.meas, h.info, h.edge_kind) == A.chi2(*_a(c)[:1], *_a(c)[2:], c["ek"])


def test_graph_slam_add_bearing():
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
    g = PoseGraph([0, 1], [[0, 0, 0], [1, 0, 0]], [1, 0], [0], [1], [[1, 0, 0]], [[1, 0, 0, 1, 0, 1]])
    s = GraphSLAM.__new__(GraphSLAM)                              # (the appenders need no device)
    s.graph = g
    l = s.addLandmark(50, (2.0, 1.0))
    e1 = s.addBearing(1, l, 0.75, 250.0)
    e2 = s.addObservation(0, l, (2.0, 1.0), (10.0, 0.5, 20.0))
    assert (l, e1, e2) == (2, 1, 2)
    assert g.edge_kind.tolist() == [0, 2, 1] and g.edge_from.tolist() == [0, 1, 0] and g.edge_to.tolist() == [1, 2, 2]
    assert g.meas[1].tolist() == [0.75, 0, 0] and g.info[1].tolist() == [250, 0, 0, 0, 0, 0]
    assert g.add_edge(1, l, [0.5], [9.0], kind=2) == 3 and g.info[3, 0] == 9.0
    vk, ek = s._typed_level0()
    assert vk.tolist() == [0, 0, 1] and ek.tolist() == [0, 2, 1, 2]


def _prototype(name):
    txt = open(os.path.join(ROOT, "include", "cgmr.h")).read()
    m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", txt)
    assert m, f"{name} is not declared in include/cgmr.h"
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name,plain,extra", [("cgmr_marginals_joint_typed", "cgmr_marginals_joint", []),
                                              ("cgmr_marginals_pairs_typed", "cgmr_marginals_pairs", []),
                                              ("cgmr_observation_covariance", "cgmr_relative_covariance", ["const uint8_t* obs_kind"])])
def test_header_and_lib_declare_the_new_entry_points(name, plain, extra):
    from cg_mrslam_amd import _lib
    lib = _lib.load_library()
    assert name in _lib.declared_symbols() and name in _lib._SYMBOLS and hasattr(lib, name)
    assert lib.cgmr_version() == 105
    args, base = _prototype(name), _prototype(plain)
    assert args[-2:] == ["const cgmr_factor_types* types", "const cgmr_robust* rk"] and base[-1] == "const cgmr_robust* rk"
    assert len(args) == len(base) + 1 + len(extra)
    assert [a.split()[0:2] for a in args[:12]] == [a.split()[0:2] for a in base[:12]]     # the graph and the pairs / queries first
    for e in extra:
        assert e in args
    hdr = open(os.path.join(ROOT, "include", "cgmr.h")).read()
    assert "#define CGMR_EDGE_BEARING_SE2_XY 2" in hdr and "reserved (bearing-only" not in hdr
    assert _lib.EDGE_BEARING_SE2_XY == 2


def test_null_context_is_refused():
    from cg_mrslam_amd import _lib
    lib = _lib.load_library()
    n = C.c_void_p(0)
    i = C.c_int(0)
    assert lib.cgmr_marginals_joint_typed(n, i, n, n, i, n, n, n, n, i, n, n, n, n) == -1
    assert lib.cgmr_marginals_pairs_typed(n, i, n, n, i, n, n, n, n, i, n, n, n, n, n, n, n) == -1
    assert lib.cgmr_observation_covariance(n, i, n, n, i, n, n, n, n, i, n, n, n, n, n, n, n, n, n, n) == -1


@pytest.mark.parametrize("name", list(AC.CASES))
def test_cases_reach_their_gap(name):
    """The predicate, the 0.5 m between pose and point on every bearing edge, and a start from which ten Gauss-Newton
    iterations of the reference decrease chi2 monotonically (to rounding once it has converged)."""
    _, why, reach = AC.CASES[name]
    g = AC.case(name)
    assert reach(g), (name, why)
    assert AC.bearing_ranges(g).min() >= AC.R_MIN and AC.bearing_ranges(g, g["truth"]).min() >= AC.R_MIN
    assert np.all(g["poses"][g["vk"] == 1, 2] == 0.0)
    obs = (g["ek"] == 1) | (g["ek"] == 2)
    assert np.all(g["vk"][g["edge_to"][obs]] == 1) and np.all(g["vk"][g["edge_from"]] == 0)
    if name in AC.GN_CASES:
        _, chi, starts = A.gn_optimize(*_a(g), 10, *AC.kinds(g))
        assert np.all(np.diff(chi) <= 1e-9 * chi[:-1] + 1e-18), chi
        assert min(AC.bearing_ranges(g, p).min() for p in starts) >= AC.R_MIN


def _dense_solve(H, b):
    return np.linalg.solve(H.toarray(), b)


def test_reference_backward_error():
    """The componentwise backward error of the reference's own steps -- SuperLU and a dense LAPACK solve -- on every case
    Gauss-Newton can step, from the initial guess and from the reference's 3rd iterate: the measurement assoc_cases.OMEGA_MAX
    rests on (ten times the largest must not exceed it; REF_OMEGA_MEASURED records it)."""
    worst = 0.0
    for name in AC.GN_CASES:
        g = AC.case(name)
        vk, ek = AC.kinds(g)
        p3, _, _ = A.gn_optimize(*_a(g), 3, vk, ek)
        for start in (g["poses"], p3):
            for solve in (A.splu_solve, _dense_solve):
                p1, _, _ = A.gn_optimize(start, *_a(g)[1:], 1, vk, ek, solve=solve)
                w = A.step_backward_error(start, p1, *_a(g)[1:], vk, ek)
                print(f"{name}: omega {w / A.U:.2f} u ({solve.__name__})")
                worst = max(worst, w)
    print(f"largest omega of the reference solves: {worst / A.U:.2f} u")
    assert 10 * worst <= AC.OMEGA_MAX, worst / A.U
    assert abs(worst / A.U - AC.REF_OMEGA_MEASURED) <= max(0.05 * AC.REF_OMEGA_MEASURED, 0.5), worst / A.U     # (recorded to half a unit)


def test_backward_error_catches_a_wrong_bearing_term():
    """A 1e-9 relative error in the step of a point that only bearings and two observations hold shows far above the bar."""
    g = AC.case("mixed5_257")
    vk, ek = AC.kinds(g)
    p1, _, _ = A.gn_optimize(*_a(g), 1, vk, ek)
    l = int(g["edge_to"][np.flatnonzero(ek == 2)[0]])
    bad = p1.copy()
    bad[l, 1] += 1e-9 * max(1.0, abs(p1[l, 1] - g["poses"][l, 1])) + 1e-9
    assert A.step_backward_error(g["poses"], p1, *_a(g)[1:], vk, ek) <= AC.OMEGA_MAX
    assert A.step_backward_error(g["poses"], bad, *_a(g)[1:], vk, ek) > 100 * AC.OMEGA_MAX


def _dense_inverse(g, p):
    vk, ek = AC.kinds(g)
    fx = A.active_fixed(len(p), g["fixed"], g["edge_from"], g["edge_to"])
    H, _, lay = A.build_system(p, fx, *_a(g)[2:], vk, ek)
    return np.linalg.inv(H.toarray()), lay


def test_reference_marginals_match_dense_inverse():
    g = AC.case("mixed5_257")
    vk, ek = AC.kinds(g)
    p, _, _ = A.gn_optimize(*_a(g), 3, vk, ek)
    pairs = list(zip(g["edge_from"][:40], g["edge_to"][:40]))
    diag, cross, err = A.marginal_blocks(p, *_a(g)[1:], vk, ek, pairs=pairs)
    assert err <= AC.REF_ERR_MAX
    Hi, lay = _dense_inverse(g, p)
    for v in range(len(p)):
        o, d = lay.off[v], lay.dim[v]
        assert np.linalg.norm(diag[v, :d, :d] - Hi[o:o + d, o:o + d]) <= 1e-9 * np.linalg.norm(diag[v])
        assert np.all(diag[v, d:, :] == 0) and np.all(diag[v, :, d:] == 0)
    for k, (a, b) in enumerate(pairs):
        oa, da, ob, db = lay.off[a], lay.dim[a], lay.off[b], lay.dim[b]
        assert np.linalg.norm(cross[k, :da, :db] - Hi[oa:oa + da, ob:ob + db]) <= 1e-9 * np.sqrt(np.linalg.norm(diag[a]) * np.linalg.norm(diag[b]))


@pytest.mark.parametrize("kind", [1, 2])
def test_reference_gate_against_brute_force(kind):
    """z, S and d2 of ref_assoc.observations against the dense joint covariance cut out of inv(H) and a plain solve."""
    g = AC.case("mixed5_257")
    vk, ek = AC.kinds(g)
    p, _, _ = A.gn_optimize(*_a(g), 3, vk, ek)
    rng = np.random.default_rng(8)
    pairs = [(int(g["P"][rng.integers(48)]), int(g["L"][rng.integers(24)])) for _ in range(12)]
    pairs = [(a, b) for a, b in pairs if np.hypot(*(p[a, :2] - p[b, :2])) >= AC.R_MIN]
    n = len(pairs)
    assert n >= 8
    z0 = np.array([A.predict(p, a, b, kind)[0] for a, b in pairs])
    zh = z0 + rng.normal(0, 0.05, (n, 3)) * ([1, 1, 0] if kind == 1 else [1, 0, 0])
    hi = np.tile([400.0, 30.0, 7.0, 300.0, -3.0, 11.0], (n, 1))
    z, S, d2, _, _ = A.observations(p, *_a(g)[1:], vk, ek, pairs, [kind] * n, zh, hi)
    _, _, d2n, _, _ = A.observations(p, *_a(g)[1:], vk, ek, pairs, [kind] * n, zh)
    Hi, lay = _dense_inverse(g, p)
    d = 2 if kind == 1 else 1
    for k, (a, b) in enumerate(pairs):
        idx = np.r_[lay.off[a] + np.arange(3), lay.off[b] + np.arange(2)]
        xa, l = p[a], p[b]
        c, s = np.cos(xa[2]), np.sin(xa[2])
        r = np.array([[c, s], [-s, c]]) @ (l[:2] - xa[:2])
        J = np.array([[-c, -s, r[1], c, s], [s, -c, -r[0], -s, c]])
        zz = r
        if kind == 2:
            q = r @ r
            J = ((-r[1] / q) * J[0] + (r[0] / q) * J[1])[None, :]
            zz = np.array([np.arctan2(r[1], r[0])])
        Sb = J @ Hi[np.ix_(idx, idx)] @ J.T
        assert np.abs(z[k, :d] - zz).max() <= 1e-14 and np.all(z[k, d:] == 0)
        assert np.linalg.norm(S[k, :d, :d] - Sb) <= 1e-9 * np.linalg.norm(Sb) and np.all(S[k, d:, :] == 0) and np.all(S[k, :, d:] == 0)
        e = zz - zh[k, :d]
        if kind == 2:
            e = np.array([float(R.normalize_theta(e[0]))])
        W = np.linalg.inv(np.array([[hi[k, 0], hi[k, 1]], [hi[k, 1], hi[k, 3]]])[:d, :d])
        assert d2[k] == pytest.approx(float(e @ np.linalg.solve(Sb + W, e)), rel=1e-8)
        assert d2n[k] == pytest.approx(float(e @ np.linalg.solve(Sb, e)), rel=1e-8)
    assert np.isnan(A.gate(np.zeros(3), np.zeros((3, 3)), kind, np.zeros(3)))     # not positive definite: NaN
