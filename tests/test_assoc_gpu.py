"""Bearing-only observations (edge kind 2), typed joint / pairwise marginals and landmark data association on the GPU, against
the true-dimension float64 reference (tests/ref_assoc.py) on the cases of tests/assoc_cases.py.  The bars are those of the
tests this builds on: typed_cases' OMEGA_MAX rule and CHI_RTOL, the trace checks of tests/test_lm_gpu.py /
tests/test_dogleg_gpu.py, MARG_TAU / AGREE_TAU and the arithmetic bars of tests/test_joint_marginals_gpu.py."""
import numpy as np
import pytest

import assoc_cases as AC
import ref_assoc as A
import reference_cases as C
import typed_cases as TC
from cg_mrslam_amd._lib import CgmrError

pytestmark = pytest.mark.gpu


def _a(g):
    return AC.args(g)


def _kw(g):
    return dict(vertex_kind=g["vk"], edge_kind=g["ek"])


def _nd(x):
    return np.linalg.norm(x, axis=(-2, -1))


_OPT = {}


def _optimised(ctx, name, fix=()):
    """(the case with the vertices ``fix`` fixed as well, its poses after three Gauss-Newton iterations on the device)."""
    key = (name, tuple(fix))
    if key not in _OPT:
        g = dict(AC.case(name))
        g["fixed"] = g["fixed"].copy()
        g["fixed"][list(fix)] = 1
        rc, p, _ = ctx.gn_optimize_typed(*_a(g), 3, **_kw(g))
        assert rc == 0
        _OPT[key] = (g, p)
    return _OPT[key]


# --------------------------------------------------------------------------------------- 1. the solvers
def test_known_answers(ctx):
    g = AC.case("bearing_answer")
    one = (g["poses"], g["fixed"], g["edge_from"][:1], g["edge_to"][:1], g["meas"][:1], g["info"][:1])
    chi = ctx.gn_optimize_typed(*one, 0, vertex_kind=g["vk"], edge_kind=g["ek"][:1])[2]
    assert chi[0] == pytest.approx(0.04, rel=1e-12)
    w = AC.case("bearing_wrap")
    one = (w["poses"], w["fixed"], w["edge_from"][:1], w["edge_to"][:1], w["meas"][:1], w["info"][:1])
    chi = ctx.gn_optimize_typed(*one, 0, vertex_kind=w["vk"], edge_kind=w["ek"][:1])[2]
    assert chi[0] == pytest.approx(50.0 * 0.02 ** 2, rel=1e-9)      # e = 0.02, not 2 pi - 0.02
    # a point on the pose: e = normalize(-z0), zero Jacobians, no NaN
    p = np.array([[1.0, 2.0, 0.7], [1.0, 2.0, 0.0], [3.0, 2.0, 0.0]])
    rc, q, chi = ctx.gn_optimize_typed(p, [0, 0, 1], [0, 2, 0], [1, 1, 0], [[0.3, 0, 0], [-2.0, 0.0, 0], [1.0, 2.0, 0]],
                                       [[2.0, 0, 0, 0, 0, 0], [1.0, 0, 0, 1.0, 0, 0], [1.0, 0, 0, 1.0, 0, 1.0]], 1,
                                       vertex_kind=[0, 1, 0], edge_kind=[2, 1, 3])
    assert rc == 0 and np.all(np.isfinite(q)) and chi[0] == pytest.approx(2.0 * 0.3 ** 2 + 0.7 ** 2, rel=1e-12)


@pytest.mark.parametrize("name", AC.GN_CASES)
def test_gn_against_reference(ctx, name):
    """chi2 before each of 10 iterations against the reference's; one step from the initial guess and one from the GPU's own
    3rd iterate within the backward-error bar; a point's third component stays exactly 0.0; fixed vertices keep their bits."""
    _, why, reach = AC.CASES[name]
    g = AC.case(name)
    assert reach(g), why
    vk, ek = AC.kinds(g)
    a = _a(g)
    rc, p10, chi = ctx.gn_optimize_typed(*a, 10, **_kw(g))
    assert rc == 0
    _, chi_ref, _ = A.gn_optimize(*a, 10, vk, ek)
    rel = np.abs(chi - chi_ref) / np.maximum(np.abs(chi_ref), 1e-300)
    print(f"{name}: chi2 {chi[0]:.6g} -> {chi[-1]:.6g}, largest relative difference to the reference {rel[chi_ref > 1e-12].max():.2e}")
    np.testing.assert_allclose(chi, chi_ref, rtol=AC.CHI_RTOL, atol=1e-18)
    fx = A.active_fixed(len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"])
    worst = 0.0
    for start in (0, 3):
        p0 = g["poses"]
        if start:
            rc, p0, _ = ctx.gn_optimize_typed(*a, start, **_kw(g))
            assert rc == 0
        rc, p1, _ = ctx.gn_optimize_typed(p0, *a[1:], 1, **_kw(g))
        assert rc == 0
        for p in (p0, p1):
            assert np.all(p[vk == 1, 2] == 0.0)                  # (the dummy's dx is exactly 0; bearing_axis: with H_jj(0,0) = 0 on one edge)
            assert np.array_equal(p[fx != 0], g["poses"][fx != 0])
        w = A.step_backward_error(p0, p1, *a[1:], vk, ek)
        worst = max(worst, w)
        assert w <= AC.OMEGA_MAX, (name, start, w / A.U)
    print(f"{name}: largest omega {worst / A.U:.1f} u")
    assert np.all(p10[vk == 1, 2] == 0.0) and np.array_equal(p10[fx != 0], g["poses"][fx != 0])


def test_a_single_bearing_fails_gauss_newton_and_leaves_the_poses(ctx):
    g = AC.case("bearing_one")
    assert AC.CASES["bearing_one"][2](g)
    rc, p, _ = ctx.gn_optimize_typed(*_a(g), 3, **_kw(g), raise_on_cholesky=False)
    assert rc == -100 and np.array_equal(p, g["poses"])         # CGMR_E_CHOLESKY_BASE - 0


@pytest.mark.parametrize("name", list(AC.CASES))
def test_lm_trace_matches_reference(ctx, name):
    """Trials, termination, lambda and chi2 at the bars of tests/test_lm_gpu.py (check_trace): lambda at 1e-9 from the first
    iteration on holds tau * max |H_jj| to the true-dimension system's -- on bearing_axis below tau * 1.0."""
    import test_lm_gpu as LM
    g = AC.case(name)
    vk, ek = AC.kinds(g)
    ref = A.lm_optimize(*_a(g), LM.ITERS, vk, ek)
    rc, poses, chi, lam, tri, done = ctx.lm_optimize_typed(*_a(g), LM.ITERS, **_kw(g))
    assert rc == 0
    k = LM.check_trace(name, ref, chi, lam, tri, done, LM.rounding_floor(g))
    assert k >= 1, "nothing compared"
    assert np.all(poses[vk == 1, 2] == 0.0)
    fx = A.active_fixed(len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"])
    H, _, _ = A.build_system(g["poses"], fx, *_a(g)[2:], vk, ek)
    assert ref["trace"][0]["lambda"] == 1e-5 * H.diagonal().max()
    if name == "bearing_axis":
        # the first trial alone, lambda given: the same trial as with the device's own tau * max |H_jj|, which lies below tau * 1.0
        lam0 = ref["trace"][0]["lambda"]
        assert lam0 < 1e-5
        one = ctx.lm_optimize_typed(*_a(g), 1, **_kw(g))
        given = ctx.lm_optimize_typed(*_a(g), 1, **_kw(g), initial_lambda=lam0)
        assert one[5] == given[5] == 1 and np.array_equal(one[4], given[4])
        np.testing.assert_allclose(one[3], given[3], rtol=LM.RTOL)
        np.testing.assert_allclose(one[2], given[2], rtol=LM.RTOL)


@pytest.mark.parametrize("name", list(AC.CASES))
def test_dogleg_trace_matches_reference(ctx, name):
    """Trials, step kinds, termination, delta and chi2 at the bars of tests/test_dogleg_gpu.py (check_trace)."""
    import test_dogleg_gpu as DL
    g = AC.case(name)
    vk, ek = AC.kinds(g)
    ref = A.dl_optimize(*_a(g), DL.ITERS, vk, ek)
    rc, poses, chi, dlt, tri, stp, done = ctx.dl_optimize_typed(*_a(g), DL.ITERS, **_kw(g))
    assert rc == 0
    k = DL.check_trace(name, ref, chi, dlt, tri, stp, done, DL.rounding_floor(g))
    assert k >= 1, "nothing compared"
    assert np.all(poses[vk == 1, 2] == 0.0)


def test_robust_cauchy_with_bearings(ctx):
    g = AC.case("mixed5_257")
    vk, ek = AC.kinds(g)
    a = _a(g)
    rc, p, chi, e2, w = ctx.gn_optimize_typed(*a, 5, **_kw(g), kind="cauchy", delta=3.0)
    assert rc == 0
    w_ref = A.weights(p, *a[2:], ek, 3, 3.0)
    assert np.abs(w - w_ref).max() <= 1e-12 and (w[ek == 2] < 0.999).any()
    _, chi_ref, _ = A.gn_optimize(*a, 5, vk, ek, 3, 3.0)
    np.testing.assert_allclose(chi, chi_ref, rtol=AC.CHI_RTOL)


def test_outputs_without_bearings_are_unchanged(ctx):
    """All-zero kinds are the plain calls bit for bit (joint, pairs, observation covariance of kind 0); a graph of the kinds
    {0, 1, 3, 4} gives identical bytes on two calls."""
    g = C.CASES["pg500"][0]()
    a = C.args(g)
    rc, p, _ = ctx.gn_optimize(*a, 3)
    b = (p,) + tuple(a[1:])
    z = dict(vertex_kind=np.zeros(len(p), np.uint8), edge_kind=np.zeros(len(g["edge_from"]), np.uint8))
    q = np.array([3, 77, 0, 120, 77, 499, 250], np.int32)
    for kw in (z, dict(vertex_kind=z["vertex_kind"]), dict(edge_kind=z["edge_kind"])):
        assert ctx.marginals_joint(*b, q).tobytes() == ctx.marginals_joint(*b, q, **kw).tobytes()
        for u, v in zip(ctx.marginals_pairs(*b, q[:5], q[2:7]), ctx.marginals_pairs(*b, q[:5], q[2:7], **kw)):
            assert u.tobytes() == v.tobytes()
    rng = np.random.default_rng(3)
    zh = rng.normal(0, 1, (5, 3))
    hi = np.tile([900.0, 50.0, 0, 800.0, 0, 5000.0], (5, 1))
    rel = ctx.relative_covariance(*b, q[:5], q[2:7], zh, hi)
    for obs in (ctx.observation_covariance(*b, q[:5], q[2:7], None, zh, hi),
                ctx.observation_covariance(*b, q[:5], q[2:7], np.zeros(5, np.uint8), zh, hi, **z)):
        for u, v in zip(rel, obs):
            assert u.tobytes() == v.tobytes()
    relz = ctx.relative_covariance(*b, q[:5], q[2:7])
    obz = ctx.observation_covariance(*b, q[:5], q[2:7])
    assert relz[0].tobytes() == obz[0].tobytes() and relz[1].tobytes() == obz[1].tobytes() and obz[2] is None
    t = TC.case("mixed255")
    one, two = (ctx.gn_optimize_typed(*TC.args(t), 5, vertex_kind=t["vk"], edge_kind=t["ek"]) for _ in range(2))
    assert all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(one, two))


# --------------------------------------------------------------------------------------- 2. marginals
@pytest.mark.parametrize("name", ["mixed5_257", "bearing_two"])
def test_marginals_with_bearings_against_reference(ctx, name):
    g, p = _optimised(ctx, name)
    vk, ek = AC.kinds(g)
    a = _a(g)
    nV, ef, et = len(p), g["edge_from"], g["edge_to"]
    want, want_x, err = A.marginal_blocks(p, *a[1:], vk, ek, pairs=list(zip(ef, et)))
    assert err <= AC.REF_ERR_MAX
    cov_q = ctx.marginals_typed(p, *a[1:], np.arange(nV, dtype=np.int32), **_kw(g))
    cov_a, cross = ctx.marginals_all_typed(p, *a[1:], cross=True, **_kw(g))
    fx = A.active_fixed(nV, g["fixed"], ef, et)
    worst = 0.0
    for cov in (cov_q, cov_a):
        for v in range(nV):
            if fx[v]:
                assert np.all(cov[v] == 0), v
                continue
            if vk[v] == 1:
                assert np.all(cov[v][2, :] == 0) and np.all(cov[v][:, 2] == 0), v
            e = np.linalg.norm(cov[v] - want[v]) / np.linalg.norm(want[v])
            worst = max(worst, e)
            assert e <= AC.MARG_TAU, (v, e)
    for k in np.flatnonzero(ef != et):
        if fx[ef[k]] or fx[et[k]]:
            assert np.all(cross[k] == 0), k
            continue
        if ek[k] in (1, 2):
            assert np.all(cross[k][:, 2] == 0), k
        assert np.linalg.norm(cross[k] - want_x[k]) <= AC.MARG_TAU * np.sqrt(np.linalg.norm(want[ef[k]]) * np.linalg.norm(want[et[k]])), k
    print(f"{name}: largest relative block error {worst:.2e}")


def _queries(g, n):
    """n queries: poses and points alternating, then the fixed vertex and a duplicate."""
    P, L = g["P"], g["L"]
    q = [int(P[(5 * k) % len(P)]) if k % 2 == 0 else int(L[k % len(L)]) for k in range(n - 2)]
    fixed = int(np.flatnonzero(g["fixed"])[0])
    return np.array(q + [fixed, q[1]], np.int32)


@pytest.mark.parametrize("nK", [5, 17])
def test_marginals_joint_typed(ctx, nK):
    """5 queries: one 16-column tile and a bit; 17: 68 columns, past a 64-column macro-tile.  Every block against the
    reference, exact symmetry, exact zeros in the points' third rows and columns and in the fixed vertex's, identical bytes twice."""
    g, p = _optimised(ctx, "mixed5_257", fix=(int(AC.case("mixed5_257")["P"][7]),))
    vk, ek = AC.kinds(g)
    q = _queries(g, nK)
    assert vk[q].min() == 0 and vk[q].max() == 1 and g["fixed"][q].sum() == 1 and len(set(q.tolist())) == nK - 1
    S = ctx.marginals_joint(p, *_a(g)[1:], q, **_kw(g))
    assert S.tobytes() == ctx.marginals_joint(p, *_a(g)[1:], q, **_kw(g)).tobytes()
    assert np.array_equal(S, S.T)
    pairs = [(int(u), int(v)) for u in q for v in q]
    diag, cross, err = A.marginal_blocks(p, *_a(g)[1:], vk, ek, pairs=pairs)
    assert err <= AC.REF_ERR_MAX
    worst = 0.0
    for i, u in enumerate(q):
        if vk[u] == 1:
            assert np.all(S[3 * i + 2, :] == 0) and np.all(S[:, 3 * i + 2] == 0)
        if g["fixed"][u]:
            assert np.all(S[3 * i:3 * i + 3, :] == 0) and np.all(S[:, 3 * i:3 * i + 3] == 0)
        for j, v in enumerate(q):
            if g["fixed"][u] or g["fixed"][v]:
                continue
            e = np.linalg.norm(S[3 * i:3 * i + 3, 3 * j:3 * j + 3] - cross[i * nK + j]) / np.sqrt(np.linalg.norm(diag[u]) * np.linalg.norm(diag[v]))
            worst = max(worst, e)
    print(f"joint typed, {nK} queries: largest block error {worst:.2e}")
    assert worst <= AC.MARG_TAU


def test_marginals_pairs_typed(ctx):
    g, p = _optimised(ctx, "mixed5_257")
    vk, ek = AC.kinds(g)
    a = (p,) + _a(g)[1:]
    ef, et = g["edge_from"], g["edge_to"]
    obs = np.flatnonzero((ek == 1) | (ek == 2))
    aa, ab, bb = ctx.marginals_pairs(*a, ef[obs], et[obs], **_kw(g))
    cov, cross = ctx.marginals_all_typed(*a, cross=True, **_kw(g))
    scale = np.sqrt(_nd(cov[ef[obs]]) * _nd(cov[et[obs]]))
    assert np.max(_nd(ab - cross[obs]) / scale) <= AC.AGREE_TAU
    assert np.max(_nd(aa - cov[ef[obs]]) / _nd(cov[ef[obs]])) <= AC.AGREE_TAU and np.max(_nd(bb - cov[et[obs]]) / _nd(cov[et[obs]])) <= AC.AGREE_TAU
    assert np.all(aa[:, 2, 2] > 0) and np.all(ab[:, :, 2] == 0) and np.all(bb[:, 2, :] == 0) and np.all(bb[:, :, 2] == 0)
    # pairs no edge joins: (pose, point) and (point, point)
    adj = set(zip(ef.tolist(), et.tolist()))
    P, L = g["P"], g["L"]
    pairs = [(int(P[k]), int(L[(7 * k) % 24])) for k in range(0, 48, 5) if (int(P[k]), int(L[(7 * k) % 24])) not in adj]
    pairs += [(int(L[k]), int(L[(k + 5) % 24])) for k in range(0, 24, 4)]
    assert len(pairs) >= 12
    pa, pb = np.array(pairs, np.int32).T
    aa, ab, bb = ctx.marginals_pairs(*a, pa, pb, **_kw(g))
    for u, v in zip(ctx.marginals_pairs(*a, pa, pb, **_kw(g)), (aa, ab, bb)):
        assert u.tobytes() == v.tobytes()
    diag, want, err = A.marginal_blocks(*a, vk, ek, pairs=pairs)
    assert err <= AC.REF_ERR_MAX
    sc = np.sqrt(_nd(diag[pa]) * _nd(diag[pb]))
    assert np.max(_nd(ab - want) / sc) <= AC.MARG_TAU and np.max(_nd(aa - diag[pa]) / _nd(diag[pa])) <= AC.MARG_TAU
    assert np.max(_nd(bb - diag[pb]) / _nd(diag[pb])) <= AC.MARG_TAU
    pt = vk[pa] == 1
    assert pt.any() and np.all(aa[pt][:, 2, :] == 0) and np.all(aa[pt][:, :, 2] == 0) and np.all(ab[pt][:, 2, :] == 0) and np.all(ab[:, :, 2] == 0)


# --------------------------------------------------------------------------------------- 3. data association
def _assoc_pairs(g, p):
    P, L = g["P"], g["L"]
    pairs = [(int(P[(3 * k) % 48]), int(L[(5 * k) % 24])) for k in range(30)]
    return [(u, v) for u, v in pairs if np.hypot(*(p[u, :2] - p[v, :2])) >= AC.R_MIN]


@pytest.mark.parametrize("kind", [1, 2])
def test_observation_covariance(ctx, kind):
    """The device's prediction, propagation and gate (a) against numpy on the device's own pair blocks, at the bars of
    tests/test_joint_marginals_gpu.py::test_relative_covariance_arithmetic -- 1e-12 of the size of the terms,
    ||J||^2 (||Saa|| + 2 ||Sab|| + ||Sbb||), and for d2 that times ||M^-1 e||^2 plus cond(M) d2 --, and (b) end to end against
    the reference's refined solves: S to MARG_TAU of ||J||^2 sqrt(||Saa|| ||Sbb||)."""
    g, p = _optimised(ctx, "mixed5_257")
    vk, ek = AC.kinds(g)
    a = (p,) + _a(g)[1:]
    pairs = _assoc_pairs(g, p)
    n = len(pairs)
    assert n >= 20
    pa, pb = np.array(pairs, np.int32).T
    kinds = np.full(n, kind, np.uint8)
    rng = np.random.default_rng(10 + kind)
    z0 = np.array([A.predict(p, u, v, kind)[0] for u, v in pairs])
    zh = z0 + rng.normal(0, 0.05, (n, 3))                        # (the components past the factor's dimension: junk, ignored)
    hi = np.tile([400.0, 30.0, 7.0, 300.0, -3.0, 11.0], (n, 1))
    blocks = ctx.marginals_pairs(*a, pa, pb, **_kw(g))
    d = 2 if kind == 1 else 1
    for info in (hi, None):
        z, S, d2 = ctx.observation_covariance(*a, pa, pb, kinds, zh, info, **_kw(g))
        assert np.all(z[:, d:] == 0) and np.all(S[:, d:, :] == 0) and np.all(S[:, :, d:] == 0) and np.array_equal(S, np.transpose(S, (0, 2, 1)))
        zr, Sr, d2r, jn, (na, nab, nb) = A.observations(*a, vk, ek, pairs, kinds, zh, info, blocks=blocks)
        assert np.abs(z - zr).max() <= 1e-12 * max(1.0, np.abs(p).max())
        scale = jn ** 2 * (na + 2 * nab + nb)
        assert np.all(_nd(S - Sr) <= 1e-12 * scale)
        ze, Se, d2e, _, _ = A.observations(*a, vk, ek, pairs, kinds, zh, info)
        assert np.all(_nd(S - Se) <= AC.MARG_TAU * jn ** 2 * np.sqrt(na * nb))
        for k in range(n):
            M = Sr[k, :d, :d].copy()
            if info is not None:
                M += np.linalg.inv(np.array([[hi[k, 0], hi[k, 1]], [hi[k, 1], hi[k, 3]]])[:d, :d])
            e = (zr[k] - zh[k])[:d]
            if kind == 2:
                e = np.array([float(A.R.normalize_theta(e[0]))])
            y2 = np.linalg.norm(np.linalg.solve(M, e)) ** 2
            assert np.isfinite(d2r[k]) and d2[k] >= 0
            assert abs(d2[k] - d2r[k]) <= 1e-12 * (scale[k] * y2 + np.linalg.cond(M) * d2r[k]), (k, d2[k], d2r[k])
            assert abs(d2[k] - d2e[k]) <= AC.MARG_TAU * (jn[k] ** 2 * np.sqrt(na[k] * nb[k]) * y2 + np.linalg.cond(M) * d2e[k]), (k, d2[k], d2e[k])
    # outputs are nullable as in relative_covariance: no hypothesis, no d2
    z1, S1, none = ctx.observation_covariance(*a, pa, pb, kinds, **_kw(g))
    assert none is None and z1.tobytes() == z.tobytes() and S1.tobytes() == S.tobytes()
    # a list of mixed kinds: every pair as in its own list
    km = np.where(np.arange(n) % 2 == 0, kind, 3 - kind).astype(np.uint8)
    zm, Sm, dm = ctx.observation_covariance(*a, pa, pb, km, zh, hi, **_kw(g))
    zo, So, do = ctx.observation_covariance(*a, pa, pb, np.full(n, 3 - kind, np.uint8), zh, hi, **_kw(g))
    z, S, d2 = ctx.observation_covariance(*a, pa, pb, kinds, zh, hi, **_kw(g))
    ev = km == kind
    assert zm[ev].tobytes() == z[ev].tobytes() and Sm[ev].tobytes() == S[ev].tobytes() and dm[ev].tobytes() == d2[ev].tobytes()
    assert zm[~ev].tobytes() == zo[~ev].tobytes() and Sm[~ev].tobytes() == So[~ev].tobytes() and dm[~ev].tobytes() == do[~ev].tobytes()


def test_observation_covariance_mixed_with_pose_pairs(ctx):
    """Kind-0 pairs in a list with landmark pairs are relative_covariance's, bit for bit."""
    g, p = _optimised(ctx, "mixed5_257")
    a = (p,) + _a(g)[1:]
    P, L = g["P"], g["L"]
    pa = np.array([P[1], P[4], P[9], P[20], P[30]], np.int32)
    pb = np.array([P[8], L[3], P[2], L[11], P[31]], np.int32)
    kinds = np.array([0, 1, 0, 2, 0], np.uint8)
    zh = np.array([[0.5, 0.1, 0.2], [1.0, 1.0, 0], [0.3, -0.2, 0.1], [0.4, 0, 0], [1.0, 0.0, 0.0]])
    hi = np.tile([400.0, 30.0, 7.0, 300.0, -3.0, 900.0], (5, 1))
    z, S, d2 = ctx.observation_covariance(*a, pa, pb, kinds, zh, hi, **_kw(g))
    m = kinds == 0
    zr, Sr, dr = ctx.observation_covariance(*a, pa[m], pb[m], None, zh[m], hi[m], **_kw(g))
    assert z[m].tobytes() == zr.tobytes() and S[m].tobytes() == Sr.tobytes() and d2[m].tobytes() == dr.tobytes()
    assert np.all(np.isfinite(d2)) and np.all(S[1, 2, :] == 0) and np.all(S[3, 1:, :] == 0)


def test_observation_covariance_edge_cases(ctx):
    g, p = _optimised(ctx, "mixed5_257")
    vk = g["vk"]
    P, L = g["P"], g["L"]
    # (a) a point exactly on the pose: the bearing is 0, S and d2 are NaN; the kind-1 prediction stays finite
    q = p.copy()
    u, v = int(P[10]), int(L[0])
    q[v, :2] = q[u, :2]
    z, S, d2 = ctx.observation_covariance(q, *_a(g)[1:], [u, u, int(P[11])], [v, v, v], [2, 1, 2], np.zeros((3, 3)), None, **_kw(g))
    assert z[0].tolist() == [0.0, 0.0, 0.0] and np.isnan(S[0, 0, 0]) and np.isnan(d2[0]) and np.all(S[0].ravel()[1:] == 0)
    assert np.all(np.isfinite(S[1:])) and np.all(np.isfinite(d2[1:])) and np.all(z[1] == 0)
    # (b) both ends fixed and no measurement noise: S = 0 is not positive definite
    f = dict(g)
    f["fixed"] = g["fixed"].copy()
    f["fixed"][[u, int(L[5])]] = 1
    for kind in (1, 2):
        z, S, d2 = ctx.observation_covariance(p, *_a(f)[1:], [u], [int(L[5])], [kind], [[1.0, 1.0, 0.0]], None, **_kw(f))
        assert np.all(S == 0) and np.isnan(d2[0])
        _, _, d2 = ctx.observation_covariance(p, *_a(f)[1:], [u], [int(L[5])], [kind], [[1.0, 1.0, 0.0]], [[4.0, 0, 0, 4.0, 0, 0]], **_kw(f))
        assert np.isfinite(d2[0]) and d2[0] > 0
    # (c) a bearing hypothesis across +-pi: e is wrapped
    w = AC.case("bearing_wrap")
    pw = w["poses"]
    zw, Sw, dw = ctx.observation_covariance(pw, *_a(w)[1:], [0], [1], [2], [[np.pi - 0.01, 0, 0]], [[50.0, 0, 0, 0, 0, 0]], **_kw(w))
    assert zw[0, 0] < -3.0 and abs(zw[0, 0] - (np.pi - 0.01)) > 6.0
    e = float(A.R.normalize_theta(zw[0, 0] - (np.pi - 0.01)))
    assert abs(e) < 0.05 and dw[0] == pytest.approx(e * e / (Sw[0, 0, 0] + 1 / 50.0), rel=1e-12) and dw[0] < 1.0


def test_gating(ctx):
    """gateObservations is the listed-pairs call; every measurement generated from landmark k is nearest to column k."""
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
    c, p = _optimised(ctx, "mixed5_257")
    s = GraphSLAM(PoseGraph(np.arange(len(p)), p, c["fixed"], *_a(c)[2:], vertex_kind=c["vk"], edge_kind=c["ek"]), ctx)
    pose = int(c["P"][20])
    t = c["truth"]
    lm = []                                                       # landmarks at least 1 m away and 0.15 rad apart as seen from the pose
    for l in c["L"]:
        d = TC._rot(t[pose, 2]) @ (t[l, :2] - t[pose, :2])
        b = np.arctan2(d[1], d[0])
        if np.hypot(*d) >= 1.0 and all(abs(float(A.R.normalize_theta(b - o))) >= 0.15 for o in [x[1] for x in lm]):
            lm.append((int(l), b))
    lm = np.array([x[0] for x in lm][:6], np.int32)
    n = len(lm)
    assert n == 6
    rng = np.random.default_rng(12)
    rel = (TC._rot(t[pose, 2]) @ (t[lm, :2] - t[pose, :2]).T).T
    for kind, zz, info in ((1, rel + 0.01 * rng.standard_normal(rel.shape), np.tile([1e4, 0, 1e4], (n, 1))),
                           (2, np.arctan2(rel[:, 1], rel[:, 0]) + 0.002 * rng.standard_normal(n), np.full(n, 2.5e5))):
        d2 = s.gateObservations(pose, lm, zz, info, kind=kind)
        assert d2.shape == (n, n) and np.all(np.isfinite(d2))
        hm, hi = np.zeros((n, 3)), np.zeros((n, 6))
        if kind == 1:
            hm[:, :2], hi[:, [0, 1, 3]] = zz, info
        else:
            hm[:, 0], hi[:, 0] = zz, info
        pairs = [(pose, int(l)) for _ in range(n) for l in lm]
        listed = s.observationCovariance(pairs, [kind] * (n * n), (np.repeat(hm, n, axis=0), np.repeat(hi, n, axis=0)))[2]
        assert d2.tobytes() == listed.reshape(n, n).tobytes()
        assert np.array_equal(np.argmin(d2, axis=1), np.arange(n)), (kind, d2)


def test_refusals(ctx):
    g, p = _optimised(ctx, "mixed5_257")
    vk, ek = AC.kinds(g)
    a = (p,) + _a(g)[1:]
    P, L = g["P"], g["L"]
    pa, pb = np.array([P[1], P[2], P[3]], np.int32), np.array([L[1], L[2], P[9]], np.int32)
    good = np.array([1, 2, 0], np.uint8)
    ctx.observation_covariance(*a, pa, pb, good, **_kw(g))
    for kinds, pair in (([1, 3, 0], 1), ([1, 2, 1], 2), ([0, 2, 0], 0), ([1, 2, 2], 2)):
        with pytest.raises(CgmrError) as ei:
            ctx.observation_covariance(*a, pa, pb, kinds, **_kw(g))
        assert ei.value.code == -1 and f"pair {pair} " in str(ei.value), str(ei.value)
    with pytest.raises(CgmrError) as ei:                          # observed from a point
        ctx.observation_covariance(*a, [L[0]], [L[1]], [1], **_kw(g))
    assert ei.value.code == -1 and "pair 0 " in str(ei.value)
    with pytest.raises(CgmrError) as ei:                          # without types every vertex is a pose
        ctx.observation_covariance(*a, pa, pb, good)
    assert ei.value.code == -1 and "pair 0 " in str(ei.value)
    k0 = int(np.flatnonzero(ek == 0)[0])
    calls = (lambda kw: ctx.marginals_joint(*a, pa, **kw), lambda kw: ctx.marginals_pairs(*a, pa, pb, **kw),
             lambda kw: ctx.observation_covariance(*a, pa, pb, good, **kw), lambda kw: ctx.gn_optimize_typed(*a, 1, **kw))
    for bad in (5, 200):
        e2 = ek.copy()
        e2[k0] = bad
        for call in calls:
            with pytest.raises(CgmrError) as ei:
                call(dict(vertex_kind=vk, edge_kind=e2))
            assert ei.value.code == -1 and f"edge {k0} " in str(ei.value), str(ei.value)
    e2 = ek.copy()
    e2[k0] = 2                                                    # a bearing between two poses
    for call in calls:
        with pytest.raises(CgmrError) as ei:
            call(dict(vertex_kind=vk, edge_kind=e2))
        assert ei.value.code == -1 and f"edge {k0} " in str(ei.value)
    # the context works afterwards
    z, S, _ = ctx.observation_covariance(*a, pa, pb, good, **_kw(g))
    assert np.all(np.isfinite(S))


def test_graph_slam_routes_typed_graphs_to_the_typed_marginals(ctx):
    """On a typed graph computeMarginalBlocks, jointMarginal and relativeCovariance match the reference -- and differ by more
    than 1e-3 from what the plain calls return for the same arrays (a landmark observation read as an EDGE_SE2, a prior as
    nothing): the silent wrong answer is gone."""
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
    c, p = _optimised(ctx, "mixed5_257", fix=(int(AC.case("mixed5_257")["P"][7]),))
    vk, ek = AC.kinds(c)
    a = (p,) + _a(c)[1:]

    def plain_call(f):                                            # (the plain H of these arrays may not even factor)
        try:
            return f()
        except CgmrError:
            return None
    s = GraphSLAM(PoseGraph(np.arange(len(p)), p, c["fixed"], *_a(c)[2:], vertex_kind=vk, edge_kind=ek), ctx)
    P, L = c["P"], c["L"]
    pairs = [(int(P[2]), int(L[4])), (int(L[1]), int(L[9])), (int(P[5]), int(P[40])), (int(P[12]), int(P[12]))]
    diag, want, err = A.marginal_blocks(*a, vk, ek, pairs=pairs)
    assert err <= AC.REF_ERR_MAX
    got = s.computeMarginalBlocks(pairs)
    pa, pb = np.array(pairs, np.int32).T
    plain = plain_call(lambda: ctx.marginals_pairs(*a, pa, pb)[1])
    for k, pr in enumerate(pairs):
        sc = np.sqrt(np.linalg.norm(diag[pr[0]]) * np.linalg.norm(diag[pr[1]]))
        assert np.linalg.norm(got[pr] - want[k]) <= AC.MARG_TAU * sc
        assert plain is None or np.linalg.norm(plain[k] - want[k]) > 1e-3 * sc
    q = [int(P[2]), int(L[4]), int(P[30])]
    S = s.jointMarginal(q)
    _, cross, _ = A.marginal_blocks(*a, vk, ek, pairs=[(u, v) for u in q for v in q])
    ref = np.block([[cross[3 * i + j] for j in range(3)] for i in range(3)])
    assert np.linalg.norm(S - ref) <= AC.MARG_TAU * np.linalg.norm(ref) and np.array_equal(S, S.T) and np.all(S[5] == 0)
    Sp = plain_call(lambda: ctx.marginals_joint(*a, q))
    assert Sp is None or np.linalg.norm(Sp - ref) > 1e-3 * np.linalg.norm(ref)
    pp = [(int(P[5]), int(P[40])), (int(P[3]), int(P[4]))]
    z, Sz = s.relativeCovariance(pp)
    zr, Sr, _, jn, (na, _, nb) = A.observations(*a, vk, ek, pp, [0, 0])
    assert np.abs(z - zr).max() <= 1e-12 * max(1.0, np.abs(p).max())
    assert np.all(_nd(Sz - Sr) <= AC.MARG_TAU * jn ** 2 * np.sqrt(na * nb))
    Sp = plain_call(lambda: ctx.relative_covariance(*a, [u for u, _ in pp], [v for _, v in pp])[1])
    assert Sp is None or np.all(_nd(Sp - Sr) > 1e-3 * _nd(Sr))
    zh = (zr + 0.01, np.tile([400.0, 0, 0, 400.0, 0, 900.0], (2, 1)))
    assert np.all(np.isfinite(s.relativeCovariance(pp, zh)[2]))
