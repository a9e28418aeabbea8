"""What tests/test_scale_gpu.py rests on, proved without a GPU: every (case, family, quantity) of tests/scale_cases.py is valid
(the truth's own error estimate is at most a hundredth of the float64 reference's error), scale_cases.MEASURED is current, the
decisions of the references (Levenberg-Marquardt's and dogleg's accept / reject, the spanning trees) are not taken within
rounding of their thresholds, ``identity`` hands the base graphs on byte for byte, the float64 reference is byte-identical
under a power-of-two scaling of the information, and the per-block norm sees one weak edge's information off by 1e-3."""
import numpy as np
import pytest

import ref_dogleg
import ref_lm
import ref_numpy as R
import ref_remove_nodes as RN
import scale_cases as S
import test_dogleg_gpu as DL
import test_lm_gpu as LM
from condense_tree_cases import MARGIN_MIN as TREE_MARGIN_MIN
from remove_nodes_cases import MARGIN_MIN as STAR_MARGIN_MIN

POSE_CASES = [n for n, (k, _) in S.CASES.items() if k == "pose"]


@pytest.mark.parametrize("name", list(S.CASES))
def test_identity_hands_the_base_graph_on_byte_for_byte(name):
    b, g = S.base(name), S.rescale(S.base(name), "identity")
    assert g is not b and set(g) == set(b)
    for k in b:
        assert np.asarray(g[k]).tobytes() == np.asarray(b[k]).tobytes(), k
    kind, mk = S.CASES[name]
    fresh = mk()                                                   # ... and the base graph is the builder's, rebuilt
    fresh = dict(zip(("nV", "edge_from", "edge_to", "meas", "info", "remove"), fresh)) if kind == "star" else fresh
    for k in fresh:
        assert np.asarray(fresh[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_rescale_is_deterministic_and_does_what_the_family_says():
    b = S.base("pg300")
    for fam in S.FAMILIES:
        x, y = S.rescale(b, fam), S.rescale(b, fam)
        assert all(np.array_equal(x[k], y[k]) for k in ("poses", "meas", "info")), fam
        O = R.info_full(x["info"])
        assert np.all(np.linalg.eigvalsh(O) > 0), fam              # every Omega stays positive definite
    O = R.info_full(S.rescale(b, "full_spread")["info"])
    ev = np.linalg.eigvalsh(O)
    assert ev.min() >= 10.0 * (1 - 1e-9) and ev.max() <= 1e5 * (1 + 1e-9) and ev.max() / ev.min() > 5e3
    d = S.rescale(b, "component_spread")["info"]
    assert not d[:, [1, 2, 4]].any() and d[:, [0, 3, 5]].min() >= 10 and d[:, [0, 3, 5]].max() <= 1e5
    r = S.rescale(b, "edge_spread")["info"][:, 0] / b["info"][:, 0]
    assert 1e-2 <= r.min() < 0.1 and 10 < r.max() <= 1e2
    assert np.array_equal(S.rescale(b, "heading_stiff")["info"][:, 5], b["info"][:, 5] * 1e6)
    assert np.array_equal(S.rescale(b, "heading_soft")["info"][:, 5], b["info"][:, 5] * 1e-3)
    mm = S.rescale(b, "millimetres")
    assert np.array_equal(mm["poses"][:, :2], b["poses"][:, :2] * 1000) and np.array_equal(mm["poses"][:, 2], b["poses"][:, 2])
    assert np.array_equal(mm["info"][:, 0], b["info"][:, 0] * 1e-6) and np.array_equal(mm["info"][:, 5], b["info"][:, 5])
    # the same chi2 in other units
    assert R.chi2(mm["poses"], *S.args(mm)[2:]) == pytest.approx(R.chi2(b["poses"], *S.args(b)[2:]), rel=1e-9)
    far = S.rescale(b, "far_origin")
    assert np.array_equal(far["meas"], b["meas"]) and np.array_equal(far["poses"][:, :2], b["poses"][:, :2] + 1e6)
    # at most one narrowed family per case, no family narrowed on two cases
    assert len({c for c, _ in S.NARROWED}) == len(S.NARROWED) == len({f for _, f in S.NARROWED})


@pytest.mark.parametrize("name,family", S.PAIRS)
def test_every_entry_is_valid_and_the_table_is_current(name, family):
    """The validity rule for every quantity, and MEASURED's e_ref within a factor 2 of what is measured now."""
    errors = S.reference_errors(name, family)
    table = S.MEASURED[(name, family)]
    assert set(table) == set(errors), (name, family)
    line = []
    for q, (e_ref, t_err) in errors.items():
        line.append(f"{q} {e_ref:.2e}/{t_err:.1e}")
        if (name, family, q) in S.PATH_INVALID:                    # a whole-path information that is not asserted: rightly so
            assert q.endswith("path_info") and not S.valid(S.EXISTING[q], e_ref, 3 * t_err), (name, family, q, e_ref, t_err)
        else:
            assert S.valid(S.EXISTING[q], e_ref, t_err), (name, family, q, e_ref, t_err)
        was = table[q][0]
        # (figures below the truth's own float64 rounding are noise: the existing bar is what is asserted there)
        if max(e_ref, was) > 100 * R.U:
            assert was / 2 <= e_ref <= was * 2, (name, family, q, e_ref, was)
    print(f"{name} {family}: e_ref / the truth's own estimate: " + ", ".join(line))


@pytest.mark.parametrize("name", POSE_CASES)
def test_no_decision_of_the_trust_region_references_is_taken_near_its_threshold(name):
    """Levenberg-Marquardt: the iterations tests/test_scale_gpu.py compares (scale_cases.lm_decided: every trial decided by
    more than RHO_MARGIN) are at least three on every family (the cliques are at their optimum after four).  Dogleg, among the iterations
    test_dogleg_gpu.compared_iterations compares: rho no nearer than RHO_MARGIN to 0, 0.25 and 0.75."""
    for family in S.FAMILIES:
        g = S.graph(name, family)
        a = S.args(g)
        floor = LM.rounding_floor(g)
        ref = ref_lm.lm_optimize(*a, LM.ITERS)
        k = S.lm_decided(ref, family)
        assert k >= 3, (name, family, k)
        assert LM.compared_iterations(S.lm_truncated(ref, k), floor)[0] >= 1, (name, family, "Levenberg: nothing compared")
        ref = ref_dogleg.dl_optimize(*a, DL.ITERS)
        k, _ = DL.compared_iterations(ref, floor)
        assert k >= 1, (name, family, "dogleg: nothing compared")
        for t in ref["trace"]:
            if t["iteration"] < k and np.isfinite(t["rho"]):
                assert min(abs(t["rho"] - x) for x in (0.0, 0.25, 0.75)) > S.RHO_MARGIN, (name, family, t)


@pytest.mark.parametrize("name", [n for n, (k, _) in S.CASES.items() if k == "star"] + list(S.CONDENSED))
def test_no_spanning_tree_is_decided_by_rounding(name):
    worst = np.inf
    for family in S.FAMILIES:
        g = S.graph(name, family)
        if S.CASES[name][0] == "star":
            m = RN.remove_nodes(*S.star_args(g))["margin"]
            assert m >= STAR_MARGIN_MIN, (name, family, m)
        else:
            m = S.condensed_reference(g)["tree_margin"]
            assert (m >= TREE_MARGIN_MIN) != ((name, family) in S.TREE_TIED), (name, family, m)
            if (name, family) in S.TREE_TIED:
                continue
        worst = min(worst, m)
    print(f"{name}: smallest decision margin over the families {worst:.2e} nats")


@pytest.mark.parametrize("name", ["clique40", "pg300", "leaf_and_hub"])
def test_float64_reference_is_byte_identical_under_a_power_of_two(name):
    """weak / strong scale H and b by 2^-+40 exactly: the unrefined SuperLU step has identity's bytes, np.linalg.inv's blocks
    identity's times 2^+-40 (no pivot changes, nothing over- or underflows)."""
    base = S.solved(S.graph(name, "identity"))
    for family, f in (("weak", 2.0 ** -40), ("strong", 2.0 ** 40)):
        s = S.solved(S.graph(name, family))
        assert np.array_equal(s.H.toarray(), base.H.toarray() * f) and np.array_equal(s.b, base.b * f)
        assert s.dx_plain.tobytes() == base.dx_plain.tobytes(), (name, family)
        assert s.inv_plain.tobytes() == (base.inv_plain / f).tobytes(), (name, family)


def test_a_weak_edge_wrong_by_a_thousandth_fails_per_block():
    """The mutation on the reference's side: one of the weakest edges of blobs20 under edge_spread with its information off by
    1e-3 of itself.  Some block of the inverse moves by 4.5e-8 of its own norm, 45 times its bar.  (Measured by the largest
    block's norm the same change is 2.4e-8: a weak edge makes the large blocks of a covariance, so here that norm sees it too;
    it is the information side -- condensed and removal edges -- where the weak blocks are the small ones.)"""
    g = S.graph("blobs20", "edge_spread")
    s = S.solved(g)
    w = np.linalg.norm(R.info_full(g["info"]), axis=(1, 2))
    leaf = (g["edge_from"] >= 20) & (g["edge_to"] >= 20)           # inside a blob, not on the separator
    k = int(np.flatnonzero(leaf)[np.argmin(w[leaf])])
    bad = dict(g, info=g["info"].copy())
    bad["info"][k] *= 1 + 1e-3
    sb = S.solved(bad)
    V = len(g["poses"])
    diag = [(v, v) for v in range(V)]
    e_ref = s.pair_error(None, diag, M=s.inv_plain)
    per_block = s.pair_error(None, diag, M=sb.inv)
    largest = max(np.linalg.norm(s.block(sb.inv, v, v) - s.block(s.inv, v, v)) for v in range(V)) / s.nd.max()
    print(f"edge {k} ({g['edge_from'][k]} -> {g['edge_to'][k]}), {w[k] / w.max():.1e} of the strongest: per block {per_block:.2e}, "
          f"of the largest block {largest:.2e}, bar {S.bar(S.EXISTING['diag'], e_ref):.1e}")
    assert per_block > S.bar(S.EXISTING["diag"], e_ref)
    assert largest <= per_block


def test_the_step_measure_holds_a_backward_stable_solve_and_sees_a_wrong_block():
    """Solved.step_error: the unrefined SuperLU step (backward error of a few u) is below u on every family of
    pg300, and a step with one vertex's solution off by 1e-9 of the scale of its own terms is above it."""
    for family in S.FAMILIES:
        s = S.solved(S.graph("pg300", family))
        if family != "far_origin":                                 # (there the pose update's rounding, 1.2e-10 m, is what shows)
            assert s.step_error(s.dx_plain) <= R.U, family
        dx = s.dx.copy()
        dx[30:33] += 1e-9 * s.dx_scale[30:33]
        assert s.step_error(dx) > 1e3 * S.STEP_FLOOR
