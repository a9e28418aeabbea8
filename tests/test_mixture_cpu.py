"""Max-mixture edges without a GPU: the contract of tests/ref_mixture.py against hand values, the reach predicates of
tests/mixture_cases.py proved on the reference alone, and the host layers (PoseGraph, GraphSLAM, .g2o, the bindings)."""
import numpy as np
import pytest

import mixture_cases as MC
import ref_mixture as RM
import ref_robust
import ref_typed

POS_TOL = 1e-6                     # the device-to-reference bar of tests/test_mixture_gpu.py, metres
SYMBOLS = ["cgmr_gn_optimize_mixture", "cgmr_gn_optimize_mixture_dev", "cgmr_lm_optimize_mixture", "cgmr_lm_optimize_mixture_dev",
           "cgmr_dl_optimize_mixture", "cgmr_dl_optimize_mixture_dev", "cgmr_mixture_select"]
GROSS = ("g60_k2_last", "g60_k5_random", "g300_k2_last", "g300_k5_random", "b255", "b256", "b257", "tie")


# ------------------------------------------------------------------------------------------------- the objective by hand
def test_anchor_offsets_and_threshold():
    g = MC.case("anchor_lo")
    c = RM.offsets(g["mix"])
    assert c[0] == 0.0 and c[1] == 0.0                                   # (one component: exactly 0, then the mixture's best)
    assert c[2] == pytest.approx(6 * np.log(10.0), rel=1e-15)
    assert MC.ANCHOR_R == pytest.approx(13.955061, rel=1e-6)
    for name, d, want in (("anchor_lo", 3.7, 0), ("anchor_hi", 3.8, 1)):
        g = MC.case(name)
        assert (d * d > MC.ANCHOR_R) == bool(want)
        sel, best, _ = RM.select(g["poses"], g["edge_from"], g["edge_to"], g["mix"])
        assert sel.tolist() == [0, want]
        assert best[1] == pytest.approx(min(d * d, 0.01 * d * d + 6 * np.log(10.0)), rel=1e-13)
        ref = MC.reference(name)
        assert ref["selected"].tolist() == [0, want] and all(s.tolist() == [0, want] for s in ref["sels"])


def test_threshold_is_where_the_two_costs_cross():
    """Just below and just above r_1 = 6 ln 10 / 0.99, at the poses themselves (no optimisation)."""
    g = MC.case("anchor_lo")
    for r1, want in ((MC.ANCHOR_R * (1 - 1e-9), 0), (MC.ANCHOR_R * (1 + 1e-9), 1)):
        mix = (g["mix"][0], g["mix"][1].copy(), g["mix"][2], g["mix"][3])
        mix[1][1:, 0] = 1.0 + np.sqrt(r1)
        assert RM.select(g["poses"], g["edge_from"], g["edge_to"], mix)[0][1] == want


def test_offsets_by_hand():
    """a = 2 ln w + ln det Omega over the factor's own dimension; c = max a - a."""
    u3 = [2.0, 0.5, 0.0, 3.0, 0.0, 4.0]                                  # det = 4 (2 * 3 - 0.25) = 23
    u3b = [1.0, 0.0, 0.0, 1.0, 0.0, 1.0]                                 # det = 1
    u2 = [2.0, 0.5, 7.0, 3.0, -3.0, 11.0]                                # leading 2x2: det = 5.75; the junk is not read
    u2b = [1.0, 0.0, 9.0, 2.0, 9.0, 9.0]                                 # det = 2
    ptr = np.array([0, 2, 4, 6, 7], np.int32)
    info = np.array([u3, u3b, u2, u2b, u3, u3b, [0.0] * 6])
    w = np.array([0.25, 0.75, 1.0, 3.0, 0.5, 0.5, -1.0])                 # (the last edge has one component: nothing is looked at)
    mix = (ptr, np.zeros((7, 3)), info, w)
    c = RM.offsets(mix, np.array([0, 1, 3, 4], np.uint8))
    a = [2 * np.log(0.25) + np.log(23.0), 2 * np.log(0.75), np.log(5.75), 2 * np.log(3.0) + np.log(2.0),
         2 * np.log(0.5) + np.log(23.0), 2 * np.log(0.5)]
    want = [max(a[0], a[1]) - a[0], max(a[0], a[1]) - a[1], max(a[2], a[3]) - a[2], max(a[2], a[3]) - a[3], 0.0, np.log(23.0), 0.0]
    np.testing.assert_allclose(c, want, rtol=1e-14, atol=1e-15)
    assert np.all(c >= 0) and c[4] == 0.0 and c[6] == 0.0


def test_one_component_is_the_plain_chi2():
    g = MC.case("g60_k2_last")["clean"]
    n = len(g["edge_from"])
    mix = (np.arange(n + 1, dtype=np.int32), g["meas"], g["info"], np.full(n, 0.3))
    a = (g["edge_from"], g["edge_to"])
    assert RM.chi2(g["poses"], *a, mix) == pytest.approx(ref_typed.R.chi2(g["poses"], *a, g["meas"], g["info"]), rel=1e-14)


def test_tie_goes_to_the_lowest_index():
    g = MC.case("tie")
    ref = MC.reference("tie")
    k = int(g["exempt"][0])
    assert np.array_equal(g["mix"][1][g["mix"][0][k]], g["mix"][1][g["mix"][0][k] + 1])
    assert ref["selected"][k] == 0 and all(s[k] == 0 for s in ref["sels"])


# ------------------------------------------------------------------------------------------------- the reach predicates
@pytest.mark.parametrize("name", list(MC.CASES))
def test_reach_gauss_newton(name):
    g, ref = MC.case(name), MC.reference(name)
    assert len(ref["visits"].gap) == g["iters"] + 1
    assert ref["visits"].min_gap > MC.MARGIN, ref["visits"].min_gap
    assert len(g["multi"]) > 0 and np.all(np.isfinite(ref["chi2"])) and ref["chi2"][-1] <= ref["chi2"][0]


@pytest.mark.parametrize("alg", ["lm", "dl"])
@pytest.mark.parametrize("name", MC.TRUST_REGION)
def test_reach_trust_region(name, alg):
    ref = MC.reference(name, alg)
    assert ref["visits"].min_gap > MC.MARGIN, ref["visits"].min_gap
    assert ref["out"]["iters_done"] == MC.TR_ITERS and ref["chi2"][-1] < 1e-2 * ref["chi2"][0]


@pytest.mark.parametrize("n", [255, 256, 257])
def test_boundary_cases_have_their_edges(n):
    g = MC.case(f"b{n}")
    assert len(g["edge_from"]) == n
    assert set(k for k in (0, 255, 256, n - 1) if k < n) <= set(g["multi"].tolist())


def test_typed_case_is_decided_by_the_offsets():
    g, ref = MC.case("typed"), MC.reference("typed")
    ek, k = g["ek"], g["prior"]
    assert ek[k] == 3 and np.any(ek[g["multi"]] == 1)
    c = RM.offsets(g["mix"], ek)
    p0 = g["mix"][0][k]
    assert c[p0] == pytest.approx(6 * np.log(10.0), rel=1e-12) and c[p0 + 1] == 0.0
    for x, sel in zip([g["poses"], ref["poses"]], [ref["sels"][0], ref["selected"]]):
        cost = RM.component_costs(x, g["edge_from"], g["edge_to"], g["mix"], ek)
        r = cost - c
        assert r[p0] < r[p0 + 1] and sel[k] == 1                         # r alone picks the null component, r + c the real one
    obs = g["multi"][ek[g["multi"]] == 1]
    np.testing.assert_allclose(c[g["mix"][0][obs]], 0.0, atol=0)          # the 2x2 determinants: det(Omega / 2) = det / 4
    np.testing.assert_allclose(c[g["mix"][0][obs] + 1], np.log(4.0), rtol=1e-12)


# ------------------------------------------------------------------------------------------------- what the method does
@pytest.mark.parametrize("name", GROSS)
def test_gross_alternatives_end_at_the_clean_optimum(name):
    g, ref = MC.case(name), MC.reference(name)
    clean = MC.clean_optimum(name)
    d_mix, d_plain = ref_robust.rms(ref["poses"], clean), ref_robust.rms(MC.plain_on_component0(name), clean)
    assert d_mix < 1e-6 * POS_TOL and d_plain > 10.0, (d_mix, d_plain)   # (measured: at most 5.5e-14 m against 11 to 22 m)
    assert all(ref["selected"][k] == t for k, t in g["true_at"].items())


def test_true_component_first_is_the_plain_graph():
    name = "g60_k2_first"
    assert ref_robust.rms(MC.reference(name)["poses"], MC.plain_on_component0(name)) < 1e-12
    assert not MC.reference(name)["selected"].any()


def test_figures_of_the_larger_gross_case():
    ref = MC.reference("g300_k2_last")
    assert ref["chi2"][-1] == pytest.approx(2150.766978, abs=1e-6)


def test_switching_case_switches_and_settles():
    g, ref = MC.case("switching"), MC.reference("switching")
    sels = ref["sels"] + [ref["selected"]]
    changes = [int((sels[i] != sels[i - 1]).sum()) for i in range(1, len(sels))]
    wrong0 = sum(1 for k, t in g["true_at"].items() if sels[0][k] != t)
    assert wrong0 == 22 and changes[:2] == [19, 3] and not any(changes[2:]), (wrong0, changes)
    clean = MC.clean_optimum("switching")
    d_mix, d_plain = ref_robust.rms(ref["poses"], clean), ref_robust.rms(MC.plain_on_component0("switching"), clean)
    assert d_mix < 1e-6 * POS_TOL and d_plain > 1.0, (d_mix, d_plain)     # (measured: 7.8e-14 m against 3.8 m)
    assert ref["visits"].min_gap > 1e-2                                   # (measured: 1.87e-2)


def test_null_hypothesis_takes_the_corrupted_closures():
    g, ref = MC.case("null"), MC.reference("null")
    assert np.all(ref["selected"][g["bad"]] == 1)
    odo = np.setdiff1d(np.arange(len(g["edge_from"])), g["closure"])
    assert not ref["selected"][odo].any()


# ------------------------------------------------------------------------------------------------- the host layers
class _FakeCtx:
    """Stands in for the device in the calls that need nothing but a selection."""

    def __init__(self, sel):
        self.sel = sel

    def mixture_select(self, *a, **kw):
        return 0.0, self.sel


def _graph_of(name, drop_junk=False):
    """The case as a PoseGraph.  drop_junk: zeros in the entries a 2-dimensional factor ignores (the typed case fills them with
    junk on purpose; the .g2o lines of those kinds do not carry them)."""
    from cg_mrslam_amd.graph import PoseGraph
    g = MC.case(name)
    if drop_junk and g["ek"] is not None:
        ptr, cm, ci, cw = (a.copy() for a in g["mix"])
        two = np.isin(g["ek"], (1, 4))[RM._owner(ptr)]
        cm[two, 2] = 0.0
        ci[np.ix_(two, [2, 4, 5])] = 0.0
        g = dict(g, mix=(ptr, cm, ci, cw), meas=cm[ptr[:-1]], info=ci[ptr[:-1]])
    pg = PoseGraph(np.arange(len(g["poses"])), g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"],
                   vertex_kind=g["vk"], edge_kind=g["ek"])
    ptr, cm, ci, cw = g["mix"]
    for k in g["multi"]:
        pg.set_edge_mixture(int(k), [(cw[p], cm[p], ci[p]) for p in range(ptr[k], ptr[k + 1])])
    return g, pg


@pytest.mark.parametrize("name", ["g60_k5_random", "typed"])
def test_posegraph_holds_the_mixture(name):
    g, pg = _graph_of(name, drop_junk=True)
    assert pg.has_mixtures and np.array_equal(pg.meas, g["meas"]) and np.array_equal(pg.info, g["info"])
    for got, want in zip(pg.mixture_arrays(), g["mix"]):
        assert np.array_equal(got, want)
    pg.set_edge_mixture(int(g["multi"][0]), [(1.0, g["meas"][g["multi"][0]], g["info"][g["multi"][0]])])
    assert int(g["multi"][0]) not in pg.mixtures


def test_graph_without_mixtures_is_as_before():
    from cg_mrslam_amd.graph import PoseGraph
    g = MC.case("g60_k2_last")["clean"]
    pg = PoseGraph.from_synth(g)
    assert not pg.has_mixtures and pg.mixture_arrays() is None


@pytest.mark.parametrize("name", ["g60_k5_random", "typed"])
def test_g2o_round_trip(name, tmp_path):
    from cg_mrslam_amd.graph import PoseGraph
    g, pg = _graph_of(name, drop_junk=True)
    path = tmp_path / "m.g2o"
    pg.save_g2o(path, precision=17)
    text = path.read_text()
    assert "EDGE_SE2_MIXTURE" in text or name == "typed"
    back = PoseGraph.load_g2o(path)
    assert np.array_equal(back.meas, pg.meas) and np.array_equal(back.info, pg.info)
    assert np.array_equal(back.edge_from, pg.edge_from) and np.array_equal(back.edge_to, pg.edge_to)
    assert sorted(back.mixtures) == sorted(pg.mixtures)
    for got, want in zip(back.mixture_arrays(), pg.mixture_arrays()):
        assert np.array_equal(got, want)
    line = next(l for l in text.splitlines() if l.startswith("EDGE_SE2_MIXTURE")) if name != "typed" else None
    if line:
        tok = line.split()
        assert len(tok) == 4 + 10 * int(tok[3])


def test_g2o_without_the_tag_is_byte_for_byte_as_before(tmp_path):
    from cg_mrslam_amd.graph import PoseGraph
    g = MC.case("typed")
    pg = PoseGraph(np.arange(len(g["poses"])), g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"],
                   vertex_kind=g["vk"], edge_kind=g["ek"])
    a, b = tmp_path / "a.g2o", tmp_path / "b.g2o"
    pg.save_g2o(a)
    text = a.read_text()
    assert "MIXTURE" not in text
    # the writer's lines for a graph without mixtures, spelled out: nothing of the new tags, one line per vertex / FIX / edge
    n_lines = len(g["poses"]) + int(g["fixed"].sum()) + len(g["edge_from"])
    assert len(text.splitlines()) == n_lines
    back = PoseGraph.load_g2o(a)
    assert not back.has_mixtures
    back.save_g2o(b)
    assert b.read_bytes() == a.read_bytes()


def test_add_null_hypothesis_builds_the_case():
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
    g = MC.case("null")
    pg = PoseGraph(np.arange(len(g["poses"])), g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"])
    slam = GraphSLAM(pg, ctx=_FakeCtx(None))
    slam.addNullHypothesis(g["closure"], weight=1.0, scale=MC.NULL_SCALE)
    for got, want in zip(pg.mixture_arrays(), g["mix"]):
        assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        slam.addNullHypothesis([0], weight=0.0)
    with pytest.raises(ValueError):
        slam.addNullHypothesis([len(g["edge_from"])])


def test_add_mixture_edge_and_set_edge_mixture():
    from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
    g = MC.case("anchor_lo")
    ptr, cm, ci, cw = g["mix"]
    pg = PoseGraph([0, 1], g["poses"], g["fixed"], g["edge_from"][:1], g["edge_to"][:1], g["meas"][:1], g["info"][:1])
    slam = GraphSLAM(pg, ctx=_FakeCtx(None))
    k = slam.addMixtureEdge(0, 1, [(cw[p], cm[p], ci[p]) for p in (1, 2)])
    assert k == 1 and np.array_equal(pg.meas, g["meas"]) and np.array_equal(pg.info, g["info"])
    for got, want in zip(pg.mixture_arrays(), g["mix"]):
        assert np.array_equal(got, want)
    slam.setEdgeMixture(1, [(1.0, cm[1], ci[1])])
    assert pg.mixture_arrays() is None
    with pytest.raises(ValueError):
        slam.addMixtureEdge(0, 1, [])


def test_collapse_mixtures():
    from cg_mrslam_amd.graph import GraphSLAM
    g, pg = _graph_of("g60_k5_random")
    ref = MC.reference("g60_k5_random")
    pg.poses[:] = ref["poses"]
    out = GraphSLAM(pg, ctx=_FakeCtx(ref["selected"])).collapseMixtures()
    meas, info = RM.selected_graph(g["mix"], ref["selected"])
    assert not out.has_mixtures and np.array_equal(out.meas, meas) and np.array_equal(out.info, info)
    assert np.array_equal(out.meas, g["clean"]["meas"])                   # the true components: the clean graph
    assert pg.has_mixtures and np.array_equal(pg.meas, g["meas"])          # the graph itself is untouched


def test_value_errors():
    from cg_mrslam_amd.graph import GraphSLAM
    _, pg = _graph_of("g60_k2_last")
    slam = GraphSLAM(pg, ctx=_FakeCtx(None))
    with pytest.raises(ValueError, match="mixture"):
        slam.optimizeGNC()
    slam.setRobustKernel("Cauchy", 1.0)
    for alg in ("gn", "levenberg", "dl"):
        slam.algorithm = alg
        with pytest.raises(ValueError, match="mixture"):
            slam.optimize(3)
    with pytest.raises(ValueError):
        pg.set_edge_mixture(len(pg.edge_from), [(1.0, [0, 0, 0], MC.I3)])
    from cg_mrslam_amd._lib import mixture_arrays
    with pytest.raises(ValueError):
        mixture_arrays((np.zeros(3, np.int32), np.zeros((0, 3)), np.zeros((0, 6)), np.zeros(0)), 5)
    with pytest.raises(ValueError):
        mixture_arrays((np.array([0, 1, 3], np.int32), np.zeros((2, 3)), np.zeros((2, 6)), np.zeros(2)), 2)


def test_header_declares_and_python_binds_every_symbol():
    from cg_mrslam_amd import _lib
    declared = _lib.declared_symbols()
    for s in SYMBOLS:
        assert s in declared and s in _lib._SYMBOLS, s
    for m in ("gn_optimize_mixture", "gn_optimize_mixture_dev", "lm_optimize_mixture", "lm_optimize_mixture_dev", "dl_optimize_mixture",
              "dl_optimize_mixture_dev", "mixture_select"):
        assert callable(getattr(_lib.Context, m)), m
    assert [f[0] for f in _lib.Mixture._fields_] == ["comp_ptr", "comp_meas", "comp_info", "comp_weight", "selected_out"]
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cgmr.h")).read()
    assert "typedef struct cgmr_mixture {" in hdr
    for f in ("comp_ptr", "comp_meas", "comp_info", "comp_weight", "selected_out"):
        assert f in hdr
    from cg_mrslam_amd.graph import GraphSLAM
    for m in ("addMixtureEdge", "setEdgeMixture", "addNullHypothesis", "selectedComponents", "mixtureChi2", "collapseMixtures"):
        assert callable(getattr(GraphSLAM, m)), m
