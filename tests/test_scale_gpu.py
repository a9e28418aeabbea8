"""The solver away from the information scale and the units of the synthetic recipes: every (case, family) of
tests/scale_cases.py on the device, every quantity per block by the block's own norm against the refined float64 / long double
truth, held to max(the quantity's existing bar, 10 e_ref) with e_ref the plain float64 path's error against the same truth as
tests/test_scale_cpu.py measures it (scale_cases.MEASURED).  One test per (case, family); nothing is skipped.

Each test prints one line per quantity, ``scale <case> <family> <quantity> e_dev e_ref e_dev/e_ref bar``; the Gauss-Newton step
is printed for the chained backward solve (Z^T v) and for the level-by-level one (substitution, CGMR_BWD_CHAIN=0) side by side."""
import numpy as np
import pytest

import ref_dogleg
import ref_lm
import ref_numpy as R
import ref_robust as RR
import ref_typed as RT
import remove_nodes_cases as K
import scale_cases as S
import test_dogleg_gpu as DL
import test_lm_gpu as LM
from reference_cases import OMEGA_MAX
from switch_contexts import assert_launch_shape, context_under, launch_counts
from test_robust_gpu import check_chi2, check_stats

pytestmark = pytest.mark.gpu

_IDENTITY = {}          # case -> what the weak / strong families compare their bytes with


@pytest.fixture(scope="module")
def ctx_levelwise():
    """The level-by-level backward solve: substitution with L11, no Z^T v."""
    env = {"CGMR_BWD_CHAIN": "0"}
    with context_under(env) as c:
        assert_launch_shape(c, env, S.args(S.graph("pg300", "identity")))      # one backward launch per level
        yield c


def _hold(name, family, quantity, e_dev, e_ref, existing=None):
    existing = S.EXISTING[quantity.split("/")[0]] if existing is None else existing
    b = S.bar(existing, e_ref)
    print(f"scale {name} {family} {quantity} {e_dev:.3e} {e_ref:.3e} {e_dev / e_ref if e_ref else float('inf'):.2f} {b:.3e}")
    assert e_dev <= b, (name, family, quantity, e_dev, e_ref, b)


def _ulps(a, b):
    """The largest distance of two float64 arrays in units of the last place of b."""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    sp = np.spacing(np.abs(b))
    return float(np.max(np.abs(a - b) / sp)) if len(a) else 0.0


def _step(c, g, p0, iters=1):
    a = S.args(g)
    vk, ek = S.kinds(g)
    if vk is None:
        rc, p1, chi = c.gn_optimize(p0, *a[1:], iters)
    else:
        rc, p1, chi = c.gn_optimize_typed(p0, *a[1:], iters, vertex_kind=vk, edge_kind=ek)
    assert rc == 0
    return p1, chi


def _omega(g, p0, p1):
    a = S.args(g)
    vk, ek = S.kinds(g)
    return R.step_backward_error(p0, p1, *a[1:]) if vk is None else RT.step_backward_error(p0, p1, *a[1:], vk, ek)


def _gn(ctx, ctx_levelwise, name, family, g, s, e_ref):
    """1. One step from the guess on both backward solves, then three more iterations."""
    dead = R.active_fixed(len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"]) != 0
    out = {}
    for label, c in (("chain", ctx), ("levelwise", ctx_levelwise)):
        p1, _ = _step(c, g, g["poses"])
        assert np.array_equal(p1[dead], g["poses"][dead])
        w = _omega(g, g["poses"], p1)
        assert w <= OMEGA_MAX, (name, family, label, w / R.U)
        out[label] = (s.step_error(s.step_of(p1)), w, p1, s.step_own_error(s.step_of(p1)))
    print(f"scale {name} {family} step forward error chain {out['chain'][0] / R.U:.2f} u, level by level {out['levelwise'][0] / R.U:.2f} u;"
          f" backward error {out['chain'][1] / R.U:.1f} u, {out['levelwise'][1] / R.U:.1f} u")
    for label in out:
        _hold(name, family, "step/" + label, out[label][0], e_ref["step"][0])
        if name in S.STEP_OWN:                                     # ... and by the blocks' own norms
            _hold(name, family, "step_own/" + label, out[label][3], s.step_own_error(s.dx_plain))
    if name in ("blobs20", "pg300") and family == "identity":      # the default context does chain its backward solve here
        from cg_mrslam_amd._lib import gn_symbolic_info
        levels = gn_symbolic_info(len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"])["launch_levels"]
        n = launch_counts(ctx, S.args(g))
        print(f"scale {name} backward-solve launches {n['solve_bwd']} on {levels} launch levels")
        assert name != "pg300" or n["solve_bwd"] < levels, (n, levels)
    p = out["chain"][2]
    for it in range(3):
        p_next, _ = _step(ctx, g, p)
        w = _omega(g, p, p_next)
        assert w <= OMEGA_MAX, (name, family, it + 1, w / R.U)
        p = p_next
    return out["chain"][2]


def _traces(ctx, name, family, g):
    """2. Levenberg-Marquardt and dogleg, five iterations, against ref_lm / ref_dogleg (pose graphs)."""
    a = S.args(g)
    floor = LM.rounding_floor(g)
    ref = ref_lm.lm_optimize(*a, LM.ITERS)
    rc, _, chi, lam, tri, done = ctx.lm_optimize(*a, LM.ITERS)
    assert rc == 0
    k = S.lm_decided(ref, family)                                  # (at least three: tests/test_scale_cpu.py)
    assert done >= min(k, ref["iters_done"])
    k_lm = LM.check_trace(f"{name}/{family}", S.lm_truncated(ref, k), chi[:k + 1], lam[:k], tri[:k], min(done, k), floor)
    ref = ref_dogleg.dl_optimize(*a, DL.ITERS)
    rc, _, chi, dlt, tri, stp, done = ctx.dl_optimize(*a, DL.ITERS)
    assert rc == 0
    k_dl = DL.check_trace(f"{name}/{family}", ref, chi, dlt, tri, stp, done, floor)
    print(f"scale {name} {family} traces compared: Levenberg {k_lm}, dogleg {k_dl} iterations")
    assert k_lm >= 1 and k_dl >= 1, (name, family, "nothing compared")


def _covariances(ctx, name, family, g, s, e_ref):
    """3. marginals (12 queries), marginals_all with cross blocks (pose graphs), marginals_typed over every vertex with a
    point's third row and column exactly zero (typed graphs), marginals_joint on 5 and 17 vertices."""
    a = S.args(g)
    vk, ek = S.kinds(g)
    V = len(g["poses"])
    q12, q5, q17 = S.queries(g)
    assert len(q12) == 12 and len(q5) == 5 and len(q17) == 17
    out = {}
    if vk is None:
        cov12 = ctx.marginals(*a, q12)
        assert not np.any(cov12[0]) and s.lay.off[q12[0]] < 0 and s.lay.off[q12[1]] >= 0      # the fixed vertex: exact zeros
        cov, cross = ctx.marginals_all(*a, cross=True)
        e12 = s.pair_error(cov12, [(int(v), int(v)) for v in q12])
        eall = s.pair_error(cov, [(v, v) for v in range(V)])
        edges = [(int(i), int(j)) for i, j in zip(g["edge_from"], g["edge_to"])]
        ecross = s.pair_error(cross, edges)
        _hold(name, family, "diag/marginals", e12, e_ref["diag"][0])
        _hold(name, family, "diag/marginals_all", eall, e_ref["diag"][0])
        _hold(name, family, "cross", ecross, e_ref["cross"][0])
        out.update(cov12=cov12, cov=cov, cross=cross)
        kw = {}
    else:
        cov = ctx.marginals_typed(*a, np.arange(V, dtype=np.int32), vertex_kind=vk, edge_kind=ek)
        pts = vk == 1
        assert pts.any() and not np.any(cov[pts, 2, :]) and not np.any(cov[pts, :, 2])         # a point's third row / column
        _hold(name, family, "diag/marginals_typed", s.pair_error(cov, [(v, v) for v in range(V)]), e_ref["diag"][0])
        out.update(cov=cov)
        kw = dict(vertex_kind=vk, edge_kind=ek)
    for q in (q5, q17):
        J = ctx.marginals_joint(*a, q, **kw)
        assert np.array_equal(J, J.T)
        blocks = S.joint_blocks(J, q)
        if vk is not None:
            for k, (u, v) in enumerate(S.joint_pairs(q)):
                assert not (vk[u] == 1 and np.any(blocks[k][2, :])) and not (vk[v] == 1 and np.any(blocks[k][:, 2]))
        _hold(name, family, f"joint/{len(q)}", s.pair_error(blocks, S.joint_pairs(q)), e_ref["joint"][0])
        out[f"joint{len(q)}"] = J
    return out


def _wire(ctx, name, family, gauge, to, est, iu):
    """The float32 wire round trip of condensed edges through the message path: finite, and the float32 nearest to the
    float64 value."""
    from cg_mrslam_amd.condensed import wire_narrow_edges
    ids = np.arange(int(max(to.max(), gauge)) + 1, dtype=np.int32)
    rec = wire_narrow_edges(ctx, gauge, to, ids, est, iu)
    assert np.array_equal(rec["from"], np.full(len(to), gauge)) and np.array_equal(rec["to"], to)
    assert np.all(np.isfinite(rec["est"])) and np.all(np.isfinite(rec["info"])), (name, family)
    assert np.array_equal(rec["est"], est.astype(np.float32)) and np.array_equal(rec["info"], iu.astype(np.float32))
    big = np.abs(iu).max(axis=1) > 0
    assert np.all(np.abs(rec["info"][big].astype(np.float64) - iu[big]).max(axis=1) <= 2.0 ** -24 * np.abs(iu[big]).max(axis=1))


def _condensed(ctx, name, family, g):
    """4. condense and condense_tree on 8 queries."""
    ref = S.condensed_reference(g)
    e_ref = ref["errors"]
    gauge, query, s = ref["gauge"], ref["query"], ref["solved"]
    a = S.args(g)
    to, est, iu, cov = ctx.condense(a[0], *a[2:], gauge, query)
    assert np.array_equal(to, ref["to"])
    _hold(name, family, "cond_cov", S.info_error(cov, ref["cov"]), e_ref["cond_cov"][0])
    _hold(name, family, "cond_est", S.est_error(est, ref["est"]), e_ref["cond_est"][0])
    # the labelling on the device's own blocks and its own step from the same guess, against long double
    rc, p1, _ = ctx.gn_optimize(ref["guess"], ref["fixed"], *a[2:], 1)
    assert rc == 0
    _, I_own = S.labels_extended(p1[gauge], p1[to], cov)
    _hold(name, family, "cond_info", S.info_error(R.info_full(iu), I_own), e_ref["cond_info"][0])
    if (name, family, "cond_path_info") not in S.PATH_INVALID:     # the whole path, where its truth is valid
        _hold(name, family, "cond_path_info", S.info_error(R.info_full(iu), ref["info"]), e_ref["cond_path_info"][0])
    _wire(ctx, name, family, gauge, to, est, iu)
    # the tree: its structure is the reference's (tests/test_scale_cpu.py holds the decision margin); every edge's measurement
    # against the truth, its information and weight on the device's own joint blocks and step against long double, and the
    # information of the whole path where its truth is valid -- all on the tree the device chose
    nodes = ref["nodes"]
    fr, to_t, est_t, iu_t, w, fl = ctx.condense_tree(a[0], *a[2:], gauge, query)
    assert np.array_equal(to_t, nodes[1:]) and not fl.any() and np.all(np.isfinite(w))
    idx = {int(v): k for k, v in enumerate(nodes)}
    parent = np.r_[-1, [idx[int(f)] for f in fr]]
    if (name, family) in S.TREE_TIED:                              # a minimum tree on the reference's weights either way
        total = sum(ref["W"][k, parent[k]] for k in range(1, len(nodes)))
        want = sum(ref["W"][k, ref["parent"][k]] for k in range(1, len(nodes)))
        assert abs(total - want) <= 1e-9 * len(to_t), (name, family, total, want)
    else:
        assert np.array_equal(parent, ref["parent"]), (name, family)
    S_own = ctx.marginals_joint(ref["guess"], ref["fixed"], *a[2:], nodes[1:])
    own = S.tree_labels(p1, nodes, parent, S_own, extended=True)
    truth = S.tree_labels(ref["p1"], nodes, parent, ref["Sigma"], extended=True)
    _hold(name, family, "tree_est", S.est_error(est_t, truth["est"]), e_ref["tree_est"][0])
    _hold(name, family, "tree_info", S.info_error(R.info_full(iu_t), own["info"]), e_ref["tree_info"][0])
    _hold(name, family, "tree_w", S.weight_error(w, own), e_ref["tree_w"][0])
    if (name, family, "tree_path_info") not in S.PATH_INVALID:
        _hold(name, family, "tree_path_info", S.info_error(R.info_full(iu_t), truth["info"]), e_ref["tree_path_info"][0])
    _wire(ctx, name, family, gauge, to_t, est_t, iu_t)
    return dict(est=est, iu=iu, cov=cov)


def _robust(ctx, name, family, g):
    """One Cauchy step against ref_robust at the bars of tests/test_robust_gpu.py."""
    a = S.args(g)
    kind, delta = 3, 3.0
    rc, p1, chi, e2, w = ctx.gn_optimize_robust(*a, 1, kind=kind, delta=delta)
    assert rc == 0
    check_chi2(chi[0], a[0], *a[2:], kind, delta)
    Ws = RR.scaled_info(a[0], *a[2:], kind, delta)
    om = R.step_backward_error(a[0], p1, a[1], *a[2:5], Ws)
    assert om <= OMEGA_MAX, (name, family, om / R.U)
    check_stats(p1, *a[2:], kind, delta, e2, w)
    assert (w < 0.9).any(), "no edge is down-weighted: the kernel does nothing here"


def _star(ctx, name, family, g):
    """6. remove_nodes on a star."""
    ref = S.star_reference(g)
    r = ref["plain"]
    nV, ef, et, meas, info, remove = S.star_args(g)
    out = ctx.remove_nodes(ef, et, meas, info, remove, num_vertices=nV)
    off, fr, to, z, iu, w, fl = out
    assert np.array_equal(fl, r["flags"]) and not fl.any()
    assert np.array_equal(off, r["off"]) and np.array_equal(fr, r["fr"]) and np.array_equal(to, r["to"])
    assert np.abs(w - r["weight"]).max() <= 0.5 * K.MARGIN_MIN
    _hold(name, family, "rm_est", S.est_error(z, ref["est"]), ref["errors"]["rm_est"][0])
    _hold(name, family, "rm_info", S.info_error(R.info_full(iu), ref["info"]), ref["errors"]["rm_info"][0])
    return out


def _scaled_bytes(name, family, what, got, want):
    """7. weak / strong against identity, byte for byte (the scaling is a power of two)."""
    same = np.asarray(got).tobytes() == np.asarray(want).tobytes()
    if not same:
        print(f"scale {name} {family} {what}: not identity's bytes, largest distance {_ulps(got, want):.1f} ulp")
    return same


@pytest.mark.parametrize("name,family", S.PAIRS)
def test_case_under_family(ctx, ctx_levelwise, name, family):
    kind = S.CASES[name][0]
    g = S.graph(name, family)
    f = {"weak": 2.0 ** -40, "strong": 2.0 ** 40}.get(family)
    needs_identity = f is not None or (kind == "star" and family == "far_origin")
    if needs_identity and name not in _IDENTITY:                   # (identity runs first; a run of this case alone makes it)
        test_case_under_family(ctx, ctx_levelwise, name, "identity")
    if kind == "star":
        out = _star(ctx, name, family, g)
        if family == "identity":
            _IDENTITY[name] = out
            for x, y in zip(out, ctx.remove_nodes(*S.star_args(S.base(name))[1:], num_vertices=S.base(name)["nV"])):
                assert x.tobytes() == y.tobytes()
        elif family == "far_origin":                               # the call takes no positions: the same input, the same bytes
            assert all(x.tobytes() == y.tobytes() for x, y in zip(out, _IDENTITY[name]))
        elif f is not None:
            base = _IDENTITY[name]
            ok = [_scaled_bytes(name, family, "remove_nodes " + what, out[k], base[k] * sc)
                  for k, what, sc in ((3, "measurements", 1.0), (4, "information", f))]
            assert all(ok) or not S.BYTE_IDENTICAL[name], (name, family, ok)
        return
    s = S.solved(g)
    e_ref = S.plain_errors(g, s)
    p1 = _gn(ctx, ctx_levelwise, name, family, g, s, e_ref)
    cov = _covariances(ctx, name, family, g, s, e_ref)
    cond = None
    if kind == "pose":
        _traces(ctx, name, family, g)
        if name in S.CONDENSED:
            cond = _condensed(ctx, name, family, g)
        if family == "edge_spread":
            _robust(ctx, name, family, g)
    if family == "identity":
        _IDENTITY[name] = dict(p1=p1, cov=cov, cond=cond)
        b = S.base(name)                                           # the harness adds nothing: the base graph's own bytes
        assert np.array_equal(_step(ctx, b, b["poses"])[0], p1)
    elif f is not None:
        base = _IDENTITY[name]
        ok = [_scaled_bytes(name, family, "step", p1, base["p1"])]
        ok += [_scaled_bytes(name, family, what, cov[what], base["cov"][what] / f) for what in cov]
        if cond is not None:
            ok += [_scaled_bytes(name, family, "condensed cov", cond["cov"], base["cond"]["cov"] / f)]
        assert all(ok) or not S.BYTE_IDENTICAL[name], (name, family, ok)
