"""The step table of the call-order tests (tests/test_call_order_cpu.py, tests/test_call_order_gpu.py).  TEST INFRASTRUCTURE ONLY.

A *step* makes one library call on the context it is given and returns everything the call returns; its inputs come from the
builders the features' own test files use and from the float64 references, never from another step, so a step's result is a
function of the context's past alone.  The GPU test runs every step on a fresh context (the baseline), then the whole table in
several orders on ONE context, and compares bytes.

What a ``cgmr_ctx`` carries from call to call (csrc/cgmr_ctx.h), and the steps that are there for it:
  the arenas and the graveyard          structures much smaller (gn_v5e4) and much larger (gn_lat40) than pg500, typed / mixture /
                                        robust / trust-region / matcher / scan calls in between
  the cached analysis and structure     17 steps on pg500's edge list (cache hits with other numbers), the other structures
                                        (misses), ``growth`` (the one extension), cache_off / cache_on
  GnDevice::pan_clean                   fail_leaf / fail_top / fail_lm / fail_marginals_all: a pass that fails below the top block
                                        of the cached structure, in front of a pass that skips the memset
  the matcher's table cache             match_default / match_kr_03 (two mtab_key values)
  pinned staging, the column mask       every host-pointer call; condense* / covariance_estimate (a gauge instead of the fixed flags)
  profiling mode                        profiling_on / profiling_off
  the side stream                       not here: the asynchronous batches have their own order tests (test_multirobot_gpu.py)
  fwd_merge_any                         no step provokes a time-out; the GPU test asserts gn_timeouts() == 0 at the end
"""
import os
from collections import namedtuple

import numpy as np

import assoc_cases as AC
import jcbb_cases as JC
import matcher_configs as MCFG
import mixture_cases as MC
import occupancy_cases as OC
import ref_numpy as R
import ref_typed as RT
import reference_cases as C
import remove_nodes_cases as RN
import scan_info_cases as SC
import typed_cases as TC
from cg_mrslam_amd import synth
from cg_mrslam_amd._lib import CgmrError, gn_front_table, gn_symbolic_info

# name: what pytest prints; run(ctx) -> the call's results; uses: the Context methods the step calls; tags: "pg500" (the call is
# on pg500's edge list), "panels" (a pg500 step that reads the assembled panels of the tree levels), "fail", "refused", "mode",
# "growth"; edges: the (edge_from, edge_to) lists the step hands to the solver, in call order
Step = namedtuple("Step", "name run uses tags edges")

GN_ITERS = 5
SKIP_KEYS = ("kernel_seconds",)          # wall-clock figures among a call's results: not a function of the inputs

_MEMO = {}


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def flat(out, path="out"):
    """A call's results as a list of (label, array): tuples, lists and dicts are walked, None is left out, scalars become
    0-d arrays of their own type (bool, int64, float64)."""
    if out is None:
        return []
    if isinstance(out, dict):
        return [x for k in sorted(out) if k not in SKIP_KEYS for x in flat(out[k], f"{path}[{k!r}]")]
    if isinstance(out, (tuple, list)):
        return [x for i, v in enumerate(out) for x in flat(v, f"{path}[{i}]")]
    return [(path, np.asarray(out))]


def first_difference(got, want):
    """None, or a sentence on the first output of ``got`` (a flat list) that is not ``want``'s in dtype, shape or bytes."""
    if [k for k, _ in got] != [k for k, _ in want]:
        return f"outputs {[k for k, _ in got]} instead of {[k for k, _ in want]}"
    for (k, a), (_, b) in zip(got, want):
        if a.dtype != b.dtype or a.shape != b.shape:
            return f"{k}: {a.dtype}{a.shape} instead of {b.dtype}{b.shape}"
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero(np.frombuffer(a.tobytes(), np.uint8) != np.frombuffer(b.tobytes(), np.uint8))
            at = int(bad[0]) // max(a.itemsize, 1)
            return f"{k}: {len(bad)} bytes differ, first in element {at}: {a.reshape(-1)[at]!r} instead of {b.reshape(-1)[at]!r}"
    return None


def status_or_error(call):
    """What a call that may fail hands back: its results, or ("error", code) when the wrapper raises."""
    try:
        return ("ok", call())
    except CgmrError as e:
        return ("error", int(e.code))


# ------------------------------------------------------------------------------------------------------------ inputs
def pg500():
    return _memo("pg500", C.CASES["pg500"][0])


def pg500_args():
    return C.args(pg500())


def pg500_optimised():
    """pg500's poses after GN_ITERS iterations of the float64 reference: where the marginal calls linearise."""
    return _memo("pg500_opt", lambda: R.gn_optimize(*pg500_args(), GN_ITERS)[0])


def pg500_perturbed_meas():
    g = pg500()
    return _memo("pg500_meas2", lambda: g["meas"] + np.random.default_rng(500).normal(0.0, 1e-3, g["meas"].shape))


def pg500_shape():
    """(info, front table, vertex -> block column, fronts of the top block) of pg500: the walk of boundary_cases.shape."""
    def make():
        g = pg500()
        a = (len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"])
        info, perm = gn_symbolic_info(*a, want_perm=True)
        t = gn_front_table(*a)
        top, f = set(), len(t) - 1
        for _ in range(info["top_block_fronts"]):
            top.add(f)
            nxt = [c for c in range(len(t)) if t[c, 3] == f and t[c, 0] + t[c, 1] == t[f, 0] and t[c, 4] == t[f, 4] - 1]
            f = nxt[0] if nxt else -1
        return info, t, perm, top
    return _memo("pg500_shape", make)


def front_of(vertex):
    _, t, perm, _ = pg500_shape()
    col = int(perm[vertex])
    return int(np.flatnonzero((t[:, 0] <= col) & (col < t[:, 0] + t[:, 1]))[0])


def fail_vertex(where):
    """The vertex of the first block column of front 0 ("leaf") or of the root front ("top")."""
    _, t, perm, _ = pg500_shape()
    col = int(t[0 if where == "leaf" else len(t) - 1, 0])
    return int(np.flatnonzero(perm == col)[0])


def fail_args(where):
    """pg500 with the information of every edge at fail_vertex(where) set to zero: that vertex's diagonal block of H is exactly
    zero, the factorisation stops at its first pivot."""
    def make():
        g, v = pg500(), fail_vertex(where)
        info = g["info"].copy()
        info[(g["edge_from"] == v) | (g["edge_to"] == v)] = 0.0
        return (g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], info)
    return _memo(("fail", where), make)


QUERY = np.array([3, 77, 250, 251, 499], dtype=np.int32)
PAIR_A = np.array([3, 77, 250, 499, 12], dtype=np.int32)
PAIR_B = np.array([77, 3, 251, 0, 400], dtype=np.int32)
GAUGE = 0


def pg120():
    return _memo("pg120", lambda: synth.make_pose_graph(120, 300, seed=48))          # test_pcm_gpu._optimised's graph


def pg120_closures():
    """The candidates of test_pcm_gpu's generator 3 at the float64 optimum of pg120."""
    def make():
        import test_pcm_gpu as TP
        g = pg120()
        p = R.gn_optimize(*C.args(g), TP.GN_ITERS)[0]
        ca, cb, z, _ = TP._pg120_candidates(p, 3)
        return p, ca, cb, z, np.tile(TP.IU, (len(ca), 1)), TP.GAMMA
    return _memo("pg120_closures", make)


def typed_case():
    g = TC.case("mixed257")
    vk, ek = TC.kinds(g)
    p = _memo("mixed257_opt", lambda: RT.gn_optimize(*TC.args(g), 3, vk, ek)[0])
    return g, dict(vertex_kind=vk, edge_kind=ek), p


def jcbb_graph():
    def make():
        g = AC.case("mixed5_256")
        return g, RT.gn_optimize(*AC.args(g), 3, g["vk"], g["ek"])[0], JC.graph_scene(g)
    return _memo("jcbb_graph", make)


def _overlapping(r):
    import ref_scan_info as RS
    w = [RS.window(h, m) for h, m in r["counts"]]
    return any(SC._overlap(w[i], w[j]) for i in range(len(w)) for j in range(i))


def scan_case():
    """The scan_info_cases case with the fewest range readings among those with two overlapping windows."""
    def make():
        names = sorted((n for n in SC.CASES if n != "prune_alloc"), key=lambda n: (np.size(SC.CASES[n]["scans"]), n))
        return next(n for n in names if _overlapping(SC.resolved(n)))
    return SC.resolved(_memo("scan_case", make))


def golden_pairs():
    return _memo("golden", lambda: dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match_close12.npz"))))


MATCH_OTHER = "kr_03"                     # matcher_configs.CONFIGS: another kernel range, so another mtab_key


def growth_lists():
    """pg500's edges ordered by their later vertex (test_reference_gpu.py's grown graph): the first ``ne`` join the first 400
    vertices."""
    def make():
        g = pg500()
        last = np.maximum(g["edge_from"], g["edge_to"])
        k = np.argsort(last, kind="stable")
        ef, et, meas, info = (np.ascontiguousarray(g[n][k]) for n in ("edge_from", "edge_to", "meas", "info"))
        return ef, et, meas, info, int(np.searchsorted(last[k], 400))
    return _memo("growth", make)


GROW_V = 400


# ------------------------------------------------------------------------------------------------------------- steps
def _pg(name, call, uses, panels=False):
    g = pg500()
    return Step(name, call, (uses,), ("pg500", "panels") if panels else ("pg500",), [(g["edge_from"], g["edge_to"])])


def _gn_dev(ctx):
    import torch
    g = pg500()
    dp, dm, di = (torch.from_numpy(np.ascontiguousarray(g[k], dtype=np.float64)).to("cuda:0") for k in ("poses", "meas", "info"))
    torch.cuda.synchronize()
    out = ctx.gn_optimize_dev(dp.data_ptr(), len(g["poses"]), g["fixed"], g["edge_from"], g["edge_to"], dm.data_ptr(), di.data_ptr(), GN_ITERS)
    ctx.synchronize()
    return out + (dp.cpu().numpy(),)


def _marg(method, *tail, **kw):
    def run(ctx):
        a = pg500_args()
        return getattr(ctx, method)(pg500_optimised(), *a[1:], *tail, **kw)
    return run


def _cond(method, **kw):
    def run(ctx):
        a = pg500_args()
        return getattr(ctx, method)(pg500_optimised(), *a[2:], GAUGE, QUERY, **kw)
    return run


def _pg500_steps():
    a = pg500_args()
    a2 = a[:4] + (pg500_perturbed_meas(), a[5])
    return [
        _pg("gn_pg500", lambda ctx: ctx.gn_optimize(*a, GN_ITERS), "gn_optimize", panels=True),
        _pg("gn_pg500_perturbed", lambda ctx: ctx.gn_optimize(*a2, GN_ITERS), "gn_optimize", panels=True),
        _pg("lm_pg500", lambda ctx: ctx.lm_optimize(*a, GN_ITERS), "lm_optimize", panels=True),
        _pg("dl_pg500", lambda ctx: ctx.dl_optimize(*a, GN_ITERS), "dl_optimize", panels=True),
        _pg("gn_robust_pg500", lambda ctx: ctx.gn_optimize_robust(*a, GN_ITERS, kind="cauchy", delta=1.0), "gn_optimize_robust"),
        _pg("gnc_pg500", lambda ctx: ctx.gnc_optimize(*a, max_outer=4), "gnc_optimize"),
        _pg("chordal_pg500", lambda ctx: ctx.chordal_initialize(*a), "chordal_initialize"),
        _pg("gn_dev_pg500", _gn_dev, "gn_optimize_dev"),
        _pg("marginals_pg500", _marg("marginals", QUERY), "marginals"),
        _pg("marginals_all_pg500", _marg("marginals_all", cross=True), "marginals_all", panels=True),
        _pg("marginals_joint_pg500", _marg("marginals_joint", QUERY), "marginals_joint"),
        _pg("marginals_pairs_pg500", _marg("marginals_pairs", PAIR_A, PAIR_B), "marginals_pairs"),
        _pg("relative_covariance_pg500", _marg("relative_covariance", PAIR_A, PAIR_B), "relative_covariance"),
        _pg("covariance_estimate_pg500", _cond("covariance_estimate"), "covariance_estimate"),
        _pg("condense_pg500", _cond("condense"), "condense"),
        _pg("condense_tree_pg500", _cond("condense_tree"), "condense_tree", panels=True),
        _pg("condense_robust_pg500", _cond("condense_robust", kind="cauchy", delta=1.0), "condense_robust"),
    ]


def _plain(name, case, iters):
    g = _memo(("case", case), C.CASES[case][0])
    return Step(name, lambda ctx: ctx.gn_optimize(*C.args(g), iters), ("gn_optimize",), (), [(g["edge_from"], g["edge_to"])])


def _match(kernel_range):
    def run(ctx):
        from cg_mrslam_amd.matcher import ScanMatcher
        d = golden_pairs()
        m = ScanMatcher(ctx, d["ranges_ref"].shape[1], float(d["angle_min"]), float(d["angle_inc"]), float(d["max_range"]),
                        kernel_range=kernel_range)
        return m.closeScanMatching(d["ranges_ref"], d["ranges_qry"], d["guess"])
    return run


def _occupancy(ctx):
    from test_occupancy_cases_gpu import _mirror
    g = _mirror(ctx, OC.resolved("multi_block"))
    ok = g.computeMap()
    return bool(ok), g.hits, g.misses, g.image


def _scan(which):
    def run(ctx):
        import test_scan_info_gpu as TS
        r = scan_case()
        return TS._info(ctx, r) if which == "information" else TS._prune(ctx, r)
    return run


def _robot_round(ctx):
    """One synchronous round of a robot that owns pg120 and has been asked for twelve vertices by its one peer."""
    from cg_mrslam_amd.condensed import RobotGraph
    g = pg120()
    ids = g["ids"].astype(np.int64)
    want = np.sort(np.random.default_rng(120).choice(len(ids), 12, replace=False)).astype(np.int32)
    rg = RobotGraph(ctx, 0, 2)
    try:
        rg.add_vertices(ids, g["poses"], g["fixed"])
        rg.add_edges(ids[g["edge_from"]], ids[g["edge_to"]], g["meas"], g["info"])
        rc, chi = rg.optimize(GN_ITERS)
        rg.insertOutClosure(1, ids[want])
        built = rg.computeCondensedGraph(-1)
        return (rc, chi, built, rg.poses()) + rg.condensed(1)
    finally:
        rg.close()


def _other_steps():
    tg, tkw, tp = typed_case()
    ta = TC.args(tg)
    mg = MC.case("g60_k5_random")
    ma, mkw = MC.args(mg), dict(vertex_kind=mg["vk"], edge_kind=mg["ek"])
    cg = pg120()
    cp, ca, cb, cz, ci, gamma = pg120_closures()
    ce = (cg["fixed"], cg["edge_from"], cg["edge_to"], cg["meas"], cg["info"])
    jg, jp, sc = jcbb_graph()
    ja = (jp,) + AC.args(jg)[1:]
    jop = np.full(len(sc["kinds"]), sc["pose"], np.int32)
    jkw = dict(vertex_kind=jg["vk"], edge_kind=jg["ek"])
    nV, ref, ret, rmeas, rinfo, remove = RN.case("lattice300")
    D = JC.case("crossed")
    kr = dict(MCFG.DEFAULT, **MCFG.CONFIGS[MATCH_OTHER][0])["kernel_range"]
    e = lambda g: [(g["edge_from"], g["edge_to"])]   # noqa: E731
    return [
        _plain("gn_v5e4", "v5e4", GN_ITERS), _plain("gn_lat40", "lat40", 3), _plain("gn_hub40", "hub40", 3),
        Step("gn_typed_mixed257", lambda ctx: ctx.gn_optimize_typed(*ta, 3, **tkw), ("gn_optimize_typed",), (), e(tg)),
        Step("marginals_all_typed_mixed257", lambda ctx: ctx.marginals_all_typed(tp, *ta[1:], cross=True, **tkw),
             ("marginals_all_typed",), (), e(tg)),
        Step("lm_typed_mixed257", lambda ctx: ctx.lm_optimize_typed(*ta, 3, **tkw), ("lm_optimize_typed",), (), e(tg)),
        Step("gn_mixture_g60", lambda ctx: ctx.gn_optimize_mixture(*ma, mg["iters"], mg["mix"], **mkw), ("gn_optimize_mixture",), (), e(mg)),
        Step("mixture_select_g60", lambda ctx: ctx.mixture_select(*ma, mg["mix"], **mkw), ("mixture_select",), (), e(mg)),
        Step("closure_consistency_pg120", lambda ctx: ctx.closure_consistency(cp, *ce, ca, cb, cz, ci, gamma),
             ("closure_consistency",), (), e(cg)),
        Step("closure_consistency_exact_pg120", lambda ctx: ctx.closure_consistency_exact(cp, *ce, ca, cb, cz, ci, gamma),
             ("closure_consistency_exact",), (), e(cg)),
        Step("joint_compatibility_mixed5", lambda ctx: ctx.joint_compatibility(*ja, jop, sc["kinds"], sc["meas"], sc["info"], sc["lms"], **jkw),
             ("joint_compatibility",), (), e(jg)),
        Step("jcbb_dense_crossed", lambda ctx: ctx.jcbb_dense(D["slot"], D["dim"], D["sigma"], D["e"], D["J"], D["R"], D["gamma"]),
             ("jcbb_dense",), (), []),
        Step("remove_nodes_lattice300", lambda ctx: ctx.remove_nodes(ref, ret, rmeas, rinfo, remove, num_vertices=nV), ("remove_nodes",), (), []),
        Step("scan_information", _scan("information"), ("scan_information",), (), []),
        Step("scan_prune", _scan("prune"), ("scan_prune",), (), []),
        Step("occupancy_multi_block", _occupancy, (), (), []),
        Step("match_default", _match(MCFG.DEFAULT["kernel_range"]), (), (), []),
        Step("match_" + MATCH_OTHER, _match(kr), (), (), []),
        Step("robot_round_pg120", _robot_round, (), (), e(cg)),
    ]


# ---- failing and refused steps
def _fail_gn(where):
    return lambda ctx: ctx.gn_optimize(*fail_args(where), GN_ITERS, raise_on_cholesky=False)


def refused_calls():
    """(label, call(ctx)) of one CGMR_E_INVALID call per family, each refused before any launch."""
    a = pg500_args()
    bad_et = a[3].copy()
    bad_et[7] = len(a[0])                                                  # an edge index out of range
    tg = TC.case("mixed255")                                               # test_typed_gpu: a landmark observation from a point
    vk, ek = TC.kinds(tg)
    k1, pt = int(np.flatnonzero(ek == 1)[0]), int(np.flatnonzero(vk == 1)[0])
    tf = tg["edge_from"].copy()
    tf[k1] = pt
    mg = MC.case("g60_k5_random")
    from test_mixture_gpu import _bad_mixtures
    bad_mix = {label: mix for label, mix, _ in _bad_mixtures(mg)}["weight 0"]
    path3 = np.array([[0, 1, 0], [1, 0, 1], [0, 1, 0]], dtype=bool)
    return [
        ("edge index out of range", lambda ctx: ctx.gn_optimize(*a[:3], bad_et, *a[4:], 1)),
        ("a landmark observation from a point",
         lambda ctx: ctx.gn_optimize_typed(tg["poses"], tg["fixed"], tf, tg["edge_to"], tg["meas"], tg["info"], 2, vertex_kind=vk, edge_kind=ek)),
        ("a mixture component of weight 0",
         lambda ctx: ctx.gn_optimize_mixture(*MC.args(mg), 2, bad_mix, vertex_kind=mg["vk"], edge_kind=mg["ek"])),
        ("max_clique_exact(node_limit=0)", lambda ctx: ctx.max_clique_exact(path3, node_limit=0)),
    ]


def _refused(ctx):
    return tuple(status_or_error(lambda call=call: call(ctx)) for _, call in refused_calls())


def _fail_steps():
    g = pg500()
    e = [(g["edge_from"], g["edge_to"])]
    return [
        Step("fail_leaf", _fail_gn("leaf"), ("gn_optimize",), ("pg500", "fail"), e),
        Step("fail_top", _fail_gn("top"), ("gn_optimize",), ("pg500", "fail"), e),
        Step("fail_lm", lambda ctx: status_or_error(lambda: ctx.lm_optimize(*fail_args("leaf"), GN_ITERS)), ("lm_optimize",), ("pg500", "fail"), e),
        Step("fail_marginals_all", lambda ctx: status_or_error(lambda: ctx.marginals_all(*fail_args("leaf"), cross=True)),
             ("marginals_all",), ("pg500", "fail"), e),
        Step("refused", _refused, ("gn_optimize", "gn_optimize_typed", "gn_optimize_mixture", "max_clique_exact"), ("refused",), []),
    ]


# ---- mode steps: no result of their own
def _mode(method, on):
    def run(ctx):
        getattr(ctx, method)(on)
        return ()
    return run


def _mode_steps():
    return [Step("profiling_on", _mode("set_profiling", True), ("set_profiling",), ("mode",), []),
            Step("profiling_off", _mode("set_profiling", False), ("set_profiling",), ("mode",), []),
            Step("cache_off", _mode("set_symbolic_cache", False), ("set_symbolic_cache",), ("mode",), []),
            Step("cache_on", _mode("set_symbolic_cache", True), ("set_symbolic_cache",), ("mode",), [])]


# ---- the growth unit: two calls, one step
def _growth(ctx):
    g = pg500()
    ef, et, meas, info, ne = growth_lists()
    first = ctx.gn_optimize(g["poses"][:GROW_V], g["fixed"][:GROW_V], ef[:ne], et[:ne], meas[:ne], info[:ne], 2)
    return first, ctx.gn_optimize(g["poses"], g["fixed"], ef, et, meas, info, 2)


def _growth_step():
    ef, et, _, _, ne = growth_lists()
    return Step("growth", _growth, ("gn_optimize",), ("growth",), [(ef[:ne], et[:ne]), (ef, et)])


def steps():
    """The table, built once: name -> Step, in table order."""
    def make():
        table = _pg500_steps() + _other_steps() + _fail_steps() + _mode_steps() + [_growth_step()]
        assert len({s.name for s in table}) == len(table)
        return {s.name: s for s in table}
    return _memo("steps", make)


# Context methods without a step, and why
_DEV = "a _dev twin of a step that has one: the same host path behind another staging of poses / meas / info (test_device_resident_gpu.py)"
_STATS = "reads statistics only"
EXCLUDED = {
    "close": "ends the context",
    "synchronize": "a wait: used by the gn_optimize_dev step, returns nothing",
    "lm_optimize_dev": _DEV, "gn_optimize_robust_dev": _DEV, "lm_optimize_robust_dev": _DEV, "dl_optimize_dev": _DEV,
    "gnc_optimize_dev": _DEV, "chordal_initialize_dev": _DEV, "gn_optimize_typed_dev": _DEV, "lm_optimize_typed_dev": _DEV,
    "dl_optimize_typed_dev": _DEV, "gn_optimize_mixture_dev": _DEV, "lm_optimize_mixture_dev": _DEV, "dl_optimize_mixture_dev": _DEV,
    "lm_optimize_robust": "lm_optimize with gn_optimize_robust's staging: both have a step",
    "dl_optimize_typed": "dl_optimize with gn_optimize_typed's staging: both have a step",
    "lm_optimize_mixture": "lm_optimize with gn_optimize_mixture's staging: both have a step",
    "dl_optimize_mixture": "dl_optimize with gn_optimize_mixture's staging: both have a step",
    "marginals_typed": "marginals with marginals_all_typed's staging: both have a step",
    "marginals_robust": "marginals with condense_robust's staging: both have a step",
    "marginals_all_robust": "marginals_all with condense_robust's staging: both have a step",
    "covariance_estimate_robust": "covariance_estimate with condense_robust's staging: both have a step",
    "observation_covariance": "the single-pair gate of joint_compatibility, which has a step and runs the same frame",
    "closure_consistency_inter": "closure_consistency with peer poses added on the host: the same device frame",
    "closure_consistency_inter_exact": "closure_consistency_exact with peer poses added on the host: the same device frame",
    "max_clique_greedy": "the clique launch of closure_consistency alone; keeps nothing in the context",
    "min_spanning_tree": "the spanning-tree launch of condense_tree alone; keeps nothing in the context",
    "initial_guess": "no device work and no context",
    "lm_last_stats": _STATS, "dl_last_stats": _STATS, "gnc_last_stats": _STATS, "scan_info_last_stats": _STATS,
    "host_threads_info": _STATS, "symbolic_cache_stats": _STATS + " (the GPU test reads it after every step)",
    "gn_timeouts": _STATS + " (the GPU test reads it at the end of every order)", "switches": _STATS, "gn_last_timing": _STATS,
    "gn_kernel_times": _STATS, "pcm_kernel_times": _STATS,
}


# ------------------------------------------------------------------------------------------------------------ orders
# Pairs (A, B) of steps outside the growth unit for which the analysis WOULD extend A's cached ordering to B's graph
# (tests/test_call_order_cpu.py asks it): v5e4's four odometry edges open the edge list of every C2-recipe graph, and the
# 60-vertex mixture graph adds fewer than 64 vertices to it.  B right behind A is a grown graph as far as the library can tell,
# and legitimately another ordering than B's on a fresh context: no order runs B behind A without a call in between that
# replaces or drops the cached structure.
EXTENDABLE = (("gn_v5e4", "gn_mixture_g60"), ("gn_v5e4", "mixture_select_g60"))
SEEDS = (2, 3, 6)          # the first seeds from 1 on whose shuffle has no such pair (extension_hazards; test_call_order_cpu.py)


def extension_hazards(names):
    """(i, k) for every step k of the order whose result legitimately depends on step i: an EXTENDABLE pair with no step in
    between that hands the solver an edge list, refuses one, or switches the cache; the growth unit behind cache_off."""
    table = steps()
    drops = lambda s: bool(s.edges) or "refused" in s.tags or s.name.startswith("cache_")   # noqa: E731
    out = []
    for a, b in EXTENDABLE:
        for i, n in enumerate(names):
            if n != a:
                continue
            for k in range(i + 1, len(names)):
                if names[k] == b:
                    out.append((i, k))
                if names[k] == b or drops(table[names[k]]):
                    break
    # ... and the growth unit extends only while the cache is on: behind cache_off its second call is analysed from scratch
    off = None
    for k, n in enumerate(names):
        if n.startswith("cache_"):
            off = k if n == "cache_off" else None
        elif "growth" in table[n].tags and off is not None:
            out.append((off, k))
    return sorted(out)


def shuffled(seed):
    names = list(steps())
    return [names[i] for i in np.random.default_rng(seed).permutation(len(names))]


FAILING = ("fail_leaf", "fail_top", "fail_lm", "fail_marginals_all")
PANEL_READERS = ("gn_pg500", "gn_pg500_perturbed", "lm_pg500", "dl_pg500", "marginals_all_pg500", "condense_tree_pg500")


def adversarial():
    """The hand-written order: every failing step immediately in front of every pg500 step that reads panels; fail_leaf twice
    in a row; fail_top then fail_leaf; the largest structure, the smallest, the largest; the matcher configurations A, B, A; a
    refused call between a solve and the marginals of the same graph; each mode step in front of a pg500 solve; then every
    step not yet run, in table order."""
    order = ["gn_pg500"]
    for reader in PANEL_READERS:
        for f in FAILING:
            order += [f, reader]
    order += ["fail_leaf", "fail_leaf", "gn_pg500", "fail_top", "fail_leaf", "marginals_all_pg500"]
    order += ["gn_lat40", "gn_v5e4", "gn_lat40", "gn_pg500"]
    order += ["match_default", "match_" + MATCH_OTHER, "match_default"]
    order += ["gn_pg500", "refused", "marginals_pg500"]
    order += ["profiling_on", "gn_pg500", "profiling_off", "lm_pg500", "cache_off", "gn_pg500", "cache_on", "gn_pg500", "dl_pg500"]
    return order + [n for n in steps() if n not in order]


def orders():
    return dict({f"shuffle_{s}": shuffled(s) for s in SEEDS}, adversarial=adversarial())


def run_order(ctx, names, baseline, label):
    """Run the steps ``names`` on ``ctx`` one after the other and hold each to ``baseline`` (name -> flat results), the cache
    counters to the rules of tests/test_call_order_gpu.py.  Returns dict(compared, hits, misses, extended, timeouts)."""
    table = steps()
    s_first = s0 = ctx.symbolic_cache_stats()
    cache_on, in_place, prev, compared = True, False, "(a fresh context)", 0
    for name in names:
        st = table[name]
        where = f"order {label}: step {name} after {prev}"
        try:
            got = flat(st.run(ctx))
        except CgmrError as e:
            raise AssertionError(f"{where}: the call raised {e}") from e
        s1 = ctx.symbolic_cache_stats()
        d = {k: s1[k] - s0[k] for k in s1}
        if ctx.gn_timeouts() != 0:
            raise AssertionError(f"{where}: a bounded device-side wait ran out (gn_timeouts {ctx.gn_timeouts()}): the launch shape "
                                 "of this context has changed, what follows is not comparable")
        diff = first_difference(got, baseline[name])
        assert diff is None, f"{where}: {diff}"
        compared += 1
        assert (d["extended"] == 1) if "growth" in st.tags else (d["extended"] == 0), f"{where}: cache counters moved by {d}"
        if "mode" in st.tags:
            assert d == dict(hits=0, misses=0, extended=0), f"{where}: {d}"
            if st.name.startswith("cache_"):
                cache_on, in_place = st.name == "cache_on", False
        elif "pg500" in st.tags:
            want = dict(hits=1, misses=0, extended=0) if in_place else dict(hits=0, misses=1, extended=0)
            assert d == want, f"{where}: cache counters moved by {d}, expected {want} (structure in place: {in_place})"
            in_place = cache_on
        elif any(d.values()):
            in_place = False
        s0, prev = s1, name
    return dict(compared=compared, timeouts=ctx.gn_timeouts(), **{k: s0[k] - s_first[k] for k in s0})
