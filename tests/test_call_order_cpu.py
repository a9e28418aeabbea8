"""The preconditions of the call-order table (tests/call_order_cases.py), without a GPU: the table is complete, the steps said
to share a structure share it, the failing inputs fail where the table says and for the reason it says, and no pair of steps
outside the growth unit is a grown graph that the analysis would extend."""
import inspect

import numpy as np
import scipy.linalg as sla

import call_order_cases as K
import ref_numpy as R
from cg_mrslam_amd._lib import Context, gn_symbolic_info_grown


def _public_methods():
    return sorted(n for n, f in vars(Context).items() if not n.startswith("_") and inspect.isfunction(f))


def test_every_context_method_has_a_step_or_a_reason():
    used = {m for s in K.steps().values() for m in s.uses}
    public = set(_public_methods())
    assert used <= public, sorted(used - public)
    assert set(K.EXCLUDED) <= public, sorted(set(K.EXCLUDED) - public)
    assert not used & set(K.EXCLUDED), sorted(used & set(K.EXCLUDED))
    missing = sorted(public - used - set(K.EXCLUDED))
    assert not missing, f"Context methods without a step in call_order_cases.steps() and without a reason in EXCLUDED: {missing}"
    assert all(isinstance(why, str) and why for why in K.EXCLUDED.values())


def test_every_step_of_an_order_is_in_the_table_and_every_order_runs_the_whole_table():
    table = K.steps()
    for label, names in K.orders().items():
        assert set(names) == set(table), (label, sorted(set(table) ^ set(names)))
    assert len({tuple(o) for o in K.orders().values()}) == 4
    adv = K.adversarial()
    at = lambda n: [i for i, x in enumerate(adv) if x == n]   # noqa: E731
    for reader in K.PANEL_READERS:
        assert "panels" in table[reader].tags
        for f in K.FAILING:
            assert any(adv[i + 1] == reader for i in at(f)), (f, reader)
    assert sorted(n for n, s in table.items() if "panels" in s.tags) == sorted(K.PANEL_READERS)
    assert any(adv[i + 1] == "fail_leaf" for i in at("fail_leaf")) and any(adv[i + 1] == "fail_leaf" for i in at("fail_top"))
    assert any(adv[i:i + 3] == ["gn_lat40", "gn_v5e4", "gn_lat40"] for i in range(len(adv)))
    assert any(adv[i:i + 3] == ["match_default", "match_" + K.MATCH_OTHER, "match_default"] for i in range(len(adv)))
    assert any(adv[i:i + 3] == ["gn_pg500", "refused", "marginals_pg500"] for i in range(len(adv)))
    for mode in ("profiling_on", "profiling_off", "cache_off", "cache_on"):
        assert "pg500" in table[adv[at(mode)[0] + 1]].tags, mode


def test_the_pg500_steps_share_one_edge_list():
    g = K.pg500()
    shared = [s for s in K.steps().values() if "pg500" in s.tags]
    assert len(shared) == 17 + 4                                   # the seventeen calls of the table and the four failing ones
    for s in shared:
        assert len(s.edges) == 1, s.name
        assert np.array_equal(s.edges[0][0], g["edge_from"]) and np.array_equal(s.edges[0][1], g["edge_to"]), s.name
    for s in K.steps().values():                                  # and nobody else does
        if "pg500" not in s.tags:
            assert not any(len(ef) == len(g["edge_from"]) and np.array_equal(ef, g["edge_from"]) and np.array_equal(et, g["edge_to"])
                           for ef, et in s.edges), s.name


def _is_proper_prefix(a, b):
    return len(a[0]) < len(b[0]) and np.array_equal(a[0], b[0][:len(a[0])]) and np.array_equal(a[1], b[1][:len(a[0])])


def _vertices(e):
    return int(max(e[0].max(), e[1].max())) + 1


def _would_extend(a, b):
    """The host analysis' own answer: with ``a`` cached, is the ordering of ``b`` extended from it?"""
    return gn_symbolic_info_grown(_vertices(a), len(a[0]), [_vertices(b)], [len(b[0])], b[0], b[1])[2] == 1


def test_no_step_grows_another_steps_graph_outside_the_growth_unit():
    """prepare_structure (gn_host.cpp) extends the cached ordering only where the cached edge list is a proper prefix of the
    new one.  The chain of v5e4 (four odometry edges) IS such a prefix of every C2-recipe graph here, pg500 included -- the
    table must hold both -- so the guard asks the analysis itself, for every prefix pair, whether it would extend.  It declines
    once the new vertices outnumber max(64, a quarter of the old ones), which leaves the 60-vertex mixture graph behind v5e4:
    call_order_cases.EXTENDABLE names that pair, and no order may run it back to back.  The growth unit's own pair must extend."""
    table = K.steps()
    lists = [(s.name, e) for s in table.values() if "growth" not in s.tags for e in s.edges]
    prefix = sorted({(na, nb) for na, a in lists for nb, b in lists if _is_proper_prefix(a, b)})
    assert {na for na, _ in prefix} == {"gn_v5e4"}, prefix
    extend = sorted({(na, nb) for na, a in lists for nb, b in lists if _is_proper_prefix(a, b) and _would_extend(a, b)})
    print(f"{len(prefix)} proper prefixes among the steps' edge lists, all of gn_v5e4's; the analysis would extend {extend}")
    assert extend == sorted(K.EXTENDABLE)
    for label, names in K.orders().items():
        assert K.extension_hazards(names) == [], (label, K.extension_hazards(names))
    assert K.extension_hazards(["gn_v5e4", "match_default", "gn_mixture_g60"]) == [(0, 2)]          # (the check itself)
    assert K.extension_hazards(["gn_v5e4", "gn_pg500", "gn_mixture_g60"]) == []
    assert K.extension_hazards(["cache_off", "gn_pg500", "growth"]) == [(0, 2)]
    assert K.extension_hazards(["cache_off", "cache_on", "growth"]) == []
    first, second = table["growth"].edges
    assert _is_proper_prefix(first, second) and _would_extend(first, second)
    for name, e in lists:                                          # nor does the growth unit extend what another step left
        for target in (first, second):
            if _is_proper_prefix(e, target):
                assert not _would_extend(e, target), name
        for source in (first, second):
            if _is_proper_prefix(source, e):
                assert not _would_extend(source, e), name


def test_pg500_has_panels_tree_levels_and_a_top_block():
    info, t, perm, top = K.pg500_shape()
    assert info["panel_doubles"] > 0 and info["launch_levels"] >= 3 and info["top_block_fronts"] >= 1
    assert len(top) == info["top_block_fronts"] and len(t) - 1 in top


def test_the_failing_vertices_lie_where_the_table_says():
    info, t, perm, top = K.pg500_shape()
    leaf, root = K.fail_vertex("leaf"), K.fail_vertex("top")
    f = K.front_of(leaf)
    assert f == 0 and t[f, 4] == 0 and t[f, 5] == 0 and f not in top, (leaf, f, t[f].tolist())
    assert K.front_of(root) in top and K.front_of(root) == len(t) - 1, (root, K.front_of(root))
    assert K.pg500()["fixed"][leaf] == 0 and K.pg500()["fixed"][root] == 0
    print(f"fail_leaf: vertex {leaf} (front 0 of {len(t)}, level 0); fail_top: vertex {root} (the root front, top block of {len(top)})")


def test_the_zero_block_is_the_only_cause_of_failure():
    for where in ("leaf", "top"):
        v = K.fail_vertex(where)
        poses, fixed, ef, et, meas, info = K.fail_args(where)
        H, _, hidx = R.build_system(poses, fixed, ef, et, meas, info)
        H = H.toarray()
        k = 3 * int(hidx[v])
        assert np.all(H[k:k + 3, k:k + 3] == 0.0), where           # so no factor exists: the reference fails in iteration 0 too
        try:
            sla.cholesky(H, lower=True)
        except sla.LinAlgError:
            pass
        else:
            raise AssertionError(f"{where}: the float64 system has a Cholesky factor")
        keep = np.ones(len(H), dtype=bool)
        keep[k:k + 3] = False
        sla.cholesky(H[np.ix_(keep, keep)], lower=True)           # (raises if the rest is not positive definite)
        # the other entries of the inputs are pg500's own
        g = K.pg500()
        touched = (ef == v) | (et == v)
        assert touched.any() and np.array_equal(info[~touched], g["info"][~touched]) and np.array_equal(meas, g["meas"])
