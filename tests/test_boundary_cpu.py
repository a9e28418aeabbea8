"""tests/boundary_cases.py on the CPU, before tests/test_boundary_gpu.py trusts the sweeps on the GPU: the host analysis puts a
case on either side of every tile, chunk, child-count, list-length and key-count constant, in the role the constant applies to
(a case that stops reaching its side fails here); the families have the front tables their descriptions claim; and the C
oracle's Gauss-Newton step on every case meets the bar the GPU's step is held to (a case on which the oracle alone misses it
would be no valid case for that check: it is listed in boundary_cases.NO_STEP_CHECK instead, the bar stays); and that
yardstick resolves a real error on the cases next to the constants (tests/test_topology_cpu.py's mutations)."""
import numpy as np
import pytest

import boundary_cases as B
import ref_numpy as R
import reference_cases as C
import test_reference_cpu as TR
from reference_cases import OMEGA_MAX
from test_topology_cpu import mutation


def _near(role, limit):
    """(below, above): a front in `role` whose border rows 3 ns are the last multiple of 3 up to `limit` / the first beyond."""
    return (lambda s: any(limit - 3 < r <= limit for r in s["role"][role]),
            lambda s: any(limit < r <= limit + 3 for r in s["role"][role]))


def _single_chain(s):
    return s["info"]["fronts"] == s["info"]["levels"]


# label -> (predicate of the near side, predicate of the far side) on boundary_cases.shape()
BOUNDARIES = {
    "leaf chunk, 95 rows": _near("leaf", B.LEAF_CHUNK),
    "mid chunk, 79 rows": _near("mid", B.MID_CHUNK),
    "upper chunk, 31 rows": _near("upper", B.TOP_CHUNK),
    "selected-inversion row tile, 64 rows": _near("any", B.SELINV_TILE),
    "update tile, 32 rows": _near("factor", B.UPDATE_TILE),
    "kChunkRows, 159 rows": _near("factor", B.CHUNK_ROWS),
    "top block, 128 columns": (
        lambda s: _single_chain(s) and B.TOP_MAX_COLS - 3 < 3 * s["info"]["free_poses"] <= B.TOP_MAX_COLS and len(s["top"]) == s["info"]["fronts"],
        lambda s: _single_chain(s) and B.TOP_MAX_COLS < 3 * s["info"]["free_poses"] <= B.TOP_MAX_COLS + 3 and len(s["top"]) < s["info"]["fronts"]),
    "children of a factor-level front, 8": (lambda s: B.WORK_CHILDREN in s["children_factor"], lambda s: B.WORK_CHILDREN + 1 in s["children_factor"]),
    "children fetched up front by the top block, 32": (lambda s: s["children_top"] == B.TOP_PRE, lambda s: s["children_top"] == B.TOP_PRE + 1),
    "children of one front, 64": (lambda s: B.CHILD_ROUND in s["children_any"], lambda s: B.CHILD_ROUND + 1 in s["children_any"]),
    **{f"assembly list, {n} entries": (lambda s, n=n: s["longest_list"] == n, lambda s, n=n: s["longest_list"] == n + 1) for n in B.LIST_EDGES},
}


def test_every_boundary_has_a_case_on_either_side():
    shapes = {name: B.shape(name) for name in B.CASES}
    print()
    for label, sides in BOUNDARIES.items():
        found = [[n for n, s in shapes.items() if side(s)] for side in sides]
        show = [", ".join(f[:6]) + (f" .. ({len(f)})" if len(f) > 6 else "") for f in found]
        print(f"{label:48s} | up to it: {show[0]:70s} | beyond: {show[1]}")
        assert found[0] and found[1], (label, found)
    # the scan's tiles: every residue mod 4 of the key count on either side
    keys = {s["keys"]: n for n, s in shapes.items()}
    for edge in B.SCAN_EDGES:
        below, above = [keys.get(k) for k in range(edge - 3, edge + 1)], [keys.get(k) for k in range(edge + 1, edge + 5)]
        print(f"{'k_asm_scan, ' + str(edge) + ' keys':48s} | up to it: {', '.join(map(str, below)):70s} | beyond: {', '.join(map(str, above))}")
        assert all(below) and all(above), (edge, below, above)


def _fronts(name):
    """[(nc, ns, level, children, in the top block)] in elimination order."""
    s = B.shape(name)
    return [(int(r[1]), int(r[2]), int(r[4]), int(r[5]), f in s["top"]) for f, r in enumerate(s["table"])]


def test_clique_family_is_a_chain_of_full_fronts_under_the_top_block():
    for n in range(2, 72):
        s, fr = B.shape(f"clique_{n}"), _fronts(f"clique_{n}")
        info = s["info"]
        # the chain (16, n - 16), (16, n - 32), .., the remainder last
        assert [(f[0], f[1]) for f in fr] == [(min(16, n - c), n - c - min(16, n - c)) for c in range(0, n, 16)], n
        assert [f[3] for f in fr] == [0] + [1] * (len(fr) - 1)
        if n <= 42:
            assert info["top_block_cols"] == 3 * n and info["launch_levels"] == 0 and all(f[4] for f in fr), n
        else:
            assert info["top_block_cols"] < 3 * n and not fr[0][4] and info["launch_levels"] == (1 if n < 59 else 2), n
    assert _fronts("clique_43")[0][:2] == (16, 27) and _fronts("clique_48")[0][:2] == (16, 32)
    assert B.shape("clique_48")["chunk"] == [B.LEAF_CHUNK] and B.shape("clique_59")["chunk"] == [B.LEAF_CHUNK, B.TOP_CHUNK]


def test_blobs_family_has_four_leaves_with_the_separator_as_their_border():
    for b in range(1, 55):
        fr = _fronts(f"blobs_{b}")
        if b <= 48:
            assert [f[:4] for f in fr[:4]] == [(16, b, 0, 0)] * 4 and not any(f[4] for f in fr[:4]), b
            assert B.shape(f"blobs_{b}")["chunk"][0] == B.LEAF_CHUNK
        assert sum(f[0] for f in fr) == b + 64
    # beyond the sweep of the leaves the analysis chains the fronts: kept as what they are, borders across kChunkRows
    assert max(f[1] for f in _fronts("blobs_54")) > B.CHUNK_ROWS // 3 and B.shape("blobs_54")["info"]["max_children"] == 1


@pytest.mark.parametrize("k", [2, 9])
def test_forest_family_has_no_top_block_and_k_fronts_on_every_level(k):
    for n in range(17, 65):
        s, fr = B.shape(f"forest{k}_{n}"), _fronts(f"forest{k}_{n}")
        assert s["info"]["top_block_fronts"] == 0 and s["info"]["launch_levels"] == s["info"]["levels"], n
        level1 = [f[:2] for f in fr if f[2] == 1]
        assert level1 == [(min(16, n - 16), max(0, n - 32))] * k, n
        assert s["chunk"][1] == (B.TOP_CHUNK if k <= B.TOP_CHUNK_FRONTS else B.MID_CHUNK)


def test_fan_family_sets_the_child_count():
    for m in B.FAN_M:
        s, fr = B.shape(f"fan_{m}"), _fronts(f"fan_{m}")
        assert fr[-1][3] == m and fr[-1][4] and s["children_top"] == m and s["info"]["max_children"] == m, m
    for m in B.FAN2_M:
        s = B.shape(f"fan2_{m}")
        if m >= 8:                  # (the two roots amalgamated: one front of the top block with 2 m children)
            assert s["info"]["max_children"] == 2 * m == s["children_top"], m
        else:                       # (two roots, no top block: factor-level fronts with m children)
            assert s["top"] == set() and m in s["children_factor"], m
    for m in B.FANLOW_M:            # the separator's lowest front, below the top block, has the m blobs as children
        s, fr = B.shape(f"fanlow_{m}"), _fronts(f"fanlow_{m}")
        assert [f[3] for f in fr if not f[4]].count(m) == 1 and s["info"]["max_children"] == m, m


def test_star_dup_and_chain_families_set_list_lengths_and_key_counts():
    for k in B.STAR_K:
        assert B.shape(f"star_{k}")["longest_list"] == k
    for d in B.DUP_D:
        s = B.shape(f"dup_{d}")
        assert s["longest_list"] == d and s["keys"] == 3
    for V in B.CHAIN_V:
        assert B.shape(f"chain_{V}")["keys"] == 2 * V - 1 and B.shape(f"ring_{V}")["keys"] == 2 * V


@pytest.mark.parametrize("family", list(B.FAMILIES))
def test_oracle_step_meets_the_bar_on_every_case(oracle, family):
    """The yardstick of tests/test_boundary_gpu.py on the C oracle's own step from the initial guess."""
    worst, over = 0.0, []
    for name in B.FAMILIES[family]:
        g = B.graph(name)
        a = C.args(g)
        st, p1, _, _ = oracle.gn_optimize(*a, 1)
        assert st == 0, name
        w = R.step_backward_error(g["poses"], p1, *a[1:])
        worst = max(worst, w)
        if w > OMEGA_MAX:
            over.append(name)
        fx = g["fixed"] != 0
        assert np.array_equal(p1[fx], g["poses"][fx])
    print(f"{family}: largest omega of the oracle's step {worst / R.U:.1f} u; above the bar: {over}")
    assert sorted(over) == sorted(n for n in B.NO_STEP_CHECK if B.FAMILY_OF[n] == family)


# the cases next to the chunk, tile and top-block constants, and one of every other family
RESOLVED = (*B.TRACE_CASES, "forest2_43", "forest9_59", "fanlow_9", "fan_33", "fan2_33", "star_257", "dup_17", "ring_2048")


@pytest.mark.parametrize("name", RESOLVED)
def test_omega_resolves_a_real_error(name):
    """One edge left out of the assembly (or, on a tree, one block of H off by 1e-9) shows above the bar; the unperturbed
    SuperLU step stays below it."""
    g = B.graph(name)
    a = C.args(g)
    p0, p1 = TR._perturbed_step(g)
    assert R.step_backward_error(p0, p1, *a[1:]) <= OMEGA_MAX
    kind, arg = mutation(g)
    q0, q1 = TR._perturbed_step(g, **{kind: arg})
    w = R.step_backward_error(q0, q1, *a[1:])
    print(f"{name}: {kind} {arg}: omega {w / R.U:.3g} u")
    assert w > OMEGA_MAX, (name, kind, w / R.U)
