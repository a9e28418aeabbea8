"""A context's calls do not depend on the calls before them: every step of tests/call_order_cases.py on a fresh context (the
baseline), then the whole table in four orders on ONE long-lived context, every result compared with the baseline in bytes.
The narrow case the table is built around -- a pass that fails below the top block of a cached structure, then a good pass on
that structure, which skips the memset of the panels -- is a test of its own at the end.

No number here is a tolerance: every comparison is dtype, shape and bytes."""
import numpy as np
import pytest

import call_order_cases as K
from cg_mrslam_amd import Context
from cg_mrslam_amd._lib import CGMR_E_CHOLESKY_BASE
from switch_contexts import context_under

pytestmark = pytest.mark.gpu

# steps that two fresh contexts do not run to the same bytes, by a documented cause: name -> (the cause, the bar of the step's
# own test file, the difference measured).  At most two may stand here; none does: on an MI355X every step of the table gave
# the same bytes on two fresh contexts.  (A step entered here also needs that bar in call_order_cases.run_order.)
NOT_BITWISE = {}


def _fresh(step):
    c = Context(0)
    try:
        return K.flat(step.run(c)), c.gn_timeouts()
    finally:
        c.close()


@pytest.fixture(scope="module")
def baseline():
    """name -> the flat results of the step on a fresh Context(0) of its own: created, used once, closed."""
    out = {}
    for name, step in K.steps().items():
        out[name], timeouts = _fresh(step)
        assert timeouts == 0, name
    return out


def test_baseline_failing_and_refused_steps_are_what_the_table_says(baseline):
    for where in ("leaf", "top"):
        given = K.fail_args(where)[0]
        (_, rc), (_, poses), (_, chi) = baseline["fail_" + where]
        assert int(rc) == CGMR_E_CHOLESKY_BASE, (where, int(rc))                       # iteration 0
        assert poses.dtype == np.float64 and poses.tobytes() == np.ascontiguousarray(given, dtype=np.float64).tobytes(), where
    for name in ("fail_lm", "fail_marginals_all"):
        print(name, "on a fresh context:", [(k, v.tolist()) for k, v in baseline[name] if v.size <= 1])
    got = dict(baseline["refused"])
    for i, (label, _) in enumerate(K.refused_calls()):
        assert str(got[f"out[{i}][0]"]) == "error" and int(got[f"out[{i}][1]"]) == -1, (label, got[f"out[{i}][0]"], got[f"out[{i}][1]"])
    for name, step in K.steps().items():
        if "mode" in step.tags:
            assert baseline[name] == []
        elif "fail" not in step.tags and "refused" not in step.tags:
            assert baseline[name], name
    for name in ("gn_pg500", "gn_pg500_perturbed", "gn_v5e4", "gn_lat40", "gn_hub40"):
        assert int(baseline[name][0][1]) == 0, name
    assert baseline["gn_pg500"][1][1].tobytes() != baseline["gn_pg500_perturbed"][1][1].tobytes()


def test_fresh_against_fresh(baseline):
    """The determinism the headers promise, and what makes the orders below meaningful."""
    differ = {}
    for name, step in K.steps().items():
        again, _ = _fresh(step)
        diff = K.first_difference(again, baseline[name])
        if diff is not None:
            differ[name] = diff
    assert set(differ) <= set(NOT_BITWISE) and len(NOT_BITWISE) <= 2, differ


@pytest.mark.parametrize("label", list(K.orders()))
def test_every_step_equals_its_baseline_in_any_order(baseline, label):
    names = K.orders()[label]
    assert K.extension_hazards(names) == []
    c = Context(0)
    try:
        got = K.run_order(c, names, baseline, label)
    finally:
        c.close()
    print(f"order {label}: {got['compared']} steps compared; hits +{got['hits']}, misses +{got['misses']}, extended +{got['extended']}; "
          f"gn_timeouts {got['timeouts']}")
    assert got["compared"] == len(names) and got["timeouts"] == 0
    assert got["extended"] == names.count("growth")


def _failing_pass_alone(c, baseline):
    a, p = K.pg500_args(), K.pg500_optimised()
    for where in ("leaf", "top"):
        first = K.flat(c.gn_optimize(*a, K.GN_ITERS))
        assert K.first_difference(first, baseline["gn_pg500"]) is None, (where, K.first_difference(first, baseline["gn_pg500"]))
        s0 = c.symbolic_cache_stats()
        failed = K.flat(c.gn_optimize(*K.fail_args(where), K.GN_ITERS, raise_on_cholesky=False))
        assert K.first_difference(failed, baseline["fail_" + where]) is None, (where, K.first_difference(failed, baseline["fail_" + where]))
        again = K.flat(c.gn_optimize(*a, K.GN_ITERS))                                   # poses, chi2, rc
        assert K.first_difference(again, first) is None, (where, K.first_difference(again, first))
        marg = K.flat(c.marginals_all(p, *a[1:], cross=True))
        assert K.first_difference(marg, baseline["marginals_all_pg500"]) is None, (where, K.first_difference(marg, baseline["marginals_all_pg500"]))
        s1 = c.symbolic_cache_stats()
        assert (s1["hits"] - s0["hits"], s1["misses"] - s0["misses"], s1["extended"] - s0["extended"]) == (3, 0, 0)   # the cached structure throughout
    assert c.gn_timeouts() == 0


@pytest.mark.parametrize("clear_in_top", [None, "1", "0"])
def test_a_good_pass_behind_a_pass_that_failed_in_the_tree(baseline, clear_in_top):
    """gn_optimize on pg500, the same with a zero pivot in a leaf front (in the root front), gn_optimize again, marginals_all:
    the good calls equal the fresh context's in bytes, with the panels cleared by the top-block launch (the default: the pass
    behind the failed one skips its memset) and with a memset per pass."""
    if clear_in_top is None:
        c = Context(0)
        try:
            assert c.switches()["CGMR_CLEAR_IN_TOP"] == 1
            _failing_pass_alone(c, baseline)
        finally:
            c.close()
    else:
        with context_under({"CGMR_CLEAR_IN_TOP": clear_in_top}) as c:
            _failing_pass_alone(c, baseline)
