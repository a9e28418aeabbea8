"""Return codes and error texts of the solver's entry points for bad input, against a record made from the library as it was
before the host layer was split (tests/golden/error_texts.json; tools/make_error_texts_golden.py made it).  Callers and tests
rely on the texts' quirks -- a typed _dev Gauss-Newton call reports robust errors as cgmr_gn_optimize_typed, mixture checks
as ..._mixture, the plain marginals family as ..._robust -- so they are held byte for byte.  The cases: error_text_cases.py.
"""
import json
import os

import pytest

import error_text_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "error_texts.json")


@pytest.fixture(scope="module")
def answers():
    from cg_mrslam_amd import Context
    ctx = Context(0)
    got = cases.run_all(ctx.lib, ctx.h)
    ctx.close()
    return got


@pytest.fixture(scope="module")
def record():
    with open(GOLDEN) as f:
        return json.load(f)


def test_record_covers_every_case(record):
    assert sorted(record["cases"]) == sorted(cases.case_ids())
    assert all(rc < 0 and text for rc, text in record["cases"].values())      # every bad input was refused, with a text


def test_every_family_and_input_is_there():
    ids = cases.case_ids()
    for family in ("gn_optimize", "lm_optimize", "dl_optimize", "gnc_optimize", "chordal_initialize", "cgmr_marginals:", "marginals_all",
                   "covariance_estimate", "condense", "marginals_joint", "marginals_pairs", "relative_covariance",
                   "observation_covariance", "closure_consistency"):
        assert any(family in i for i in ids), family
    for bad in cases.BAD_INPUTS:
        assert any(i.endswith(":" + bad) for i in ids), bad


@pytest.mark.parametrize("bad", cases.BAD_INPUTS)
def test_codes_and_texts_match_the_record(answers, record, bad):
    ids = [i for i in cases.case_ids() if i.endswith(":" + bad)]
    assert ids
    wrong = {i: (answers[i], record["cases"][i]) for i in ids if answers[i] != record["cases"][i]}
    assert not wrong, wrong
