"""The all-pose marginals entry point (cgmr_marginals_all) as the header, the library and the Python layers declare it; no GPU
needed.  tests/test_marginals_all_gpu.py checks what it computes."""
import os
import re

from cg_mrslam_amd import _lib
from cg_mrslam_amd.graph import GraphSLAM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _prototype(name):
    txt = open(os.path.join(ROOT, "include", "cgmr.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/cgmr.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_marginals_all_with_eleven_parameters():
    args = _prototype("cgmr_marginals_all")
    assert len(args) == 11, args
    assert args[0].startswith("cgmr_ctx*") and args[3].startswith("const uint8_t*")
    assert args[-2].startswith("double*") and args[-1].startswith("double*")


def test_library_exports_marginals_all_and_reports_version_103():
    lib = _lib.load_library()
    assert hasattr(lib, "cgmr_marginals_all")
    assert lib.cgmr_version() >= 103


def test_python_layers_expose_marginals_all():
    assert callable(getattr(_lib.Context, "marginals_all", None))
    assert callable(getattr(GraphSLAM, "computeMarginals", None))
