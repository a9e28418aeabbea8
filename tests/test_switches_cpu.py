"""The library's environment switches (csrc/switches.h): one table, one reader, and documents that say what the table says.
No device."""
import glob
import os
import re

from cg_mrslam_amd import _lib, switch_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cg_mrslam_amd", "csrc")
PYTHON_SIDE = {"CGMR_LIB", "CGMR_RCCL_INIT_TIMEOUT"}        # read by the binding, listed beside the table


def test_every_switch_is_listed_once_with_a_scope():
    rows = switch_table()
    names = [r["name"] for r in rows]
    assert len(names) == len(set(names)) and len(names) >= 40
    for r in rows:
        assert re.fullmatch(r"CGMR_[A-Z0-9_]+", r["name"]) and r["scope"] in ("context", "call", "process") and r["effect"], r


def test_defaults_name_the_constants_of_the_analysis():
    d = {r["name"]: r["value"] for r in switch_table()}
    src = open(os.path.join(CSRC, "gn_symbolic.h")).read()
    for name, const in (("CGMR_CHUNK", "kMidChunkRows"), ("CGMR_LEAF_CHUNK", "kLeafChunkRows"), ("CGMR_TOP_CHUNK", "kTopChunkRows"),
                        ("CGMR_TOP_CHUNK_FRONTS", "kTopChunkFronts")):
        assert d[name] == int(re.search(r"constexpr int %s = (\d+);" % const, src).group(1)), name
    assert d["CGMR_BWD_SPIN_LIMIT"] == 1 << 22 and d["CGMR_MATCH_SPLIT"] == 16 and d["CGMR_HOST_SPIN_US"] == 200
    assert d["CGMR_HOST_MOVE"] == 0 and d["CGMR_RCCL_LIB"] == ""


def test_readme_lists_exactly_the_table():
    txt = open(os.path.join(ROOT, "tools", "README.md")).read()
    m = re.search(r"^## Environment switches$(.*?)(?=^## |\Z)", txt, re.S | re.M)
    assert m, "tools/README.md has no '## Environment switches' section"
    assert set(re.findall(r"CGMR_[A-Z_]+", m.group(1))) == {r["name"] for r in switch_table()} | PYTHON_SIDE


def test_the_environment_is_read_in_one_place():
    """A text search of the library's own sources for its own variable names: only switches.h calls getenv for a CGMR_* variable;
    elsewhere getenv reads the launcher's neutral variables."""
    neutral = {"LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE"}
    files = [f for ext in ("cpp", "hip", "h") for f in glob.glob(os.path.join(CSRC, "*." + ext))]
    assert len(files) > 20
    for f in files:
        src = open(f).read()
        if os.path.basename(f) == "switches.h":
            assert src.count("getenv(") == 1
            continue
        assert 'getenv("CGMR_' not in src, f
        assert set(re.findall(r'getenv\(([^)]*)\)', src)) <= {'"%s"' % n for n in neutral}, f


def test_the_listing_call_is_declared_and_sized():
    assert "cgmr_switches" in _lib.declared_symbols() and "cgmr_switches" in _lib._SYMBOLS
    lib = _lib.load_library()
    need = lib.cgmr_switches(None, None, 0)
    import ctypes
    short = ctypes.create_string_buffer(b"x" * 64, 64)
    assert lib.cgmr_switches(None, short, 64) == need and len(short.value) == 63      # truncated, terminated
    assert lib.cgmr_switches(None, None, 8) < 0
