"""Record tests/golden/error_texts.json: the (return code, cgmr_last_error text) of every bad call of
tests/error_text_cases.py, from a build of the commit BEFORE the solver's host layer was split into one file per concern.

    CGMR_LIB=/abs/path/to/parent/libcgmr.so python tools/make_error_texts_golden.py [--out tests/golden/error_texts.json]

The record is what the split is held to, so it is never made from the library under test: CGMR_LIB must name another build, and
the in-tree one is refused.  Needs an MI355X (a context is created; every call is refused on the host before any launch).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "error_texts.json"))
    args = ap.parse_args()
    lib_path = os.environ.get("CGMR_LIB")
    in_tree = os.path.join(ROOT, "cg_mrslam_amd", "libcgmr.so")
    if not lib_path or os.path.realpath(lib_path) == os.path.realpath(in_tree):
        sys.exit("CGMR_LIB must name a libcgmr.so built from the parent commit, not the in-tree build")
    import error_text_cases as cases
    from cg_mrslam_amd import Context
    ctx = Context(0)
    got = cases.run_all(ctx.lib, ctx.h)
    version = int(ctx.lib.cgmr_version())
    ctx.close()
    accepted = [i for i, (rc, _t) in got.items() if rc >= 0]
    if accepted:
        sys.exit(f"not refused: {accepted}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"library_version": version, "cases": got}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(got)} cases -> {args.out}")


if __name__ == "__main__":
    main()
