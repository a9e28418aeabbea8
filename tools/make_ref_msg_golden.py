#!/usr/bin/env python3
"""Regenerate tests/golden/msg_ref.npz from the reference's own message serialiser.

    make -C oracle _ref/ref_msg REF=<reference checkout>
    python tools/make_ref_msg_golden.py [--binary oracle/_ref/ref_msg] [--out tests/golden/msg_ref.npz]

Every case of tests/ref_msg_cases.py goes through ``ref_msg encode`` (toCharArray with bsize = MAX_LENGTH_MSG), the bytes that
come back through ``ref_msg decode`` (MessageFactory::fromCharArray).  The fixture holds data only: the inputs, the
reference's bytes and decoded fields; for the messages around MAX_LENGTH_MSG the returned length and a SHA-256.
"""
import argparse
import hashlib
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_msg_cases as RC   # noqa: E402


def _run(binary, mode, payload):
    return subprocess.run([binary, mode], input=payload, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout


def encode(binary, records):
    """-> [(length or -1, bytes)] in the order of ``records``"""
    out = _run(binary, "encode", b"".join(RC.pack_record(r) for r in records))
    res, o = [], 0
    for _ in records:
        (n,) = struct.unpack_from("<q", out, o)
        o += 8
        res.append((n, out[o:o + max(n, 0)]))
        o += max(n, 0)
    if o != len(out):
        raise RuntimeError("ref_msg encode: unexpected output length")
    return res


def decode(binary, messages):
    out = _run(binary, "decode", b"".join(struct.pack("<q", len(b)) + b for b in messages))
    res, o = [], 0
    for _ in messages:
        r, o = RC.parse_record(out, o)
        res.append(r)
    if o != len(out):
        raise RuntimeError("ref_msg decode: unexpected output length")
    return res


def generate(binary):
    """The fixture as a dict of arrays."""
    names = RC.case_names()
    recs = [RC.case_record(n) for n in names]
    enc = encode(binary, recs)
    if any(n < 0 for n, _ in enc):
        raise RuntimeError("a small case came back null")
    dec = decode(binary, [b for _, b in enc])
    fx = {"names": np.array(names)}
    for name, r, (_, b), d in zip(names, recs, enc, dec):
        fx[name + "/in"] = np.frombuffer(RC.pack_record(r), dtype=np.uint8)
        fx[name + "/bytes"] = np.frombuffer(b, dtype=np.uint8)
        fx[name + "/dec"] = np.frombuffer(RC.pack_record(d), dtype=np.uint8)
    big = encode(binary, [RC.size_record(row) for row in RC.SIZE_ROWS])
    fx["sizes"] = np.array([[t, a, b, RC.SIZE_SEED + k, n] for k, ((_, t, a, b, _), (n, _)) in enumerate(zip(RC.SIZE_ROWS, big))],
                           dtype=np.int64)
    fx["sizes_sha"] = np.array([hashlib.sha256(b).hexdigest() if n >= 0 else "" for n, b in big])
    return fx


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--binary", default=os.path.join(ROOT, "oracle", "_ref", "ref_msg"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "msg_ref.npz"))
    a = ap.parse_args()
    fx = generate(a.binary)
    np.savez_compressed(a.out, **fx)
    print(f"{a.out}: {len(fx['names'])} cases, {len(fx['sizes'])} size rows, {os.path.getsize(a.out)} bytes")
    for row, (t, x, y, _, n) in zip(RC.SIZE_ROWS, fx["sizes"].tolist()):
        print(f"  {row[0]:>18}: reference returns {'null' if n < 0 else n}")


if __name__ == "__main__":
    main()
