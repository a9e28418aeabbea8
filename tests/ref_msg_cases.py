"""Cases and record format behind tests/golden/msg_ref.npz: what the reference's own message serialiser
(src/mrslam/msg_factory.cpp, compiled as oracle/_ref/ref_msg) wrote and read back.

The fixture is made by tools/make_ref_msg_golden.py and holds data only:

    names               the cases below, in order
    <name>/in           the record given to ``ref_msg encode`` (format: ``pack_record`` / oracle/ref_msg_main.cpp)
    <name>/bytes        what ``toCharArray(buf, MAX_LENGTH_MSG)`` wrote
    <name>/dec          the record ``ref_msg decode`` made of those bytes (MessageFactory::fromCharArray)
    sizes, sizes_sha    the messages around MAX_LENGTH_MSG: {type, counts, seed, returned length (-1: null)} and the SHA-256
                        of the bytes; their inputs are ``size_record(row)``

Every input is a pure function of the numbers in this file, so the fixture can be regenerated and compared.
"""
import struct

import numpy as np

TYPE_VERTEX_ARRAY, TYPE_COMBO, TYPE_EDGE_ARRAY, TYPE_CLOSURES, TYPE_CONDENSED_GRAPH = 1, 4, 5, 6, 7
TYPE_NAME = {TYPE_VERTEX_ARRAY: "vertex", TYPE_COMBO: "combo", TYPE_EDGE_ARRAY: "edge", TYPE_CLOSURES: "closures",
             TYPE_CONDENSED_GRAPH: "condensed"}
SIZES_N = (0, 1, 3, 130)

_T = 2.0 ** -24                                   # half a float32 ulp at 1.0
FLT_MAX = float(np.finfo(np.float32).max)
#: doubles whose narrowing to float32 is where a conversion can go wrong; their float32 images as the reference's
#: ``_toCharArray<double>`` writes them are in the fixture, a few are spelled out in HARD_IMAGES below
HARD = np.array([
    0.1, 0.0, -0.0,
    1 + _T, 1 + 3 * _T, -(1 + _T), -(1 + 3 * _T),                       # exact ties: to even, downwards and upwards
    np.nextafter(1 + _T, 2.0), np.nextafter(1 + _T, 0.0),               # one double ulp above / below a tie
    np.nextafter(1 + 3 * _T, 2.0), np.nextafter(1 + 3 * _T, 0.0),
    1e-40, -1e-40, 2.0 ** -149, 2.0 ** -150, 2.0 ** -150 + 2.0 ** -190, 1e-46,     # float32 image subnormal (or zero)
    FLT_MAX, -FLT_MAX, FLT_MAX + 2.0 ** 102, FLT_MAX + 2.0 ** 103, 3.5e38, -3.5e38, np.inf, -np.inf,
], dtype=np.float64)
#: a few of them with the float32 pattern the reference's own code gives (also what numpy's astype gives)
HARD_IMAGES = {1e-40: 0x000116c2, 2.0 ** -150: 0x00000000, 2.0 ** -150 + 2.0 ** -190: 0x00000001, 1 + _T: 0x3f800000,
               1 + _T + 2.0 ** -52: 0x3f800001, FLT_MAX + 2.0 ** 102: 0x7f7fffff, FLT_MAX + 2.0 ** 103: 0x7f800000}

#: the messages around MAX_LENGTH_MSG = 100000 (lengths only): type, (edges, closures) or (vertices, readings), and whether
#: the reference writes past its own ``char bufferc[MAX_LENGTH_MSG]`` there (graph_comm.cpp:112) -- the rows this package
#: deliberately answers with None
SIZE_ROWS = [
    ("cond_2270_0", TYPE_CONDENSED_GRAPH, 2270, 0, False),
    ("cond_2272_0", TYPE_CONDENSED_GRAPH, 2272, 0, False),
    ("cond_2272_10", TYPE_CONDENSED_GRAPH, 2272, 10, True),
    ("cond_2273_0", TYPE_CONDENSED_GRAPH, 2273, 0, False),
    ("cond_2272_24998", TYPE_CONDENSED_GRAPH, 2272, 24998, True),
    ("cond_2272_24999", TYPE_CONDENSED_GRAPH, 2272, 24999, False),
    ("cond_0_24998", TYPE_CONDENSED_GRAPH, 0, 24998, True),
    ("combo_6249_24000", TYPE_COMBO, 6249, 24000, True),
    ("combo_6250_24000", TYPE_COMBO, 6250, 24000, False),
]
SIZE_SEED = 7100


def _numbers(rng, shape, offset):
    """Seeded ordinary values of mixed magnitude with every HARD value put somewhere (all of them where the array has room,
    a run of them starting at ``offset`` where it has not)."""
    a = rng.normal(size=shape) * 10.0 ** rng.integers(-3, 4, size=shape)
    flat = a.reshape(-1)
    if flat.size >= len(HARD):
        flat[rng.choice(flat.size, len(HARD), replace=False)] = HARD
    else:
        flat[:] = HARD[(offset + np.arange(flat.size)) % len(HARD)]
    return a


def make_record(mtype, robot, seed, nv=0, nr=0, ne=0, nc=0):
    """One message's fields.  Edges leave one vertex (a condensed star: the gauge) for distinct vertices of the sender."""
    rng = np.random.default_rng(seed)
    base = robot * 10000 + mtype * 500
    rec = dict(type=int(mtype), robot=int(robot))
    rec["vid"] = (base + rng.permutation(nv)).astype(np.int32)
    rec["vest"] = _numbers(rng, (nv, 3), 0)
    rec["node_id"] = int(base + nv)
    rec["readings"] = np.abs(_numbers(rng, (nr,), 9)) if mtype == TYPE_COMBO else np.zeros(0)
    rec["laser"] = np.array([-2.35619449, 0.00436332313, 30.0, 0.1]) if mtype == TYPE_COMBO else np.zeros(4)
    ft = np.empty((ne, 2), dtype=np.int32)
    ft[:, 0] = base + 400 + ne % 50
    ft[:, 1] = base + rng.permutation(ne)
    rec["from_to"] = ft
    rec["edge_numbers"] = np.concatenate([_numbers(rng, (ne, 3), 3), _numbers(rng, (ne, 6), 12)], axis=1)
    rec["closures"] = (10000 + 3 * np.sort(rng.choice(4 * nc + 4, nc, replace=False))).astype(np.int32)   # a std::set: ascending
    return rec


def _counts(mtype, n, m=None):
    m = n if m is None else m
    return {TYPE_VERTEX_ARRAY: dict(nv=n), TYPE_COMBO: dict(nv=n, nr=m), TYPE_EDGE_ARRAY: dict(ne=n), TYPE_CLOSURES: dict(nc=n),
            TYPE_CONDENSED_GRAPH: dict(ne=n, nc=m)}[mtype]


def case_names():
    return [f"{TYPE_NAME[t]}{n}" for t in TYPE_NAME for n in SIZES_N]


def case_record(name):
    """The sender alternates so that a receiver (robot 1 in the GPU tests) has two peers with full and short messages:
    condensed130 and condensed0 come from robot 0, every other case from robot 2."""
    for t, tn in TYPE_NAME.items():
        for k, n in enumerate(SIZES_N):
            if name == f"{tn}{n}":
                robot = 0 if (t == TYPE_CONDENSED_GRAPH and n in (0, 130)) else 2
                return make_record(t, robot, 1000 * t + n, **_counts(t, n))
    raise KeyError(name)


def size_record(row):
    name, t, a, b, _ = row
    return make_record(t, 3, SIZE_SEED + SIZE_ROWS.index(row), **_counts(t, a, b))


# ------------------------------------------------------------------------------------------------ records
def pack_record(r) -> bytes:
    vid, vest = np.ascontiguousarray(r["vid"], dtype="<i4"), np.ascontiguousarray(r["vest"], dtype="<f8")
    rd, la = np.ascontiguousarray(r["readings"], dtype="<f8"), np.ascontiguousarray(r["laser"], dtype="<f8")
    ft, en = np.ascontiguousarray(r["from_to"], dtype="<i4"), np.ascontiguousarray(r["edge_numbers"], dtype="<f8")
    cl = np.ascontiguousarray(r["closures"], dtype="<i4")
    return b"".join([struct.pack("<iiq", r["type"], r["robot"], len(vid)), vid.tobytes(), vest.tobytes(),
                     struct.pack("<iq", r["node_id"], len(rd)), rd.tobytes(), la.tobytes(),
                     struct.pack("<q", len(ft)), ft.tobytes(), en.tobytes(), struct.pack("<q", len(cl)), cl.tobytes()])


def parse_record(buf, o=0):
    """-> (record, offset behind it)"""
    buf = bytes(buf)

    def arr(dtype, count, shape):
        nonlocal o
        a = np.frombuffer(buf, dtype=dtype, count=count, offset=o).reshape(shape).copy()
        o += a.nbytes
        return a
    r = {}
    r["type"], r["robot"], nv = struct.unpack_from("<iiq", buf, o); o += 16
    r["vid"], r["vest"] = arr("<i4", nv, (nv,)), arr("<f8", 3 * nv, (nv, 3))
    r["node_id"], nr = struct.unpack_from("<iq", buf, o); o += 12
    r["readings"], r["laser"] = arr("<f8", nr, (nr,)), arr("<f8", 4, (4,))
    (ne,) = struct.unpack_from("<q", buf, o); o += 8
    r["from_to"], r["edge_numbers"] = arr("<i4", 2 * ne, (ne, 2)), arr("<f8", 9 * ne, (ne, 9))
    (nc,) = struct.unpack_from("<q", buf, o); o += 8
    r["closures"] = arr("<i4", nc, (nc,))
    return r, o


def records_equal_bitwise(a, b):
    """Floats compared as integer views: -0.0 is not 0.0, and there is no NaN to excuse."""
    if (a["type"], a["robot"], a["node_id"]) != (b["type"], b["robot"], b["node_id"]):
        return False
    for k in ("vid", "from_to", "closures"):
        if not np.array_equal(a[k], b[k]):
            return False
    for k in ("vest", "readings", "laser", "edge_numbers"):
        x, y = np.ascontiguousarray(a[k], dtype=np.float64), np.ascontiguousarray(b[k], dtype=np.float64)
        if x.shape != y.shape or not np.array_equal(x.view(np.int64), y.view(np.int64)):
            return False
    return True


# ------------------------------------------------------------------------------------------------ the fixture
def load_fixture(path):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def fixture_case(fx, name):
    """(input record, reference bytes, decoded record) of one case"""
    return parse_record(fx[name + "/in"].tobytes())[0], fx[name + "/bytes"].tobytes(), parse_record(fx[name + "/dec"].tobytes())[0]


def wire_records(ref_bytes):
    """The 44-byte edge records of a reference EdgeArrayMessage / CondensedGraphMessage, verbatim."""
    (n,) = struct.unpack_from("<Q", ref_bytes, 8)
    return np.frombuffer(ref_bytes, dtype=np.uint8, count=44 * n, offset=16).reshape(n, 44).copy()
