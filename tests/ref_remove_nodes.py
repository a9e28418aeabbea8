"""Float64 numpy reference of vertex removal (include/cgmr.h: cgmr_remove_nodes; GraphSLAM.removeVertices).  TEST INFRASTRUCTURE
ONLY, written from the definitions:

  1. the local configuration of a removed vertex v: v at ``xv`` (the identity unless a test moves it), each neighbour n at
     xv (+) z_vn of the lowest-index edge between v and n, inverted where the edge is stored n -> v;
  2. H = sum J^T Omega J over all incident edges there (ref_numpy.build_system on the star as a graph of its own);
  3. one neighbour fixed (the lowest unless a test picks another), the rest factored by np.linalg.cholesky (flag 1 without a
     factor) and inverted densely; the blocks of the neighbours, zeros for the fixed one;
  4. the weights by ref_condense_tree.weights (log det Sigma_z from a Cholesky factor);
  5. the tree by ref_condense_tree.kruskal -- not the device's Prim -- rooted at the lowest neighbour;
  6. the labels by ref_condense_tree.label_first_order;
  7. m - 1 edges per removed vertex in order of the child; flags 0, 1, 2 (more than MAX_DEGREE neighbours), 3 (a chosen weight
     is +inf)."""
import numpy as np

import ref_condense_tree as T
import ref_joint_marginals as J
import ref_numpy as R

MAX_DEGREE = 16


def incident(ef, et, v):
    """(inc, other, nbrs): v's incident edges in index order, the other end of each, the distinct neighbours sorted."""
    ef, et = np.asarray(ef), np.asarray(et)
    inc = np.flatnonzero((ef == v) | (et == v))
    other = np.where(ef[inc] == v, et[inc], ef[inc])
    return inc, other, np.unique(other)


def local_star(ef, et, meas, info, v, fix=0, xv=(0.0, 0.0, 0.0)):
    """Steps 1 to 3 for vertex v.  Returns a dict: nbrs [m], x [m, 3] (the neighbours' local poses), xv, the star as a graph
    (poses: v then the neighbours; lef, let, inc), H (v, then the neighbours but the fixed one), Sigma [3 m, 3 m] over the
    neighbours in order (zero rows for the fixed one) or None without a Cholesky factor."""
    ef, et = np.asarray(ef), np.asarray(et)
    meas, info = np.asarray(meas, dtype=np.float64).reshape(-1, 3), np.asarray(info, dtype=np.float64).reshape(-1, 6)
    inc, other, nbrs = incident(ef, et, v)
    m = len(nbrs)
    xv = np.asarray(xv, dtype=np.float64)
    x = np.zeros((m, 3))
    for k, n in enumerate(nbrs):
        e = inc[other == n][0]
        z = meas[e] if ef[e] == v else R._se2_inv(meas[e])
        x[k] = R._se2_mul(xv, z)
    node = 1 + np.searchsorted(nbrs, other)
    lef = np.where(ef[inc] == v, 0, node).astype(np.int32)
    let = np.where(ef[inc] == v, node, 0).astype(np.int32)
    poses = np.vstack([xv[None, :], x])
    out = dict(v=int(v), nbrs=nbrs, x=x, xv=xv, poses=poses, lef=lef, let=let, inc=inc, fix=int(fix), H=None, Sigma=None)
    if m < 2:
        return out
    fixed = np.zeros(m + 1, np.uint8)
    fixed[1 + fix] = 1
    H, _, hidx = R.build_system(poses, fixed, lef, let, meas[inc], info[inc])
    H = H.toarray()
    out["H"] = H
    try:
        if not np.all(np.isfinite(H)):
            raise np.linalg.LinAlgError
        np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return out
    Hinv = np.linalg.inv(H)
    Hinv = 0.5 * (Hinv + Hinv.T)
    Sigma = np.zeros((3 * m, 3 * m))
    free = [k for k in range(m) if k != fix]
    for a in free:
        for b in free:
            ia, ib = hidx[1 + a], hidx[1 + b]
            Sigma[3 * a:3 * a + 3, 3 * b:3 * b + 3] = Hinv[3 * ia:3 * ia + 3, 3 * ib:3 * ib + 3]
    out["Sigma"] = Sigma
    return out


def pair_weights(star):
    """W [m, m] over the neighbours in order, by ref_condense_tree.weights with the fixed neighbour in the gauge's place."""
    m, fix = len(star["nbrs"]), star["fix"]
    perm = np.array([fix] + [k for k in range(m) if k != fix])
    keep = np.concatenate([np.arange(3 * k, 3 * k + 3) for k in perm[1:]])
    Wp, _ = T.weights(star["x"], perm, star["Sigma"][np.ix_(keep, keep)])
    W = np.full((m, m), np.inf)
    W[np.ix_(perm, perm)] = Wp
    return W


def remove_one(ef, et, meas, info, v, fix=0, xv=(0.0, 0.0, 0.0)):
    """Steps 1 to 7 for one vertex: local_star's dict plus flag, and with flag 0 and m >= 2: W, parent [m] (nodes 0 .. m - 1,
    node 0 the root), margin, fr, to (vertex indices), est [m - 1, 3], iu [m - 1, 6], weight [m - 1], Sz [m - 1, 3, 3]."""
    inc, other, nbrs = incident(ef, et, v)
    m = len(nbrs)
    none = dict(fr=np.zeros(0, np.int32), to=np.zeros(0, np.int32), est=np.zeros((0, 3)), iu=np.zeros((0, 6)), weight=np.zeros(0))
    if m > MAX_DEGREE:
        return dict(v=int(v), nbrs=nbrs, flag=2, **none)
    star = local_star(ef, et, meas, info, v, fix, xv)
    if m < 2:
        return dict(star, flag=0, **none)
    if star["Sigma"] is None:
        return dict(star, flag=1, **none)
    W = pair_weights(star)
    parent = T.kruskal(W, root=0)
    weight = np.array([W[k, parent[k]] for k in range(1, m)])
    if not np.all(np.isfinite(weight)):
        return dict(star, flag=3, W=W, **none)
    S, x = star["Sigma"], star["x"]
    blk = lambda a, b: S[3 * a:3 * a + 3, 3 * b:3 * b + 3]   # noqa: E731
    est, iu, Szs = np.zeros((m - 1, 3)), np.zeros((m - 1, 6)), np.zeros((m - 1, 3, 3))
    for k in range(1, m):
        p = int(parent[k])
        Szs[k - 1] = J.relative_cov(x[p], x[k], blk(p, p), blk(p, k), blk(k, k))
        est[k - 1], iu[k - 1] = T.label_first_order(x[p], x[k], Szs[k - 1])
    return dict(star, flag=0, W=W, parent=parent, margin=T.decision_margin(W, parent), fr=nbrs[parent[1:]].astype(np.int32),
                to=nbrs[1:].astype(np.int32), est=est, iu=iu, weight=weight, Sz=Szs)


def check_call(nV, ef, et, remove):
    """What cgmr_remove_nodes refuses: the reason, or None."""
    ef, et, remove = np.asarray(ef), np.asarray(et), np.asarray(remove)
    if len(ef) and (min(ef.min(), et.min()) < 0 or max(ef.max(), et.max()) >= nV):
        return "edge index out of range"
    if len(remove) and (remove.min() < 0 or remove.max() >= nV):
        return "remove index out of range"
    if len(np.unique(remove)) != len(remove):
        return "repeated vertex"
    rm = np.zeros(nV, bool)
    rm[remove] = True
    if np.any(rm[ef] & (ef == et)):
        return "self edge"
    if np.any(rm[ef] & rm[et]):
        return "not independent"
    return None


def remove_nodes(nV, ef, et, meas, info, remove):
    """cgmr_remove_nodes restated: a dict of off [nR + 1], fr, to, est, iu, weight, flags [nR], margin (the smallest decision
    margin of the removed vertices' trees) and per (the remove_one dicts).  Raises ValueError where the call is refused."""
    why = check_call(nV, ef, et, remove)
    if why:
        raise ValueError(why)
    per = [remove_one(ef, et, meas, info, int(v)) for v in remove]
    off = np.concatenate([[0], np.cumsum([len(p["to"]) for p in per])]).astype(np.int32)
    cat = lambda k, shape, dt: np.concatenate([np.zeros(0)] + [p[k].ravel() for p in per]).astype(dt).reshape(shape)   # noqa: E731
    return dict(off=off, fr=cat("fr", (-1,), np.int32), to=cat("to", (-1,), np.int32), est=cat("est", (-1, 3), np.float64),
                iu=cat("iu", (-1, 6), np.float64), weight=cat("weight", (-1,), np.float64),
                flags=np.array([p["flag"] for p in per], dtype=np.int32),
                margin=min([p["margin"] for p in per if "margin" in p] + [np.inf]), per=per)


# ------------------------------------------------------------------------------------------- rewriting a graph
def independent_round(ef, et, wanted):
    """Of ``wanted`` (sorted), in index order, the vertices not adjacent in (ef, et) to one already taken."""
    taken, blocked = [], set()
    adj = {}
    for a, b in zip(ef.tolist(), et.tolist()):
        adj.setdefault(a, set()).add(b)
        adj.setdefault(b, set()).add(a)
    for v in wanted:
        if v not in blocked:
            taken.append(v)
            blocked |= adj.get(v, set())
    return taken


def remove_vertices(nV, ef, et, meas, info, indices):
    """GraphSLAM.removeVertices restated on bare arrays, vertex indices unchanged: rounds of independent sets, each round's
    vertices and their edges deleted and the new edges appended before the next.  Returns (ef, et, meas, info, skipped) with
    skipped = [(vertex, flag), ...]; the vertices of ``indices`` not skipped have no edge left."""
    ef, et = np.asarray(ef, dtype=np.int32).copy(), np.asarray(et, dtype=np.int32).copy()
    meas, info = np.asarray(meas, dtype=np.float64).reshape(-1, 3).copy(), np.asarray(info, dtype=np.float64).reshape(-1, 6).copy()
    left, skipped = sorted(set(int(v) for v in indices)), []
    while left:
        take = independent_round(ef, et, left)
        out = remove_nodes(nV, ef, et, meas, info, np.array(take, dtype=np.int32))
        gone = [v for v, f in zip(take, out["flags"]) if f == 0]
        skipped += [(v, int(f)) for v, f in zip(take, out["flags"]) if f != 0]
        keep = ~(np.isin(ef, gone) | np.isin(et, gone))
        ef, et = np.concatenate([ef[keep], out["fr"]]), np.concatenate([et[keep], out["to"]])
        meas, info = np.vstack([meas[keep], out["est"]]), np.vstack([info[keep], out["iu"]])
        left = [v for v in left if v not in take]
    return ef, et, meas, info, skipped


def compact(nV, gone):
    """The old-to-new index map [nV] after deleting the vertices ``gone``: -1 for them."""
    keep = np.ones(nV, bool)
    keep[list(gone)] = False
    new = np.full(nV, -1, dtype=np.int64)
    new[keep] = np.arange(int(keep.sum()))
    return new
