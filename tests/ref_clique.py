"""Exact maximum clique on Python integers as bit sets: a branch and bound with the greedy colouring bound (San Segundo's
BBMC), the yardstick of cgmr_max_clique_exact beyond the 20 vertices ref_pcm.max_clique_exact (Bron-Kerbosch) reaches.
TEST INFRASTRUCTURE ONLY; shares no code with the device, and is built differently: one search over the whole graph from an
empty clique, recursive, the colour-ordered candidate list kept per level and walked from the highest colour down.

    max_clique(A) -> (members ascending, nodes)          omega(A) -> (omega, nodes)

The vertices are relabelled by descending degree (ties: ascending index); bit i of a set is the vertex with label i.  A node
(C, P): P is coloured greedily in label order, class by class -- a class takes every vertex not adjacent to one it holds --,
which gives the list v_1 .. v_m with colours c_1 <= .. <= c_m.  From j = m down: if |C| + c_j <= best the node is done (no
clique through the vertices left can be larger); else v_j joins C, the child (C + v_j, P & N(v_j)) is searched, and v_j leaves
P.  A node without candidates records C when it is larger than the best so far.  `nodes` counts the (C, P) pairs searched, the
root's included."""
import sys

import numpy as np


def _rows(A):
    """(neighbour sets in labels, vertex of every label) with labels by descending degree, ties by ascending index."""
    A = np.asarray(A, dtype=bool)
    n = len(A)
    order = sorted(range(n), key=lambda v: (-int(A[v].sum()), v))
    label = {v: i for i, v in enumerate(order)}
    rows = []
    for v in order:
        m = 0
        for u in np.flatnonzero(A[v]).tolist():
            if u != v:
                m |= 1 << label[u]
        rows.append(m)
    return rows, order


def _colour(P, rows):
    """The candidates of P in colour order and their colours (1, 2, ..)."""
    vs, cs = [], []
    k = 0
    while P:
        k += 1
        Q = P
        while Q:
            low = Q & -Q
            v = low.bit_length() - 1
            vs.append(v)
            cs.append(k)
            P ^= low
            Q &= ~(rows[v] | low)
    return vs, cs


def max_clique(A, lower_bound=0):
    """(a maximum clique's members ascending, nodes searched).  With ``lower_bound`` only larger cliques are looked for; the
    members are [] when there is none."""
    rows, order = _rows(A)
    n = len(rows)
    state = {"best": int(lower_bound), "set": 0, "nodes": 0}
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 4 * n + 100))

    def search(C, size, P):
        state["nodes"] += 1
        if not P:
            if size > state["best"]:
                state["best"], state["set"] = size, C
            return
        vs, cs = _colour(P, rows)
        for j in range(len(vs) - 1, -1, -1):
            if size + cs[j] <= state["best"]:
                return
            v = vs[j]
            search(C | (1 << v), size + 1, P & rows[v])
            P &= ~(1 << v)

    try:
        search(0, 0, (1 << n) - 1)
    finally:
        sys.setrecursionlimit(limit)
    members = sorted(order[i] for i in range(n) if (state["set"] >> i) & 1)
    return members, state["nodes"]


def omega(A):
    """(the clique number, nodes searched)."""
    members, nodes = max_clique(A)
    return len(members), nodes


def is_clique(A, members):
    """Distinct, ascending, pairwise adjacent."""
    m = [int(v) for v in members]
    A = np.asarray(A, dtype=bool)
    return m == sorted(set(m)) and all(A[i, j] for i in m for j in m if i != j)
