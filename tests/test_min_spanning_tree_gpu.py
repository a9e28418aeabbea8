"""cgmr_min_spanning_tree -- the single-workgroup Prim of condense_tree_kernels.hip -- against the Kruskal reference
(ref_condense_tree.kruskal), byte for byte: integer-valued weights make every comparison exact, and under the total order
(w, max(a, b), min(a, b)) the tree is unique whichever algorithm finds it.  The sizes straddle the wavefront (64, 65), the
workgroup (256, 257: a thread owns more than one node) and reach the limit (1025: the fifth node of thread 0)."""
import numpy as np
import pytest

import ref_condense_tree as T
from cg_mrslam_amd._lib import TREE_MAX_NODES, CgmrError

pytestmark = pytest.mark.gpu

E_INVALID = -1
SIZES = [1, 2, 3, 64, 65, 256, 257, 1024, 1025]


def _sym(L):
    L = np.tril(L, -1)
    return L + L.T


def _check(ctx, W, root=0):
    got = ctx.min_spanning_tree(W, root)
    want = T.kruskal(W, root)
    assert got.dtype == np.int32 and got.tobytes() == want.tobytes(), (W.shape[0], root, np.flatnonzero(got != want)[:8])
    return got


@pytest.mark.parametrize("n", SIZES)
def test_equal_random_and_path_weights(ctx, n):
    assert TREE_MAX_NODES == 1025
    rng = np.random.default_rng(n)
    star = _check(ctx, np.ones((n, n)))
    assert star[0] == -1 and np.all(star[1:] == 0)                # all weights equal: a star on node 0
    W = _sym(rng.integers(0, 8, (n, n)).astype(np.float64))       # many ties
    _check(ctx, W)
    # path-graph weights: |a - b|, the tree is the path 0 - 1 - ... - (n - 1)
    k = np.arange(n)
    path = _check(ctx, np.abs(k[:, None] - k[None, :]).astype(np.float64))
    assert np.array_equal(path, k - 1)
    # ... and with the nodes relabelled at random, a path that winds through the workgroup's threads
    perm = rng.permutation(n)
    _check(ctx, np.abs(perm[:, None] - perm[None, :]).astype(np.float64))


@pytest.mark.parametrize("n", [3, 65, 257, 1025])
def test_nan_infinite_row_root_and_lower_triangle(ctx, n):
    rng = np.random.default_rng(100 + n)
    W = _sym(rng.integers(0, 8, (n, n)).astype(np.float64))
    v = n // 2
    W[v, :] = W[:, v] = np.inf                                    # a +inf row hangs on node 0
    W[n - 1, 0] = W[0, n - 1] = np.nan                            # a NaN entry counts as +inf
    p = _check(ctx, W)
    assert p[v] == 0
    for root in (n - 1, v, 1):                                    # a non-zero root: the same edges, oriented from it
        pr = _check(ctx, W, root)
        assert pr[root] == -1
        assert {(max(a, int(b)), min(a, int(b))) for a, b in enumerate(pr) if b >= 0} == \
               {(max(a, int(b)), min(a, int(b))) for a, b in enumerate(p) if b >= 0}
    # only the lower triangle is read
    U = np.tril(W, -1) + np.triu(np.full((n, n), -5.0), 0)
    assert ctx.min_spanning_tree(U).tobytes() == p.tobytes()


def test_limits_and_two_calls_give_identical_bytes(ctx):
    n = TREE_MAX_NODES + 1
    for call in (lambda: ctx.min_spanning_tree(np.ones((n, n))),
                 lambda: ctx.min_spanning_tree(np.ones((5, 5)), 5),
                 lambda: ctx.min_spanning_tree(np.ones((5, 5)), -1),
                 lambda: ctx.min_spanning_tree(np.ones((0, 0)))):
        with pytest.raises(CgmrError) as ei:
            call()
        assert ei.value.code == E_INVALID
    W = _sym(np.random.default_rng(9).normal(size=(700, 700)))    # real-valued weights: no ties at all
    a = ctx.min_spanning_tree(W, 3)
    b = ctx.min_spanning_tree(W, 3)
    assert a.tobytes() == b.tobytes() == T.kruskal(W, 3).tobytes()
