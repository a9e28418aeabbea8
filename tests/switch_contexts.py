"""Contexts under environment switches, in-process.  A context reads the context-scoped CGMR_* variables once, when it is
created (csrc/switches.h), so a launch variant is a context made under its variables -- no child process.  The entry points
without a context (gn_symbolic_info, ...) read them when called: ``environment`` around the call."""
import contextlib
import os

from cg_mrslam_amd._lib import gn_symbolic_info


@contextlib.contextmanager
def environment(env):
    """``env`` set in os.environ inside the block, the previous values back behind it."""
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def assert_held(c, env):
    """The context holds every variable of ``env`` at the value given (not silently the default)."""
    sw = c.switches()
    for k, v in env.items():
        assert k in sw and sw[k] == int(v), (k, v, sw.get(k))


@contextlib.contextmanager
def context_under(env, device=0):
    """A Context created under ``env``; the environment is restored before the block runs, the context closed behind it (one
    variant's arenas are gone before the next variant's context is made)."""
    from cg_mrslam_amd import Context
    with environment(env):
        c = Context(device)
    try:
        assert_held(c, env)
        yield c
    finally:
        c.close()


def launch_counts(c, a):
    """Launches of one Gauss-Newton pass on the problem ``a`` by class (profiling mode counts them)."""
    c.set_profiling(True)
    try:
        rc, _, _ = c.gn_optimize(*a, 1)
        assert rc == 0
        t = c.gn_kernel_times()
    finally:
        c.set_profiling(False)
    return {k: v[1] for k, v in t.items()}


def assert_launch_shape(c, env, a):
    """What the launch-shape switches of ``env`` must do to a pass on the problem ``a`` = (poses, fixed, ef, et, meas, info)."""
    with environment(env):
        info = gn_symbolic_info(len(a[0]), a[1], a[2], a[3])
    n = launch_counts(c, a)
    if env.get("CGMR_FWD_MERGE") == "0":
        assert n["front_level"] == 0, n
    if env.get("CGMR_BWD_CHAIN") == "0":
        assert n["solve_bwd"] == info["launch_levels"], (n, info["launch_levels"])
    if env.get("CGMR_TOP_BLOCK") == "0":
        assert info["top_block_fronts"] == 0, info
