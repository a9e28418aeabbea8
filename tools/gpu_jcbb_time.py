"""What the joint-compatibility search (cgmr_jcbb_dense, cgmr_joint_compatibility) costs, for the choice of
CGMR_JC_DEFAULT_NODE_LIMIT.

  python tools/gpu_jcbb_time.py [reps]            runs the three steps below, each in a process of its own under a time limit
  python tools/gpu_jcbb_time.py [reps] --step S   one step: rate | worst | graph

The driver stops at the first step that does not end with status 0 (a fault, an abort or its time limit): nothing is started on
the device after that.

rate   the ambiguous-row family of tests/jcbb_cases.py (landmarks 0.5 m apart along the line of sight, the pose's variance
       along it 4) at (M, L) = (8, 12), (16, 64), (32, 256), at node limit 512 and at the default: device ms of one call
       (events on the context's stream, the median of ``reps`` (5) warm calls), the joint tests made and tests per second
       over the call.
worst  the cap shape (32, 256) with the pose's variance along the row 4, 100 and 1e4 -- the larger, the more landmarks every
       measurement is individually compatible with and the deeper every root searches --, and jcbb_cases.decoy_row, where the
       greedy hypothesis has one pairing and the first round prunes no root by the count, at node limits 64 .. 4096: the
       largest time of a limit over the four is what a call costs in which the roots spend their budgets.
graph  tree600b (tests/assoc_cases.py) after three Gauss-Newton iterations: the scan of jcbb_cases.graph_scene through
       GraphSLAM.gateObservations (the gate alone, one call per kind) and through Context.joint_compatibility.
The figures are in DESIGN.md section 2.9."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"rate": 240, "worst": 420, "graph": 240}                  # seconds a step may take
ARGS = [a for a in sys.argv[1:] if a.isdigit()]
REPS = int(ARGS[0]) if ARGS else 5


def driver():
    for step, limit in STEPS.items():
        print(f"--- {step} (at most {limit} s)", flush=True)
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), str(REPS), "--step", step], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            print(f"{step}: not finished after {limit} s; stopping here", flush=True)
            return 124
        if rc != 0:
            print(f"{step}: ended with status {rc}; stopping here", flush=True)
            return rc
    return 0


def main(step):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch

    import jcbb_cases as JC
    from cg_mrslam_amd import Context
    from cg_mrslam_amd._lib import JC_DEFAULT_NODE_LIMIT, JC_ROUNDS

    stream = torch.cuda.Stream(0)
    ctx = Context(0, stream=stream.cuda_stream)

    def device_ms(fn):
        """(median, minimum) device ms of REPS warm calls, and the last result."""
        out = fn()
        t = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            out = fn()
            e1.record(stream)
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1))
        return float(np.median(t)), float(min(t)), out

    def dense(P, limit):
        return ctx.jcbb_dense(P["slot"], P["dim"], P["sigma"], P["e"], P["J"], P["R"], P["gamma"], node_limit=limit)

    def report(tag, P, limit):
        med, lo, (assign, count, d2, dof, proven, ic, nodes) = device_ms(lambda: dense(P, limit))
        roots = int(np.sum(ic < P["gamma"][2]))
        print(f"  {tag} node_limit {limit}: device median {med:.3f} min {lo:.3f} ms, count {count} of {P['M']}, dof {dof}, proven {proven}, "
              f"{roots} roots, {nodes} tests = {nodes / max(1, roots * JC_ROUNDS * limit):.1%} of the budget, "
              f"{nodes / (1e-3 * med):.3e} tests/s over the call", flush=True)
        return med

    print(f"default node limit {JC_DEFAULT_NODE_LIMIT}, {JC_ROUNDS} rounds, {REPS} repetitions")
    if step == "rate":
        for M, L in ((8, 12), (16, 64), (32, 256)):
            for limit in (512, JC_DEFAULT_NODE_LIMIT):
                report(f"row ({M}, {L})", JC.row(M, L), limit)
    elif step == "worst":
        worst = {}
        families = [(f"row (32, 256), variance {v:g},", JC.row(32, 256, x_var=v)) for v in (4.0, 100.0, 1e4)]
        families.append(("decoy row (32, 256), variance 1e4,", JC.decoy_row(32, 256)))
        for tag, P in families:
            for limit in (64, 256, 512, 1024, 2048, 4096):
                med = report(tag, P, limit)
                worst[limit] = max(worst.get(limit, 0.0), med)
                if med > 1000.0:
                    break
        for limit, ms in sorted(worst.items()):
            print(f"node_limit {limit}: slowest call {ms:.3f} ms ({'at or under' if ms <= 270.0 else 'over'} 270 ms)")
    elif step == "graph":
        import assoc_cases as AC
        from cg_mrslam_amd.graph import GraphSLAM, PoseGraph
        g = AC.case("tree600b")
        rc, p, _ = ctx.gn_optimize_typed(*AC.args(g), 3, vertex_kind=g["vk"], edge_kind=g["ek"])
        assert rc == 0
        sc = JC.graph_scene(g)
        s = GraphSLAM(PoseGraph(np.arange(len(p)), p, g["fixed"], *AC.args(g)[2:], vertex_kind=g["vk"], edge_kind=g["ek"]), ctx)
        xy = sc["kinds"] == 1
        z, info = sc["meas"][:, :2], sc["info"][:, [0, 1, 3]]
        med, lo, _ = device_ms(lambda: s.gateObservations(sc["pose"], sc["lms"], z[xy], info[xy], kind=1))
        print(f"  gateObservations, {int(xy.sum())} xy measurements x {len(sc['lms'])} landmarks: device median {med:.3f} min {lo:.3f} ms")
        med, lo, _ = device_ms(lambda: s.gateObservations(sc["pose"], sc["lms"], z[~xy, 0], info[~xy, 0], kind=2))
        print(f"  gateObservations, {int((~xy).sum())} bearing x {len(sc['lms'])} landmarks: device median {med:.3f} min {lo:.3f} ms")
        med, lo, (assign, d2, dof, proven) = device_ms(lambda: s.associateObservations(sc["pose"], sc["lms"], z, info, kind=sc["kinds"]))
        print(f"  associateObservations, all {len(z)}: device median {med:.3f} min {lo:.3f} ms; assign {assign.tolist()}, dof {dof}, proven {proven}")
    else:
        raise SystemExit(f"unknown step {step!r}: one of {', '.join(STEPS)}")
    ctx.close()


if __name__ == "__main__":
    if "--step" in sys.argv:
        main(sys.argv[sys.argv.index("--step") + 1])
    else:
        sys.exit(driver())
