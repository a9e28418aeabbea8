"""Host-side mirror of the reference's optimiser interface for the hot path.

``GraphSLAM.optimize(nrunnings)`` has the reference's name, argument and error behaviour
(``void GraphSLAM::optimize(int nrunnings)``, src/slam/graph_slam.cpp:561-575: the solver status
is swallowed, the poses are simply left where the last successful iteration put them) but runs
on the MI355X through libcgmr.so.  ``PoseGraph`` is the flat-array form of the g2o graph the
reference keeps in a ``SparseOptimizer`` (vertices = VertexSE2 ids + estimates + fixed flags,
edges = EdgeSE2 measurement + information), with the ``.g2o`` text reader/writer of
``GraphSLAM::saveGraph/loadGraph`` (src/slam/graph_slam.cpp:620-628).
"""
from __future__ import annotations

import numpy as np

from ._lib import CGMR_E_CHOLESKY_BASE, DL_DEFAULTS, REMOVE_MAX_DEGREE, Context, dl_params_checked, robust_arrays, robust_code

ODOM_INFO = (100.0, 100.0, 1000.0)      # _odominf, src/slam/graph_slam.cpp:72-73
SM_INFO = (1000.0, 1000.0, 10000.0)     # _SMinf,   src/slam/graph_slam.cpp:75-76


class RobotLaser:
    """The ``ROBOTLASER1`` data element g2o attaches to a vertex (RobotLaser::read/write [g2o-recalled], SURVEY.md
    Appendix D): laser parameters, ranges, remissions, odometry pose and the laser's pose on the robot."""

    def __init__(self, ranges, first_beam_angle, angular_step, max_range, odom_pose=(0.0, 0.0, 0.0),
                 laser_pose=(0.0, 0.0, 0.0), laser_type=0, accuracy=0.1, remission_mode=0, fov=None, remissions=(),
                 tail=("0", "0", "0", "0", "0"), timestamp="0", hostname="hostname", logger_timestamp="0"):
        self.ranges = np.ascontiguousarray(ranges, dtype=np.float32)
        self.first_beam_angle, self.angular_step, self.max_range = float(first_beam_angle), float(angular_step), float(max_range)
        self.fov = float(angular_step) * len(self.ranges) if fov is None else float(fov)     # LaserParameters ctor
        self.laser_type, self.accuracy, self.remission_mode = int(laser_type), float(accuracy), int(remission_mode)
        self.remissions = np.ascontiguousarray(remissions, dtype=np.float64)
        self.odom_pose = np.asarray(odom_pose, dtype=np.float64).copy()
        self.laser_pose = np.asarray(laser_pose, dtype=np.float64).copy()                      # laser in the robot frame
        self.tail = tuple(str(v) for v in tail)               # laserTv laserRv forwardSafetyDist sideSafetyDist turnAxis
        self.timestamp, self.hostname, self.logger_timestamp = str(timestamp), str(hostname), str(logger_timestamp)

    def write(self, fmt="%g"):
        from .matcher import _se2_mul
        w = _se2_mul(self.odom_pose, self.laser_pose)         # laser pose in the world
        tok = ["ROBOTLASER1", str(self.laser_type), fmt % self.first_beam_angle, fmt % self.fov, fmt % self.angular_step,
               fmt % self.max_range, fmt % self.accuracy, str(self.remission_mode), str(len(self.ranges))]
        tok += [fmt % float(r) for r in self.ranges]
        tok.append(str(len(self.remissions)))
        tok += [fmt % float(r) for r in self.remissions]
        tok += [fmt % v for v in (*w, *self.odom_pose)]
        tok += [*self.tail, self.timestamp, self.hostname, self.logger_timestamp]
        return " ".join(tok)

    @classmethod
    def read(cls, tok):
        """``tok``: the whitespace-split line including the leading ROBOTLASER1 tag."""
        from .matcher import _se2_inv, _se2_mul
        laser_type, first, fov, step, max_range, acc = int(tok[1]), *(float(v) for v in tok[2:7])
        rem_mode = int(tok[7])
        nb = int(tok[8])
        ranges = np.array([float(v) for v in tok[9:9 + nb]], dtype=np.float32)
        q = 9 + nb
        nr = int(tok[q])
        rem = [float(v) for v in tok[q + 1:q + 1 + nr]]
        q += 1 + nr
        world = np.array([float(v) for v in tok[q:q + 3]])
        odom = np.array([float(v) for v in tok[q + 3:q + 6]])
        q += 6
        return cls(ranges, first, step, max_range, odom_pose=odom, laser_pose=_se2_mul(_se2_inv(odom), world),
                   laser_type=laser_type, accuracy=acc, remission_mode=rem_mode, fov=fov, remissions=rem,
                   tail=tok[q:q + 5], timestamp=tok[q + 5], hostname=tok[q + 6], logger_timestamp=tok[q + 7])


class PoseGraph:
    def __init__(self, ids, poses, fixed, edge_from, edge_to, meas, info, edge_level=None, vertex_kind=None, edge_kind=None):
        self.ids = np.ascontiguousarray(ids, dtype=np.int64)
        self.poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3).copy()
        self.fixed = np.ascontiguousarray(fixed, dtype=np.uint8).copy()
        self.edge_from = np.ascontiguousarray(edge_from, dtype=np.int32)   # vertex *indices*
        self.edge_to = np.ascontiguousarray(edge_to, dtype=np.int32)
        self.meas = np.ascontiguousarray(meas, dtype=np.float64).reshape(-1, 3)
        self.info = np.ascontiguousarray(info, dtype=np.float64).reshape(-1, 6)
        # g2o edge level: 0 = optimised, r+1 = condensed graph built for robot r
        # (src/mrslam/condensed_graph/condensed_graph_buffer.cpp:469-473)
        self.edge_level = (np.zeros(len(self.edge_from), dtype=np.int32) if edge_level is None
                           else np.ascontiguousarray(edge_level, dtype=np.int32))
        self.lasers = {}          # vertex index -> RobotLaser (user data; written/read as ROBOTLASER1 lines)
        # typed factors (include/cgmr.h: cgmr_factor_types): per vertex 0 = SE2 pose, 1 = point (VERTEX_XY; its third pose
        # component stays 0); per edge 0 = EDGE_SE2, 1 = EDGE_SE2_XY, 2 = EDGE_BEARING_SE2_XY, 3 = EDGE_PRIOR_SE2, 4 =
        # EDGE_PRIOR_SE2_XY (priors: from == to).  A 2-dimensional factor keeps (zx, zy, 0) and (I11, I12, 0, I22, 0, 0), a bearing
        # (z, 0, 0) and (I, 0, 0, 0, 0, 0).  None: a pure pose graph, as ever.
        self.vertex_kind = None if vertex_kind is None else np.ascontiguousarray(vertex_kind, dtype=np.uint8).copy()
        self.edge_kind = None if edge_kind is None else np.ascontiguousarray(edge_kind, dtype=np.uint8).copy()
        # max-mixture edges (include/cgmr.h: cgmr_mixture): edge index -> (meas [K, 3], info [K, 6], weight [K]), K >= 2, in the
        # padded layout of meas / info; row 0 is the edge's own (meas, info), which every other call goes on reading.  Empty: a
        # graph without mixtures, as ever.
        self.mixtures = {}

    @property
    def has_mixtures(self):
        """True when some edge has more than one component (the solver then takes the mixture entry points)."""
        return bool(self.mixtures)

    def set_edge_mixture(self, edge, components):
        """Make edge ``edge`` a mixture of ``components`` = [(weight, meas, info), ...] in add_edge's value counts; component 0
        becomes the edge's own (meas, info).  One component: a plain edge again."""
        k = int(edge)
        if not 0 <= k < self.n_edges:
            raise ValueError(f"edge index out of range 0..{self.n_edges - 1}")
        comps = list(components)
        if not comps:
            raise ValueError("a mixture edge needs at least one component")
        kind = int(self.kinds()[1][k])
        zs, us, ws = np.zeros((len(comps), 3)), np.zeros((len(comps), 6)), np.zeros(len(comps))
        for c, (w, meas, info) in enumerate(comps):
            zs[c], us[c] = self._pad_factor(kind, meas, info)
            ws[c] = float(w)
        self.meas[k], self.info[k] = zs[0], us[0]
        if len(comps) > 1:
            self.mixtures[k] = (zs, us, ws)
        else:
            self.mixtures.pop(k, None)

    def mixture_arrays(self, level0=True):
        """(comp_ptr [n + 1], comp_meas [nC, 3], comp_info [nC, 6], comp_weight [nC]) over the level-0 edges in level0() order
        (``level0=False``: over all edges), or None for a graph without mixtures."""
        if not self.mixtures:
            return None
        idx = np.flatnonzero(self.edge_level == 0) if level0 else np.arange(self.n_edges)
        ptr, zs, us, ws = [0], [], [], []
        for k in idx:
            mz, mu, mw = self.mixtures.get(int(k), (self.meas[k][None, :], self.info[k][None, :], np.ones(1)))
            if int(k) in self.mixtures:
                mz = mz.copy()
                mu = mu.copy()
                mz[0], mu[0] = self.meas[k], self.info[k]          # (component 0 is the edge's own, wherever it was changed)
            zs.append(mz)
            us.append(mu)
            ws.append(mw)
            ptr.append(ptr[-1] + len(mw))
        if ptr[-1] == len(idx):
            return None                                            # (the mixtures are on edges of other levels)
        return (np.asarray(ptr, dtype=np.int32), np.concatenate(zs).reshape(-1, 3), np.concatenate(us).reshape(-1, 6),
                np.concatenate(ws))

    @staticmethod
    def _pad_factor(kind, meas, info):
        """(meas [3], info [6]) of a factor of ``kind`` from add_edge's value counts."""
        m, u = np.zeros(3), np.zeros(6)
        mv, uv = np.asarray(meas, dtype=np.float64).reshape(-1), np.asarray(info, dtype=np.float64).reshape(-1)
        if kind in (1, 4):
            m[:2] = mv[:2]
            u[[0, 1, 3]] = uv[:3] if uv.size == 3 else uv[[0, 1, 3]]
        elif kind == 2:
            m[0], u[0] = mv[0], uv[0]
        else:
            m[:], u[:] = mv[:3], uv[:6]
        return m, u

    @property
    def typed(self):
        """True when some vertex or edge is not of kind 0 (the solver then takes the typed entry points)."""
        return bool((self.vertex_kind is not None and self.vertex_kind.any()) or
                    (self.edge_kind is not None and self.edge_kind.any()))

    def kinds(self):
        """(vertex kinds [nV], edge kinds [nE]) with zeros where none were given."""
        vk = self.vertex_kind if self.vertex_kind is not None else np.zeros(self.n_vertices, dtype=np.uint8)
        ek = self.edge_kind if self.edge_kind is not None else np.zeros(self.n_edges, dtype=np.uint8)
        return vk, ek

    def add_vertex(self, vid, estimate, kind=0, fixed=False):
        """Append a vertex (``estimate``: (x, y, theta), or (x, y) for a point); returns its index."""
        est = np.zeros(3)
        est[:2 if kind == 1 else 3] = np.asarray(estimate, dtype=np.float64).reshape(-1)[:2 if kind == 1 else 3]
        vk, _ = self.kinds()
        self.ids = np.append(self.ids, np.int64(vid))
        self.poses = np.vstack([self.poses, est[None, :]])
        self.fixed = np.append(self.fixed, np.uint8(1 if fixed else 0))
        if kind or self.vertex_kind is not None:
            self.vertex_kind = np.append(vk, np.uint8(kind))
        return self.n_vertices - 1

    def add_edge(self, i, j, meas, info, kind=0, level=0):
        """Append an edge between the vertex indices ``i`` and ``j`` (a prior: i == j).  ``meas`` / ``info``: 3 and 6 values, or
        2 and 3 (I11, I12, I22) for a 2-dimensional factor, or one of each for a bearing (kind 2); returns the edge's index."""
        m, u = np.zeros(3), np.zeros(6)
        mv, uv = np.asarray(meas, dtype=np.float64).reshape(-1), np.asarray(info, dtype=np.float64).reshape(-1)
        if kind in (1, 4):
            m[:2] = mv[:2]
            u[[0, 1, 3]] = uv[:3] if uv.size == 3 else uv[[0, 1, 3]]
        elif kind == 2:
            m[0], u[0] = mv[0], uv[0]
        else:
            m[:], u[:] = mv[:3], uv[:6]
        _, ek = self.kinds()
        self.edge_from = np.append(self.edge_from, np.int32(i))
        self.edge_to = np.append(self.edge_to, np.int32(j))
        self.meas = np.vstack([self.meas, m[None, :]])
        self.info = np.vstack([self.info, u[None, :]])
        self.edge_level = np.append(self.edge_level, np.int32(level))
        if kind or self.edge_kind is not None:
            self.edge_kind = np.append(ek, np.uint8(kind))
        return self.n_edges - 1

    @property
    def n_vertices(self):
        return self.poses.shape[0]

    @property
    def n_edges(self):
        return len(self.edge_from)

    @classmethod
    def from_synth(cls, g):
        return cls(g["ids"], g["poses"], g["fixed"], g["edge_from"], g["edge_to"], g["meas"], g["info"])

    def level0(self):
        """Arrays of the edges g2o's initializeOptimization() would activate (level 0)."""
        m = self.edge_level == 0
        return self.edge_from[m], self.edge_to[m], self.meas[m], self.info[m]

    # ---------------------------------------------------------------- .g2o text format
    def save_g2o(self, path, precision=None):
        """VERTEX_SE2 (+ ROBOTLASER1 data) / FIX / EDGE_SE2 lines, and for a typed graph VERTEX_XY, EDGE_SE2_XY,
        EDGE_BEARING_SE2_XY, EDGE_PRIOR_SE2 and EDGE_PRIOR_SE2_XY; a mixture edge as ``EDGE_SE2_MIXTURE from to K`` followed by K groups
        ``w x y th I11 I12 I13 I22 I23 I33`` (an edge of another kind: its own line, then ``MIXTURE_COMPONENTS K`` and the
        groups; the project's own tags).  ``precision=None`` reproduces g2o's default ostream precision (6 significant
        digits, lossy -- SURVEY.md section 5); pass 17 for round trips."""
        fmt = "%g" if precision is None else f"%.{precision}g"
        vk, ek = self.kinds()
        with open(path, "w") as f:
            for k in range(self.n_vertices):
                x, y, t = self.poses[k]
                if vk[k] == 1:
                    f.write(f"VERTEX_XY {int(self.ids[k])} {fmt % x} {fmt % y}\n")
                else:
                    f.write(f"VERTEX_SE2 {int(self.ids[k])} {fmt % x} {fmt % y} {fmt % t}\n")
                if k in self.lasers:
                    f.write(self.lasers[k].write(fmt) + "\n")      # saveUserData: the data lines follow their vertex
                if self.fixed[k]:
                    f.write(f"FIX {int(self.ids[k])}\n")
            for k in range(self.n_edges):
                if self.edge_level[k] != 0:
                    continue                      # only level-0 edges are saved by default
                m = self.meas[k]
                i = self.info[k]
                if k in self.mixtures:
                    # the project's own tags (no claim of compatibility with vertigo's): K groups of weight, the three
                    # measurement values and the six information values of the padded layout.  An EDGE_SE2 becomes one
                    # EDGE_SE2_MIXTURE line; an edge of another kind keeps its line (component 0) and a MIXTURE_COMPONENTS
                    # line follows it
                    mz, mu, mw = self.mixtures[k]
                    groups = " ".join(fmt % v for c in range(len(mw)) for v in (mw[c], *(m if c == 0 else mz[c]), *(i if c == 0 else mu[c])))
                    if ek[k] == 0:
                        f.write("EDGE_SE2_MIXTURE %d %d %d " % (self.ids[self.edge_from[k]], self.ids[self.edge_to[k]], len(mw))
                                + groups + "\n")
                        continue
                    tail = "MIXTURE_COMPONENTS %d " % len(mw) + groups + "\n"
                else:
                    tail = ""
                if ek[k] == 1:
                    f.write("EDGE_SE2_XY %d %d " % (self.ids[self.edge_from[k]], self.ids[self.edge_to[k]])
                            + " ".join(fmt % v for v in (*m[:2], i[0], i[1], i[3])) + "\n" + tail)
                    continue
                if ek[k] == 2:
                    f.write("EDGE_BEARING_SE2_XY %d %d " % (self.ids[self.edge_from[k]], self.ids[self.edge_to[k]])
                            + " ".join(fmt % v for v in (m[0], i[0])) + "\n" + tail)
                    continue
                if ek[k] == 3:
                    f.write("EDGE_PRIOR_SE2 %d " % self.ids[self.edge_from[k]] + " ".join(fmt % v for v in (*m, *i)) + "\n" + tail)
                    continue
                if ek[k] == 4:
                    f.write("EDGE_PRIOR_SE2_XY %d " % self.ids[self.edge_from[k]]
                            + " ".join(fmt % v for v in (*m[:2], i[0], i[1], i[3])) + "\n" + tail)
                    continue
                f.write("EDGE_SE2 %d %d " % (self.ids[self.edge_from[k]], self.ids[self.edge_to[k]])
                        + " ".join(fmt % v for v in (*m, *i)) + "\n")

    @classmethod
    def load_g2o(cls, path):
        ids, poses, fixed_ids, ef, et, meas, info = [], [], set(), [], [], [], []
        vkind, ekind = [], []     # typed graphs: VERTEX_XY, EDGE_SE2_XY, EDGE_BEARING_SE2_XY, EDGE_PRIOR_SE2, EDGE_PRIOR_SE2_XY
        lasers = {}               # vertex id -> RobotLaser
        mixtures = {}             # edge index -> (meas [K, 3], info [K, 6], weight [K]): EDGE_SE2_MIXTURE / MIXTURE_COMPONENTS

        def info2(t):             # I11 I12 I22 in the 3x3 upper-triangle layout
            a, b, c = (float(v) for v in t)
            return [a, b, 0.0, c, 0.0, 0.0]
        with open(path) as f:
            for line in f:
                tok = line.split()
                if not tok:
                    continue
                if tok[0] == "VERTEX_SE2":
                    ids.append(int(tok[1]))
                    poses.append([float(v) for v in tok[2:5]])
                    vkind.append(0)
                elif tok[0] == "VERTEX_XY":
                    ids.append(int(tok[1]))
                    poses.append([float(tok[2]), float(tok[3]), 0.0])
                    vkind.append(1)
                elif tok[0] == "FIX":
                    fixed_ids.update(int(v) for v in tok[1:])
                elif tok[0] == "EDGE_SE2":
                    ef.append(int(tok[1]))
                    et.append(int(tok[2]))
                    meas.append([float(v) for v in tok[3:6]])
                    info.append([float(v) for v in tok[6:12]])
                    ekind.append(0)
                elif tok[0] == "EDGE_SE2_XY":
                    ef.append(int(tok[1]))
                    et.append(int(tok[2]))
                    meas.append([float(tok[3]), float(tok[4]), 0.0])
                    info.append(info2(tok[5:8]))
                    ekind.append(1)
                elif tok[0] == "EDGE_BEARING_SE2_XY":
                    ef.append(int(tok[1]))
                    et.append(int(tok[2]))
                    meas.append([float(tok[3]), 0.0, 0.0])
                    info.append([float(tok[4]), 0.0, 0.0, 0.0, 0.0, 0.0])
                    ekind.append(2)
                elif tok[0] == "EDGE_PRIOR_SE2":
                    ef.append(int(tok[1]))
                    et.append(int(tok[1]))
                    meas.append([float(v) for v in tok[2:5]])
                    info.append([float(v) for v in tok[5:11]])
                    ekind.append(3)
                elif tok[0] == "EDGE_PRIOR_SE2_XY":
                    ef.append(int(tok[1]))
                    et.append(int(tok[1]))
                    meas.append([float(tok[2]), float(tok[3]), 0.0])
                    info.append(info2(tok[4:7]))
                    ekind.append(4)
                elif tok[0] == "EDGE_SE2_MIXTURE":
                    K = int(tok[3])
                    v = np.array([float(x) for x in tok[4:4 + 10 * K]]).reshape(K, 10)
                    ef.append(int(tok[1]))
                    et.append(int(tok[2]))
                    meas.append(list(v[0, 1:4]))
                    info.append(list(v[0, 4:10]))
                    ekind.append(0)
                    if K > 1:
                        mixtures[len(ef) - 1] = (v[:, 1:4].copy(), v[:, 4:10].copy(), v[:, 0].copy())
                elif tok[0] == "MIXTURE_COMPONENTS" and ef:
                    K = int(tok[1])
                    v = np.array([float(x) for x in tok[2:2 + 10 * K]]).reshape(K, 10)
                    if K > 1:
                        mixtures[len(ef) - 1] = (v[:, 1:4].copy(), v[:, 4:10].copy(), v[:, 0].copy())
                elif tok[0] == "ROBOTLASER1" and ids:
                    lasers[ids[-1]] = RobotLaser.read(tok)     # data lines belong to the preceding vertex
        ids = np.asarray(ids, dtype=np.int64)
        order = np.argsort(ids, kind="stable")          # g2o keeps vertices in an id-ordered map
        ids = ids[order]
        poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)[order]
        index = {int(v): k for k, v in enumerate(ids)}
        fixed = np.array([1 if int(v) in fixed_ids else 0 for v in ids], dtype=np.uint8)
        efi = np.array([index[v] for v in ef], dtype=np.int32)
        eti = np.array([index[v] for v in et], dtype=np.int32)
        g = cls(ids, poses, fixed, efi, eti, np.asarray(meas).reshape(-1, 3), np.asarray(info).reshape(-1, 6))
        if any(vkind) or any(ekind):
            g.vertex_kind = np.asarray(vkind, dtype=np.uint8)[order]
            g.edge_kind = np.asarray(ekind, dtype=np.uint8)
        g.lasers = {index[v]: l for v, l in lasers.items()}
        g.mixtures = mixtures
        return g


class GraphSLAM:
    """The optimiser face of the reference's ``GraphSLAM`` (src/slam/graph_slam.h:49-76)."""

    def __init__(self, graph: PoseGraph, ctx: Context | None = None, device: int = 0, algorithm: str = "gn",
                 lm_params: dict | None = None, dl_params: dict | None = None):
        """``algorithm``: "gn" (the reference's Gauss-Newton), "levenberg" (g2o's OptimizationAlgorithmLevenberg, with
        ``lm_params``: tau, initial_lambda, max_trials, good_step_lower, good_step_upper) or "dl" (g2o's
        OptimizationAlgorithmDogleg, the factory's "dl_var", with ``dl_params``: initial_delta, max_trials, initial_lambda,
        lambda_factor)."""
        if algorithm == "levenberg":
            pass
        elif algorithm == "dl":
            dl_params_checked(dl_params or {})
        elif algorithm != "gn":
            raise ValueError(f"algorithm must be 'gn', 'levenberg' or 'dl', not {algorithm!r}")
        self.graph = graph
        self.ctx = ctx or Context(device)
        self.algorithm = algorithm
        self.lm_params = dict(lm_params or {})
        self.dl_params = dict(dl_params or {})
        self.last_deltas = None
        self.last_steps = None
        self.last_chi2 = None
        self.last_status = 0
        self.last_lambdas = None
        self.last_trials = None
        self.last_iterations = 0
        # robust kernels per edge of the graph (setRobustKernel): C codes and deltas, None while none is set
        self._rk_kind = None
        self._rk_delta = None
        self.last_edge_chi2 = None
        self.last_weights = None
        self.last_mu = None
        self._gnc_rejected = None
        self.last_init_counts = None
        self.last_selected = None

    def optimize(self, nrunnings: int) -> None:
        """``nrunnings`` iterations on the level-0 edges; estimates updated in place.  Returns nothing and never raises on
        a Cholesky failure, like the reference.  With "levenberg" the call may terminate early: ``last_iterations`` holds
        the iterations run (g2o's SparseOptimizer::optimize return value)."""
        g = self.graph
        ef, et, meas, info = g.level0()
        rk = self._robust_level0()
        self.last_edge_chi2 = self.last_weights = None
        ty = self._typed_level0()
        mix = g.mixture_arrays()
        if mix is not None:
            # max-mixture edges: the mixture entry points, under every algorithm; no robust kernel beside them
            if rk is not None:
                raise ValueError("optimize: a graph with mixture edges takes no robust kernel (clearRobustKernels, or collapseMixtures)")
            a = (g.poses, g.fixed, ef, et, meas, info, int(nrunnings), mix)
            kw = {} if ty is None else dict(vertex_kind=ty[0], edge_kind=ty[1])
            if self.algorithm == "levenberg":
                rc, poses, chi2, lam, tri, done, sel = self.ctx.lm_optimize_mixture(*a, **kw, **self.lm_params)
                self.last_lambdas, self.last_trials, self.last_iterations = lam[:done], tri[:done], done
            elif self.algorithm == "dl":
                rc, poses, chi2, dlt, tri, stp, done, sel = self.ctx.dl_optimize_mixture(*a, **kw, raise_on_fail=False, **self.dl_params)
                self.last_deltas, self.last_trials, self.last_steps = dlt[:done], tri[:done], stp[:done]
                self.last_iterations = done if rc == 0 else 0
            else:
                rc, poses, chi2, sel = self.ctx.gn_optimize_mixture(*a, **kw, raise_on_cholesky=False)
                self.last_iterations = int(nrunnings) if rc == 0 else CGMR_E_CHOLESKY_BASE - rc
            self.last_selected = sel
        elif ty is not None:
            # landmarks / priors: the typed entry points (the same records; e2 and weights behind them with a kernel set)
            a = (g.poses, g.fixed, ef, et, meas, info, int(nrunnings))
            kw = dict(vertex_kind=ty[0], edge_kind=ty[1], **({} if rk is None else dict(kind=rk[0], delta=rk[1])))
            if self.algorithm == "levenberg":
                out = self.ctx.lm_optimize_typed(*a, **kw, **self.lm_params)
                rc, poses, chi2, lam, tri, done = out[:6]
                self.last_lambdas, self.last_trials, self.last_iterations = lam[:done], tri[:done], done
            elif self.algorithm == "dl":
                out = self.ctx.dl_optimize_typed(*a, **kw, raise_on_fail=False, **self.dl_params)
                rc, poses, chi2, dlt, tri, stp, done = out[:7]
                self.last_deltas, self.last_trials, self.last_steps = dlt[:done], tri[:done], stp[:done]
                self.last_iterations = done if rc == 0 else 0
            else:
                out = self.ctx.gn_optimize_typed(*a, **kw, raise_on_cholesky=False)
                rc, poses, chi2 = out[:3]
                self.last_iterations = int(nrunnings) if rc == 0 else CGMR_E_CHOLESKY_BASE - rc
            if rk is not None:
                self.last_edge_chi2, self.last_weights = out[-2:]
        elif self.algorithm == "levenberg":
            if rk is None:
                rc, poses, chi2, lam, tri, done = self.ctx.lm_optimize(g.poses, g.fixed, ef, et, meas, info, int(nrunnings),
                                                                       **self.lm_params)
            else:
                rc, poses, chi2, lam, tri, done, self.last_edge_chi2, self.last_weights = self.ctx.lm_optimize_robust(
                    g.poses, g.fixed, ef, et, meas, info, int(nrunnings), *rk, **self.lm_params)
            self.last_lambdas, self.last_trials, self.last_iterations = lam[:done], tri[:done], done
        elif self.algorithm == "dl":
            out = self.ctx.dl_optimize(g.poses, g.fixed, ef, et, meas, info, int(nrunnings), *(rk or (None,)),
                                       raise_on_fail=False, **self.dl_params)
            rc, poses, chi2, dlt, tri, stp, done = out[:7]
            if rk is not None:
                self.last_edge_chi2, self.last_weights = out[7:]
            self.last_deltas, self.last_trials, self.last_steps = dlt[:done], tri[:done], stp[:done]
            self.last_iterations = done if rc == 0 else 0          # (g2o's optimize() returns 0 after Fail)
        else:
            if rk is None:
                rc, poses, chi2 = self.ctx.gn_optimize(g.poses, g.fixed, ef, et, meas, info, int(nrunnings),
                                                       raise_on_cholesky=False)
            else:
                rc, poses, chi2, self.last_edge_chi2, self.last_weights = self.ctx.gn_optimize_robust(
                    g.poses, g.fixed, ef, et, meas, info, int(nrunnings), *rk, raise_on_cholesky=False)
            self.last_iterations = int(nrunnings) if rc == 0 else CGMR_E_CHOLESKY_BASE - rc
        g.poses[:] = poses
        self.last_chi2 = chi2
        self.last_status = rc

    # ---------------------------------------------------------------- starting points
    def initializeChordal(self, stages="rt") -> None:     # noqa: N802
        """A starting point by chordal relaxation (Context.chordal_initialize) on the level-0 edges, whatever the estimates
        are: ``stages`` "r" the headings, "t" the positions with the headings held, "rt" both.  A typed graph goes through its
        kinds; robust kernels play no part (the method is not robust to wrong closures).  Estimates updated in place.  Leaves
        ``last_chi2`` (the SE(2) chi2 at the start and at the result), ``last_status`` and ``last_init_counts`` (vertices solved
        in the rotation stage, in the translation stage, degenerate headings); never raises on a Cholesky failure."""
        g = self.graph
        ef, et, meas, info = g.level0()
        ty = self._typed_level0()
        kw = {} if ty is None else dict(vertex_kind=ty[0], edge_kind=ty[1])
        out = self.ctx.chordal_initialize(g.poses, g.fixed, ef, et, meas, info, stages, raise_on_cholesky=False, **kw)
        g.poses[:] = out["poses"]
        self.last_chi2, self.last_status, self.last_init_counts = out["chi2"], out["status"], out["counts"]

    def computeInitialGuess(self) -> None:     # noqa: N802
        """g2o's spanning-tree guess (Context.initial_guess) over the level-0 edges of a pose graph, from the fixed vertices;
        estimates updated in place."""
        g = self.graph
        if g.typed:
            raise ValueError("computeInitialGuess: pose graphs only (a landmark observation is no SE(2) transform)")
        ef, et, meas, _ = g.level0()
        g.poses[:] = self.ctx.initial_guess(g.poses, g.fixed, ef, et, meas)

    # ---------------------------------------------------------------- graduated non-convexity
    def optimizeGNC(self, max_outer: int = 100, loss: str = "tls", barc_sq=None, known_inliers=None, **params) -> None:     # noqa: N802
        """Outlier rejection by graduated non-convexity (Context.gnc_optimize) on the level-0 edges, from the estimates as they
        stand; estimates updated in place.  ``loss``: "tls" or "gm"; ``barc_sq``: a scalar, an array over the graph's edges or
        None (the chi2 0.99 quantile of each factor's dimension); ``known_inliers``: indices of the graph's edges or a mask
        over them, None for none; ``params``: mu_factor, inner_iters, outer_per_wait.  A typed graph goes through its kinds;
        robust kernels set with setRobustKernel play no part.  Leaves ``last_weights`` and ``last_edge_chi2`` (over the
        level-0 edges), ``last_mu``, ``last_chi2`` (the cost record, [outer iterations run + 1]), ``last_iterations`` (outer
        iterations run) and ``last_status``; never raises on a Cholesky failure."""
        from ._lib import gnc_known_mask
        g = self.graph
        if g.mixture_arrays() is not None:
            raise ValueError("optimizeGNC: not offered on a graph with mixture edges (collapseMixtures first)")
        m = g.edge_level == 0
        ef, et, meas, info = g.level0()
        ty = self._typed_level0()
        kw = {} if ty is None else dict(vertex_kind=ty[0], edge_kind=ty[1])
        c = barc_sq if barc_sq is None or np.ndim(barc_sq) == 0 else np.asarray(barc_sq, dtype=np.float64).reshape(-1)[m]
        known = None if known_inliers is None else gnc_known_mask(known_inliers, g.n_edges)[m]
        out = self.ctx.gnc_optimize(g.poses, g.fixed, ef, et, meas, info, int(max_outer), loss, c, known, raise_on_cholesky=False,
                                    **kw, **params)
        done = out["outer_done"]
        g.poses[:] = out["poses"]
        self.last_weights, self.last_edge_chi2 = out["weights"], out["edge_chi2"]
        self.last_mu, self.last_chi2 = out["mu"][:done], out["cost"][:done + 1]
        self.last_iterations, self.last_status = done, out["status"]
        self._gnc_rejected = np.flatnonzero(m)[out["weights"] == 0.0] if str(loss).lower() in ("tls", "0") else np.zeros(0, np.int64)

    def rejectedEdges(self):     # noqa: N802
        """Indices (into the graph's edges) of the edges the last optimizeGNC call with the TLS loss gave weight 0."""
        if self._gnc_rejected is None:
            raise RuntimeError("rejectedEdges: call optimizeGNC first")
        return self._gnc_rejected.copy()

    # ---------------------------------------------------------------- max-mixture edges
    def addMixtureEdge(self, i, j, components, kind: int = 0) -> int:     # noqa: N802
        """An edge between the vertex indices ``i`` and ``j`` that is one of ``components`` = [(weight, meas, info), ...]; every
        linearisation keeps the most likely one at the current estimate (include/cgmr.h: cgmr_mixture).  Component 0 is what
        every call outside the mixture path sees of the edge.  Returns the edge index."""
        comps = list(components)
        if not comps:
            raise ValueError("addMixtureEdge: at least one component")
        k = self.graph.add_edge(i, j, comps[0][1], comps[0][2], kind=kind)
        self.graph.set_edge_mixture(k, comps)
        return k

    def setEdgeMixture(self, edge, components) -> None:     # noqa: N802
        """Replace edge ``edge``'s measurement by the mixture ``components`` = [(weight, meas, info), ...] (one: a plain edge)."""
        self.graph.set_edge_mixture(edge, components)

    def addNullHypothesis(self, edges, weight: float = 1.0, scale: float = 1e-2) -> None:     # noqa: N802
        """Give each of the graph's edges ``edges`` a second component with the same measurement and ``scale`` times its
        information, weights (1, ``weight``): outlier rejection without a schedule.  An edge that is a mixture already gains
        the component behind its own."""
        if not (np.isfinite(weight) and weight > 0 and np.isfinite(scale) and scale > 0):
            raise ValueError("addNullHypothesis: weight and scale must be finite and > 0")
        g = self.graph
        for k in np.asarray(edges, dtype=np.int64).reshape(-1):
            k = int(k)
            if not 0 <= k < g.n_edges:
                raise ValueError(f"edge index out of range 0..{g.n_edges - 1}")
            mz, mu, mw = g.mixtures.get(k, (g.meas[k][None, :], g.info[k][None, :], np.ones(1)))
            g.mixtures[k] = (np.vstack([mz, g.meas[k][None, :]]), np.vstack([mu, scale * g.info[k][None, :]]),
                             np.append(mw, float(weight)))

    def _mixture_select(self):
        g = self.graph
        ty = self._typed_level0()
        kw = {} if ty is None else dict(vertex_kind=ty[0], edge_kind=ty[1])
        return self.ctx.mixture_select(g.poses, g.fixed, *g.level0(), g.mixture_arrays(), **kw)

    def selectedComponents(self):     # noqa: N802
        """The selected component of every level-0 edge (level0() order) at the current estimates; zeros without mixtures."""
        return self._mixture_select()[1]

    def mixtureChi2(self) -> float:     # noqa: N802
        """The mixture cost at the current estimates: the sum over the level-0 edges of min_k (r_k + c_k); chi2() without
        mixtures.  chi2() itself stays the plain chi2 of every edge's component 0."""
        return self._mixture_select()[0]

    def collapseMixtures(self) -> PoseGraph:     # noqa: N802
        """A new PoseGraph without mixtures: every level-0 mixture edge takes its selected (z, Omega) at the current estimates,
        every other mixture edge its component 0.  The supported route to marginals and condensed graphs."""
        g = self.graph
        sel = self.selectedComponents()
        out = PoseGraph(g.ids, g.poses, g.fixed, g.edge_from, g.edge_to, g.meas.copy(), g.info.copy(), g.edge_level.copy(),
                        g.vertex_kind, g.edge_kind)
        out.lasers = dict(g.lasers)
        for pos, k in enumerate(np.flatnonzero(g.edge_level == 0)):
            if int(k) in g.mixtures and sel[pos] > 0:
                mz, mu, _ = g.mixtures[int(k)]
                out.meas[k], out.info[k] = mz[sel[pos]], mu[sel[pos]]
        return out

    # ---------------------------------------------------------------- landmarks and priors (g2o's slam2d types)
    def _typed_level0(self):
        """(vertex kinds, kinds of the level-0 edges), or None for a pure pose graph (the plain path)."""
        g = self.graph
        if not g.typed:
            return None
        vk, ek = g.kinds()
        return vk, ek[g.edge_level == 0]

    def addLandmark(self, vid, xy, fixed: bool = False) -> int:     # noqa: N802
        """A VertexPointXY with id ``vid`` at ``xy``; returns its vertex index."""
        return self.graph.add_vertex(vid, xy, kind=1, fixed=fixed)

    def addObservation(self, pose_idx, landmark_idx, z_xy, info) -> int:     # noqa: N802
        """An EdgeSE2PointXY: the point seen at ``z_xy`` in the pose's frame; ``info`` = (I11, I12, I22).  Returns the edge index."""
        return self.graph.add_edge(pose_idx, landmark_idx, z_xy, info, kind=1)

    def addBearing(self, pose_idx, landmark_idx, z, info) -> int:     # noqa: N802
        """An EdgeSE2PointXYBearing: the point seen under the angle ``z`` in the pose's frame, with the scalar information
        ``info``.  Returns the edge index."""
        return self.graph.add_edge(pose_idx, landmark_idx, [float(z)], [float(info)], kind=2)

    def addPrior(self, pose_idx, z_xyt, info) -> int:     # noqa: N802
        """An EdgeSE2Prior on a pose; ``info`` = the 6 upper-triangle values.  Returns the edge index."""
        return self.graph.add_edge(pose_idx, pose_idx, z_xyt, info, kind=3)

    def addPositionPrior(self, pose_idx, z_xy, info) -> int:     # noqa: N802
        """An EdgeSE2XYPrior (a GPS / UWB fix) on a pose; ``info`` = (I11, I12, I22).  Returns the edge index."""
        return self.graph.add_edge(pose_idx, pose_idx, z_xy, info, kind=4)

    # ---------------------------------------------------------------- robust kernels (g2o's edge->setRobustKernel)
    def setRobustKernel(self, name, delta: float = 1.0, edges=None) -> None:     # noqa: N802 (g2o spelling)
        """``edge->setRobustKernel(new RobustKernel<name>); kernel->setDelta(delta)`` for the graph's edges ``edges`` (indices
        into its edge list; None: every level-0 edge).  ``name``: "Huber", "PseudoHuber", "Cauchy", "Welsch", "Tukey",
        "Saturated", "DCS" (delta = phi) or "none"; anything else, or a delta that is not finite and > 0, raises
        ValueError.  optimize() then minimises the robust chi2; chi2() stays the plain one (g2o's activeChi2)."""
        code = robust_code(name)
        n = self.graph.n_edges
        idx = np.flatnonzero(self.graph.edge_level == 0) if edges is None else np.asarray(edges, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= n):
            raise ValueError(f"edge index out of range 0..{n - 1}")
        robust_arrays(code, delta, idx.size)                       # (the delta's check)
        self._grow_robust()
        self._rk_kind[idx] = code
        self._rk_delta[idx] = float(delta) if code else 1.0

    def clearRobustKernels(self) -> None:     # noqa: N802
        """Every edge back to no robust kernel."""
        self._rk_kind = self._rk_delta = None

    def edgeWeights(self):     # noqa: N802
        """rho1 of every level-0 edge (level0() order) at the estimate the last optimize() returned; None when that ran with
        no robust kernel set."""
        return self.last_weights

    def robustChi2(self) -> float:     # noqa: N802
        """g2o's activeRobustChi2 at the current estimates: the sum of rho0 over the level-0 edges (chi2() with no kernel)."""
        g = self.graph
        ef, et, meas, info = g.level0()
        rk = self._robust_level0()
        if rk is None:
            return self.chi2()
        ty = self._typed_level0()
        if ty is not None:
            return float(self.ctx.gn_optimize_typed(g.poses, g.fixed, ef, et, meas, info, 0, ty[0], ty[1], rk[0], rk[1])[2][0])
        _, _, chi2, _, _ = self.ctx.gn_optimize_robust(g.poses, g.fixed, ef, et, meas, info, 0, *rk)
        return float(chi2[0])

    def _grow_robust(self):
        n = self.graph.n_edges
        if self._rk_kind is None:
            self._rk_kind, self._rk_delta = np.zeros(n, dtype=np.uint8), np.ones(n)
        elif len(self._rk_kind) != n:                              # (edges added since: no kernel; a graph loaded since: its own)
            m = min(len(self._rk_kind), n)
            self._rk_kind = np.concatenate([self._rk_kind[:m], np.zeros(n - m, dtype=np.uint8)])
            self._rk_delta = np.concatenate([self._rk_delta[:m], np.ones(n - m)])

    def _robust_level0(self):
        """(kinds, deltas) of the level-0 edges, or None when no edge has a kernel (the plain path)."""
        if self._rk_kind is None or not self._rk_kind.any():
            return None
        self._grow_robust()
        m = self.graph.edge_level == 0
        return self._rk_kind[m], self._rk_delta[m]

    def trustRegion(self) -> float:     # noqa: N802 (g2o spelling)
        """OptimizationAlgorithmDogleg::trustRegion: delta after the last iteration of the last optimize (the initial delta
        before any dogleg iteration)."""
        if self.last_deltas is None or len(self.last_deltas) == 0:
            return float(self.dl_params.get("initial_delta", DL_DEFAULTS["initial_delta"]))
        return float(self.last_deltas[-1])

    def lastStep(self) -> int:     # noqa: N802 (g2o spelling)
        """OptimizationAlgorithmDogleg::lastStep: the kind of the last trial's step, 1 SD, 2 GN, 3 DL (DL_STEP_*; 0 before
        any dogleg iteration)."""
        if self.last_steps is None or len(self.last_steps) == 0:
            return 0
        return int(self.last_steps[-1])

    def currentLambda(self) -> float:     # noqa: N802 (g2o spelling)
        """OptimizationAlgorithmLevenberg::currentLambda: lambda after the last iteration of the last optimize (0 before
        any Levenberg iteration)."""
        if self.last_lambdas is None or len(self.last_lambdas) == 0:
            return 0.0
        return float(self.last_lambdas[-1])

    def levenbergIterations(self) -> int:     # noqa: N802 (g2o spelling)
        """OptimizationAlgorithmLevenberg::levenbergIteration: trials of the last iteration of the last optimize."""
        if self.last_trials is None or len(self.last_trials) == 0:
            return 0
        return int(self.last_trials[-1])

    def computeMarginals(self, cross: bool = False, robust: bool = False):     # noqa: N802 (g2o spelling)
        """SparseOptimizer::computeMarginals over every vertex, on the level-0 edges at the current estimates:
        ``cov[nV, 3, 3]``, or ``(cov, cross[nE0, 3, 3])`` with ``cross=True`` (the block of each level-0 edge, rows the
        from vertex, columns the to vertex).  Fixed vertices and their edges get zeros.  ``robust=True``: H with the kernels of
        setRobustKernel, every edge's information scaled by rho1 at the current estimates (g2o inverts the H of the last
        buildSystem, robust weights included); with no kernel set, the plain result."""
        g = self.graph
        ef, et, meas, info = g.level0()
        rk = self._robust_level0() if robust else None
        ty = self._typed_level0()
        if ty is not None:
            kw = {} if rk is None else dict(kind=rk[0], delta=rk[1])
            out = self.ctx.marginals_all_typed(g.poses, g.fixed, ef, et, meas, info, cross, ty[0], ty[1], **kw)
            return out[:2] if cross else (out if rk is None else out[0])
        if rk is None:
            return self.ctx.marginals_all(g.poses, g.fixed, ef, et, meas, info, cross=cross)
        out = self.ctx.marginals_all_robust(g.poses, g.fixed, ef, et, meas, info, cross, *rk)
        return out[:2] if cross else out[0]

    def _joint_args(self, robust):
        """The level-0 problem at the current estimates, the robust and the typed arguments of the joint / pairwise marginals
        calls (a typed graph: the kinds, and with them the typed entry points), and whether the call returns statistics."""
        g = self.graph
        rk = self._robust_level0() if robust else None
        kw = {} if rk is None else dict(kind=rk[0], delta=rk[1])
        ty = self._typed_level0()
        if ty is not None:
            kw.update(vertex_kind=ty[0], edge_kind=ty[1])
        return (g.poses, g.fixed, *g.level0()), kw, rk is not None

    def computeMarginalBlocks(self, blockIndices, robust: bool = False):     # noqa: N802, N803 (g2o spelling)
        """SparseOptimizer::computeMarginals(spinv, blockIndices): the 3x3 blocks Sigma_ij of H^-1 for arbitrary vertex index
        pairs ``(i, j)`` -- adjacent or not --, on the level-0 edges at the current estimates as computeMarginals.  Returns
        ``{(i, j): 3x3}``, rows indexing i.  ``robust`` as for computeMarginals."""
        pairs = [(int(i), int(j)) for i, j in blockIndices]
        if not pairs:
            return {}
        a, kw, _ = self._joint_args(robust)
        ab = self.ctx.marginals_pairs(*a, [p[0] for p in pairs], [p[1] for p in pairs], **kw)[1]
        return {p: ab[k].copy() for k, p in enumerate(pairs)}

    def jointMarginal(self, vertices, robust: bool = False):     # noqa: N802 (g2o spelling)
        """The joint covariance ``[3 n, 3 n]`` of the given vertex indices, in their order (the input of a Mahalanobis test on
        several poses at once, or of a condensed graph denser than a star)."""
        a, kw, stats = self._joint_args(robust)
        out = self.ctx.marginals_joint(*a, vertices, **kw)
        return out[0] if stats else out

    def condensedTree(self, vertices, gauge, robust: bool = False):     # noqa: N802 (g2o spelling)
        """The condensed graph over the given vertex indices as a spanning tree of relative poses rooted at ``gauge``
        (Context.condense_tree on the level-0 edges at the current estimates): ``(from_ids, to_ids, est [n, 3], info_upper
        [n, 6], weight [n], flags [n])``, the edges by vertex id -- what a peer receives as ordinary EdgeSE2.  ``robust`` as for
        computeMarginals.  A typed graph raises ValueError: condensed graphs are pose-only."""
        a, kw, _ = self._joint_args(robust)
        if "vertex_kind" in kw:
            raise ValueError("condensedTree: pose graphs only (the graph has landmarks or priors)")
        fr, to, est, iu, w, fl = self.ctx.condense_tree(a[0], *a[2:], int(gauge), vertices, **kw)[:6]
        ids = np.asarray(self.graph.ids)
        return ids[fr], ids[to], est, iu, w, fl

    def removeVertices(self, indices, max_degree: int = REMOVE_MAX_DEGREE):     # noqa: N802
        """Take the vertices ``indices`` out of the graph: each is marginalised out of the star of its level-0 edges and the
        star replaced by a spanning tree of relative-pose edges over its neighbours (Context.remove_nodes; the estimates are
        not an input).  The vertices and their edges are deleted, the new edges appended at level 0 without a robust kernel,
        and ``ids``, ``poses``, ``fixed``, ``lasers`` and the robust-kernel arrays compacted.

        One device call removes an independent set.  A request that is not one is worked off in rounds: each round takes, in
        index order, the requested vertices not adjacent in the *current* graph to one already taken this round, and its new
        edges join the graph before the next round -- so the result depends on this order.  A vertex with more than
        ``max_degree`` (at most 16) distinct neighbours when its round comes, or whose local system has no Cholesky factor,
        stays in the graph with its edges.

        Returns ``(index_map [old nV], new_edges, skipped)``: the new index of every old vertex (-1: removed), the indices of
        the new edges in the rewritten graph, and ``[(old vertex index, flag), ...]`` of the vertices left in place (flags as
        Context.remove_nodes).  Raises ValueError for an index out of range, a fixed vertex, a typed graph, a graph with
        mixtures, a vertex touched by an edge of another level, or a ``max_degree`` outside 1..16."""
        g = self.graph
        if g.typed:
            raise ValueError("removeVertices: pose graphs only (the graph has landmarks or priors)")
        if g.has_mixtures:
            raise ValueError("removeVertices: a graph with mixture edges (collapseMixtures first)")
        if not 1 <= int(max_degree) <= REMOVE_MAX_DEGREE:
            raise ValueError(f"removeVertices: max_degree must be 1..{REMOVE_MAX_DEGREE}")
        nV = g.n_vertices
        left = sorted(set(int(v) for v in np.asarray(indices, dtype=np.int64).reshape(-1)))
        if left and (left[0] < 0 or left[-1] >= nV):
            raise ValueError(f"removeVertices: vertex index out of range 0..{nV - 1}")
        if g.fixed[left].any():
            raise ValueError("removeVertices: a fixed vertex cannot be removed")
        other = g.edge_level != 0
        if np.isin(g.edge_from[other], left).any() or np.isin(g.edge_to[other], left).any():
            raise ValueError("removeVertices: a vertex is touched by an edge of another level")
        orig = np.flatnonzero(~other)                              # the level-0 edges at work: their old index, -1 for a new one
        ef, et, meas, info = (a.copy() for a in g.level0())
        skipped, removed = [], []
        while left:
            adj = {}
            for a, b in zip(ef.tolist(), et.tolist()):
                adj.setdefault(a, set()).add(b)
                adj.setdefault(b, set()).add(a)
            take, blocked = [], set()
            for v in left:
                if v not in blocked:
                    take.append(v)
                    blocked |= adj.get(v, set())
            call = [v for v in take if len(adj.get(v, ())) <= int(max_degree)]
            skipped += [(v, 2) for v in take if len(adj.get(v, ())) > int(max_degree)]
            _, fr, to, z, iu, _, fl = self.ctx.remove_nodes(ef, et, meas, info, call, num_vertices=nV)
            gone = [v for v, f in zip(call, fl) if f == 0]
            removed += gone
            skipped += [(v, int(f)) for v, f in zip(call, fl) if f != 0]
            keep = ~(np.isin(ef, gone) | np.isin(et, gone))
            ef, et = np.concatenate([ef[keep], fr]), np.concatenate([et[keep], to])
            meas, info = np.vstack([meas[keep], z]), np.vstack([info[keep], iu])
            orig = np.concatenate([orig[keep], np.full(len(fr), -1, dtype=orig.dtype)])
            taken = set(take)
            left = [v for v in left if v not in taken]
        # the rewritten graph: the old edges that stay, in their order, then the new ones; the vertices compacted
        stay_v = np.ones(nV, dtype=bool)
        stay_v[removed] = False
        index_map = np.full(nV, -1, dtype=np.int64)
        index_map[stay_v] = np.arange(int(stay_v.sum()))
        stay_e = other.copy()
        stay_e[orig[orig >= 0]] = True
        new = orig < 0
        n_new = int(new.sum())
        if self._rk_kind is not None:
            self._grow_robust()
            self._rk_kind = np.concatenate([self._rk_kind[stay_e], np.zeros(n_new, dtype=np.uint8)])
            self._rk_delta = np.concatenate([self._rk_delta[stay_e], np.ones(n_new)])
        if g.edge_kind is not None:
            g.edge_kind = np.concatenate([g.edge_kind[stay_e], np.zeros(n_new, dtype=np.uint8)])
        if g.vertex_kind is not None:
            g.vertex_kind = g.vertex_kind[stay_v]
        g.edge_from = np.concatenate([index_map[g.edge_from[stay_e]], index_map[ef[new]]]).astype(np.int32)
        g.edge_to = np.concatenate([index_map[g.edge_to[stay_e]], index_map[et[new]]]).astype(np.int32)
        g.meas = np.vstack([g.meas[stay_e], meas[new]])
        g.info = np.vstack([g.info[stay_e], info[new]])
        g.edge_level = np.concatenate([g.edge_level[stay_e], np.zeros(n_new, dtype=np.int32)])
        g.ids, g.poses, g.fixed = g.ids[stay_v], g.poses[stay_v].copy(), g.fixed[stay_v]
        g.lasers = {int(index_map[v]): l for v, l in g.lasers.items() if index_map[v] >= 0}
        # what the last optimize() left per edge no longer fits the edge list
        self.last_edge_chi2 = self.last_weights = self.last_selected = self._gnc_rejected = None
        return index_map, np.arange(g.n_edges - n_new, g.n_edges), skipped

    def _laser_map(self, who, **map_kw):
        """(vertex indices that carry a laser, in id order; the Graph2occupancy over them at the current estimates).  The scans
        must share one laser: beam count, first beam angle, angular step, maximum range, mounting pose."""
        from .occupancy import Graph2occupancy
        g = self.graph
        idx = np.array(sorted(g.lasers, key=lambda v: int(g.ids[v])), dtype=np.int64)
        if len(idx) == 0:
            raise ValueError(f"{who}: no vertex carries a laser scan")
        first = g.lasers[int(idx[0])]
        for v in idx[1:]:
            l = g.lasers[int(v)]
            if (len(l.ranges) != len(first.ranges) or (l.first_beam_angle, l.angular_step, l.max_range) !=
                    (first.first_beam_angle, first.angular_step, first.max_range) or not np.array_equal(l.laser_pose, first.laser_pose)):
                raise ValueError(f"{who}: the scans of vertices {int(idx[0])} and {int(v)} come from different lasers")
        scans = np.stack([g.lasers[int(v)].ranges for v in idx])
        occ = Graph2occupancy(self.ctx, g.poses[idx], scans, first.first_beam_angle, first.angular_step, first.max_range,
                              laser_pose=first.laser_pose, fixed=g.fixed[idx], **map_kw)
        return idx, occ

    def scanInformation(self, **map_kw):     # noqa: N802
        """``(vertex indices with a laser, dH [n])``: for every key frame the entropy, in nats, the occupancy map of all of them
        gains if its scan is dropped (Graph2occupancy.scanInformation at the current estimates; ``map_kw``: Graph2occupancy's
        keywords -- resolution, usableRange, ...).  The higher, the more the map owes to the scan."""
        idx, occ = self._laser_map("scanInformation", **map_kw)
        return idx, occ.scanInformation()["delta"]

    def pruneScans(self, max_remove, max_entropy_increase: float = -1.0, keep=(), **map_kw):     # noqa: N802
        """Choose up to ``max_remove`` key frames by what their scans tell the occupancy map and take them out of the graph.
        The greedy selection (Graph2occupancy.pruneScans at the current estimates) drops, one at a time, the scan whose loss
        raises the map's entropy least, while the sum of the increases stays within ``max_entropy_increase`` (negative: no
        budget).  Fixed vertices and ``keep`` are never chosen; a vertex without a laser is not a candidate.  The chosen
        vertices go to ``removeVertices``.

        Returns ``(index_map, new_edges, skipped, order, delta)``: ``removeVertices``' result -- ``skipped`` lists the chosen
        vertices it left in place, with their flags -- then the chosen vertices as old indices in the order chosen, and the
        entropy increase of each.  Raises as ``removeVertices`` does (typed graphs, mixtures), before anything is selected."""
        g = self.graph
        if g.typed:
            raise ValueError("pruneScans: pose graphs only (the graph has landmarks or priors)")
        if g.has_mixtures:
            raise ValueError("pruneScans: a graph with mixture edges (collapseMixtures first)")
        idx, occ = self._laser_map("pruneScans", **map_kw)
        keep = np.asarray(keep, dtype=np.int64).reshape(-1)
        if len(keep) and (keep.min() < 0 or keep.max() >= g.n_vertices):
            raise ValueError(f"pruneScans: keep: vertex index out of range 0..{g.n_vertices - 1}")
        protected = np.asarray(g.fixed[idx]).astype(bool) | np.isin(idx, keep)
        res = occ.pruneScans(max_remove, max_entropy_increase, protected)
        order = idx[res["order"]]
        return self.removeVertices(order) + (order, res["delta"])

    def relativeCovariance(self, pairs, hypotheses=None, robust: bool = False):     # noqa: N802 (g2o spelling)
        """For the vertex index pairs ``(a, b)``: ``(z [n, 3], Sigma_z [n, 3, 3])``, z = x_a^-1 x_b and its covariance, without
        re-gauging the graph per pair.  ``hypotheses`` = ``(meas [n, 3], info_upper [n, 6] or None)``: a candidate measurement
        per pair; then ``(z, Sigma_z, d2 [n])`` with the squared Mahalanobis distance a closure is gated on."""
        pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        a, kw, _ = self._joint_args(robust)
        hm, hi = (None, None) if hypotheses is None else hypotheses
        if "vertex_kind" in kw:                                    # a typed graph: the same launch behind the typed check
            z, cz, d2 = self.ctx.observation_covariance(*a, pairs[:, 0], pairs[:, 1], None, hm, hi, **kw)[:3]
        else:
            z, cz, d2 = self.ctx.relative_covariance(*a, pairs[:, 0], pairs[:, 1], hm, hi, **kw)[:3]
        return (z, cz) if hypotheses is None else (z, cz, d2)

    def closureConsistency(self, closures, gamma, robust: bool = False, exact: bool = False, node_limit=None):     # noqa: N802
        """Pairwise consistency maximisation over closure candidates that are not (yet) edges: ``closures`` a list of
        ``(i, j, meas, info_upper)`` on vertex indices.  Returns ``(d2 [N, N], adj [N, N] bool, clique, seed)`` as
        Context.closure_consistency does, on the level-0 edges at the current estimates (as relativeCovariance).  The clique is
        the greedy heuristic's, not an exact maximum.  ``exact``: ``(d2, adj, clique, proven)`` as
        Context.closure_consistency_exact does, the clique a maximum one when ``proven`` (every root's search stays within
        ``node_limit`` nodes; None: the binding's default), else the best found and no smaller than the greedy one.  A typed
        graph raises ValueError: pose graphs only."""
        a, kw, _ = self._joint_args(robust)
        if "vertex_kind" in kw:
            raise ValueError("closureConsistency: pose graphs only (the graph has landmarks or priors)")
        cl = list(closures)
        ca = np.array([c[0] for c in cl], dtype=np.int32)
        cb = np.array([c[1] for c in cl], dtype=np.int32)
        cm = np.array([c[2] for c in cl], dtype=np.float64).reshape(len(cl), 3)
        ci = np.array([c[3] for c in cl], dtype=np.float64).reshape(len(cl), 6)
        if exact:
            if node_limit is not None:
                kw = dict(kw, node_limit=node_limit)
            return self.ctx.closure_consistency_exact(*a, ca, cb, cm, ci, gamma, **kw)[:4]
        return self.ctx.closure_consistency(*a, ca, cb, cm, ci, gamma, **kw)[:4]

    # the default gamma: the 0.99 quantile of chi2 with 3 degrees of freedom (scipy.stats.chi2.ppf(0.99, 3)) -- two candidates
    # that both agree with the graph fail the test together once in a hundred
    GAMMA_99 = 11.344866730144373

    def consistentClosures(self, closures, gamma: float = GAMMA_99, robust: bool = False, exact: bool = False):     # noqa: N802
        """The indices (ascending) of the largest set of pairwise consistent candidates closureConsistency finds (``exact``: by
        the exact search, at its default node limit)."""
        return self.closureConsistency(closures, gamma, robust, exact)[2]

    def interRobotConsistency(self, cands, gamma: float = GAMMA_99, peer_cov=None, exact: bool = False,     # noqa: N802
                              robust: bool = False, node_limit=None):
        """closureConsistency for candidates between this graph and a peer robot's: ``cands`` a list of ``(i, peer_pose, meas,
        info_upper)``, i an own vertex index, peer_pose the pose of the peer's vertex as the peer sent it (in no graph yet).
        ``peer_cov`` [3 N, 3 N]: the joint covariance of the peer poses, indexed by candidate; None: they are taken as exact (as
        LoopClosureChecker takes them), and the gate is stricter than the data justify.  Returns ``(d2, adj, clique, seed)``,
        with ``exact`` ``(d2, adj, clique, proven)``, as closureConsistency; a typed graph raises ValueError."""
        a, kw, _ = self._joint_args(robust)
        if "vertex_kind" in kw:
            raise ValueError("interRobotConsistency: pose graphs only (the graph has landmarks or priors)")
        cl = list(cands)
        ca = np.array([c[0] for c in cl], dtype=np.int32)
        pp = np.array([c[1] for c in cl], dtype=np.float64).reshape(len(cl), 3)
        cm = np.array([c[2] for c in cl], dtype=np.float64).reshape(len(cl), 3)
        ci = np.array([c[3] for c in cl], dtype=np.float64).reshape(len(cl), 6)
        if exact:
            if node_limit is not None:
                kw = dict(kw, node_limit=node_limit)
            return self.ctx.closure_consistency_inter_exact(*a, ca, pp, cm, ci, gamma, peer_cov=peer_cov, **kw)[:4]
        return self.ctx.closure_consistency_inter(*a, ca, pp, cm, ci, gamma, peer_cov=peer_cov, **kw)[:4]

    def observationCovariance(self, pairs, kinds, hypotheses=None, robust: bool = False):     # noqa: N802
        """Data association: for the vertex index pairs ``(pose, b)`` predicted as factors of ``kinds`` (per pair 0 EDGE_SE2,
        1 EDGE_SE2_XY, 2 EDGE_BEARING_SE2_XY): ``(z [n, 3], S [n, 3, 3])``, the predicted observation and its covariance
        J Sigma J^T, padded with zeros outside the factor's dimension.  ``hypotheses`` = ``(meas [n, 3], info_upper [n, 6] or
        None)``: then ``(z, S, d2 [n])``, d2 the squared Mahalanobis distance of the candidate measurement under S + Omega^-1."""
        pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        a, kw, _ = self._joint_args(robust)
        hm, hi = (None, None) if hypotheses is None else hypotheses
        z, cz, d2 = self.ctx.observation_covariance(*a, pairs[:, 0], pairs[:, 1], kinds, hm, hi, **kw)[:3]
        return (z, cz) if hypotheses is None else (z, cz, d2)

    def gateObservations(self, pose_idx, landmark_idxs, z, info, kind: int = 1, robust: bool = False):     # noqa: N802
        """The individual-compatibility gate of M measurements taken from pose ``pose_idx`` against L known landmarks:
        ``d2 [M, L]``, the squared Mahalanobis distance of measurement m as an observation of landmark l.  ``z`` [M, 2] and
        ``info`` [M, 3] (I11, I12, I22) for ``kind`` 1, ``z`` [M] and ``info`` [M] for ``kind`` 2 (bearings).  One call over the
        M L pairs (L + 1 unique vertices); the assignment is the caller's."""
        lm = np.asarray(landmark_idxs, dtype=np.int32).reshape(-1)
        zz = np.asarray(z, dtype=np.float64).reshape(-1, 2 if kind == 1 else 1)
        uu = np.asarray(info, dtype=np.float64).reshape(len(zz), -1)
        M, L = len(zz), len(lm)
        hm, hi = np.zeros((M, 3)), np.zeros((M, 6))
        if kind == 1:
            hm[:, :2] = zz
            hi[:, [0, 1, 3]] = uu if uu.shape[1] == 3 else uu[:, [0, 1, 3]]
        elif kind == 2:
            hm[:, 0], hi[:, 0] = zz[:, 0], uu[:, 0]
        else:
            raise ValueError("gateObservations: kind must be 1 (EDGE_SE2_XY) or 2 (EDGE_BEARING_SE2_XY)")
        pairs = np.stack([np.full(M * L, int(pose_idx), dtype=np.int32), np.tile(lm, M)], axis=1)
        d2 = self.observationCovariance(pairs, np.full(M * L, kind, dtype=np.uint8), (np.repeat(hm, L, axis=0), np.repeat(hi, L, axis=0)),
                                        robust)[2]
        return d2.reshape(M, L)

    def associateObservations(self, pose_idx, landmark_idxs, z, info, kind=1, gamma_by_dof=None, node_limit=None,     # noqa: N802
                              robust: bool = False):
        """Joint-compatibility data association (JCBB) of M measurements taken from pose ``pose_idx`` against L known
        landmarks: where gateObservations leaves the assignment to the caller, this returns it.  ``z`` / ``info`` as for
        gateObservations; ``kind`` 1, 2, or one kind per measurement (then ``z`` [M, 2] and ``info`` [M, 3], a bearing in
        column 0).  ``gamma_by_dof``: the thresholds by degrees of freedom (None: the 0.99 quantiles, _lib.JC_GAMMA_99);
        ``node_limit``: joint tests per root and round (None: the binding's default).  Returns ``(assign [M] of vertex indices or
        -1, d2, dof, proven)``: the hypothesis with the most pairings whose every pairing passes its own gate and whose every
        prefix passes the joint one, among those the smallest joint d2; ``proven`` False: the best found within the limit."""
        lm = np.asarray(landmark_idxs, dtype=np.int32).reshape(-1)
        kinds = np.asarray(kind, dtype=np.uint8).reshape(-1)
        mixed = kinds.size > 1
        zz = np.asarray(z, dtype=np.float64)
        zz = zz.reshape(-1, 2) if mixed or int(kinds[0]) == 1 else zz.reshape(-1, 1)
        M = len(zz)
        kinds = kinds if mixed else np.full(M, int(kinds[0]), dtype=np.uint8)
        if kinds.shape != (M,) or not np.all((kinds == 1) | (kinds == 2)):
            raise ValueError("associateObservations: kind must be 1 (EDGE_SE2_XY) or 2 (EDGE_BEARING_SE2_XY), one or one per measurement")
        uu = np.asarray(info, dtype=np.float64).reshape(M, -1)
        hm, hi = np.zeros((M, 3)), np.zeros((M, 6))
        xy = kinds == 1
        if xy.any():
            hm[xy, :2] = zz[xy, :2]
            hi[np.ix_(xy, [0, 1, 3])] = uu[xy][:, :3] if uu.shape[1] == 3 else uu[xy][:, [0, 1, 3]]
        hm[~xy, 0], hi[~xy, 0] = zz[~xy, 0], uu[~xy, 0]
        a, kw, _ = self._joint_args(robust)
        if node_limit is not None:
            kw = dict(kw, node_limit=node_limit)
        assign, _count, d2, dof, proven = self.ctx.joint_compatibility(*a, np.full(M, int(pose_idx), dtype=np.int32), kinds, hm, hi, lm,
                                                                       gamma_by_dof, **kw)[:5]
        return assign, d2, dof, proven

    def addAssociatedObservations(self, pose_idx, landmark_idxs, z, info, kind=1, gamma_by_dof=None, node_limit=None,     # noqa: N802
                                  robust: bool = False):
        """associateObservations, then an addObservation / addBearing edge for every paired measurement (in measurement
        order).  Returns the new edges' indices; an unpaired measurement adds nothing."""
        assign = self.associateObservations(pose_idx, landmark_idxs, z, info, kind, gamma_by_dof, node_limit, robust)[0]
        M = len(assign)
        kinds = np.broadcast_to(np.asarray(kind, dtype=np.uint8).reshape(-1), (M,))
        zz = np.asarray(z, dtype=np.float64).reshape(M, -1)
        uu = np.asarray(info, dtype=np.float64).reshape(M, -1)
        edges = []
        for m in np.flatnonzero(assign >= 0):
            if kinds[m] == 1:
                edges.append(self.addObservation(int(pose_idx), int(assign[m]), zz[m, :2], uu[m, :3] if uu.shape[1] == 3 else uu[m, [0, 1, 3]]))
            else:
                edges.append(self.addBearing(int(pose_idx), int(assign[m]), zz[m, 0], uu[m, 0]))
        return edges

    def chi2(self) -> float:
        g = self.graph
        ef, et, meas, info = g.level0()
        ty = self._typed_level0()
        if ty is not None:
            return float(self.ctx.gn_optimize_typed(g.poses, g.fixed, ef, et, meas, info, 0, ty[0], ty[1])[2][0])
        _, _, chi2 = self.ctx.gn_optimize(g.poses, g.fixed, ef, et, meas, info, 0)
        return float(chi2[0])

    def saveGraph(self, filename):     # noqa: N802 (reference spelling)
        self.graph.save_g2o(filename)
        return True

    def loadGraph(self, filename):     # noqa: N802
        self.graph = PoseGraph.load_g2o(filename)
        return True
