"""Test infrastructure: an independent plain-Python restatement of the reference's occupancy map, written from the reference's
own lines and from nothing else (not from oracle/occupancy_oracle.c, not from the HIP kernels):

  world2map / isInside                      src/ros_map_publisher/frequency_map.h:42-50
  integrateScan / fillRobotPose             src/ros_map_publisher/frequency_map.cpp:27-103
  gridLineCore / gridLine                   src/ros_map_publisher/grid_line_traversal.cpp:3-126
  Graph2occupancy::computeMap               src/ros_map_publisher/graph2occupancy.cpp:29-164 (members: graph2occupancy.h:66-76)

Arithmetic.  Whatever the reference computes in ``float`` is computed here on ``np.float32`` scalars, one operation at a time
(IEEE single precision, no contraction); whatever it computes in ``double`` on Python floats.  ``lrint`` is ``np.rint``
(round half to even, the default rounding mode).  The beam's ``cosf`` / ``sinf`` (frequency_map.cpp:53-54) are the C library's,
called through ctypes with the double sum ``firstBeamAngle + i * angularStep`` narrowed to float as the call narrows it: numpy's
vectorised float32 cos / sin may dispatch to SIMD variants that differ by an ulp from one CPU to the next.  ``cos`` / ``sin`` of
a double are ``math.cos`` / ``math.sin``, the same C library the reference's Eigen Rotation2D calls.

g2o's SE2 (not part of the reference's tree) is restated as recalled from g2o/types/slam2d/se2.h and g2o/stuff/misc.h:
SE2(x, y, theta) keeps theta as given; ``a * b`` has translation a.t + R(a.theta) b.t and angle normalize_theta(a.theta +
b.theta); ``a * v`` is a.t + R(a.theta) v; normalize_theta leaves [-pi, pi) alone, otherwise subtracts floor(theta / 2 pi)
turns and then corrects by one more turn if needed.

Nothing under ``cg_mrslam_amd/`` imports this file and it imports nothing from there.
"""
import ctypes
import ctypes.util
import math

import numpy as np

f32 = np.float32
DBL_MAX = float(np.finfo(np.float64).max)
DBL_MIN = float(np.finfo(np.float64).tiny)            # numeric_limits<double>::min(): the smallest positive normal double
FREE, UNKNOWN, OCCUPIED = 0, 255, 100                 # graph2occupancy.h:79-81 (unsigned char -1 == 255)
SIZE_ROBOT = 4                                        # frequency_map.cpp:94

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
for _f in (_libm.cosf, _libm.sinf):
    _f.restype, _f.argtypes = ctypes.c_float, [ctypes.c_float]


def cosf(a):
    return f32(_libm.cosf(ctypes.c_float(float(a))))


def sinf(a):
    return f32(_libm.sinf(ctypes.c_float(float(a))))


# ------------------------------------------------------------------------------------------------------------------ g2o's SE2
def normalize_theta(theta):
    if -math.pi <= theta < math.pi:
        return theta
    multiplier = math.floor(theta / (2 * math.pi))
    theta = theta - multiplier * 2 * math.pi
    if theta >= math.pi:
        theta -= 2 * math.pi
    if theta < -math.pi:
        theta += 2 * math.pi
    return theta


def se2_mul(a, b):
    c, s = math.cos(a[2]), math.sin(a[2])
    return (a[0] + (c * b[0] - s * b[1]), a[1] + (s * b[0] + c * b[1]), normalize_theta(a[2] + b[2]))


def se2_apply(a, v):
    c, s = math.cos(a[2]), math.sin(a[2])
    return (a[0] + (c * v[0] - s * v[1]), a[1] + (s * v[0] + c * v[1]))


# --------------------------------------------------------------------------------------------------------- frequency_map.h:42-50
def world2map(wx, wy, offset, resolution):
    """``wx``, ``wy`` already narrowed to float by the caller, as the Vector2f argument is."""
    assert all(isinstance(v, f32) for v in (wx, wy, offset[0], offset[1], resolution))
    return int(np.rint((wx - offset[0]) / resolution)), int(np.rint((wy - offset[1]) / resolution))


def is_inside(p, rows, cols):
    return p[0] >= 0 and p[1] >= 0 and p[0] < rows and p[1] < cols


# ------------------------------------------------------------------------------------------------- grid_line_traversal.cpp:3-126
def grid_line_core(start, end):
    dx = abs(end[0] - start[0])
    dy = abs(end[1] - start[1])
    pts = []
    if dy <= dx:
        d = 2 * dy - dx
        incr1 = 2 * dy
        incr2 = 2 * (dy - dx)
        if start[0] > end[0]:
            x, y, ydirflag, xend = end[0], end[1], -1, start[0]
        else:
            x, y, ydirflag, xend = start[0], start[1], 1, end[0]
        pts.append((x, y))
        if (end[1] - start[1]) * ydirflag > 0:
            while x < xend:
                x += 1
                if d < 0:
                    d += incr1
                else:
                    y += 1
                    d += incr2
                pts.append((x, y))
        else:
            while x < xend:
                x += 1
                if d < 0:
                    d += incr1
                else:
                    y -= 1
                    d += incr2
                pts.append((x, y))
    else:
        d = 2 * dx - dy
        incr1 = 2 * dx
        incr2 = 2 * (dx - dy)
        if start[1] > end[1]:
            y, x, yend, xdirflag = end[1], end[0], start[1], -1
        else:
            y, x, yend, xdirflag = start[1], start[0], end[1], 1
        pts.append((x, y))
        if (end[0] - start[0]) * xdirflag > 0:
            while y < yend:
                y += 1
                if d < 0:
                    d += incr1
                else:
                    x += 1
                    d += incr2
                pts.append((x, y))
        else:
            while y < yend:
                y += 1
                if d < 0:
                    d += incr1
                else:
                    x -= 1
                    d += incr2
                pts.append((x, y))
    return pts


def grid_line(start, end):
    """gridLine (:113-126): the cells of gridLineCore, turned round where they do not begin at ``start``."""
    start, end = (int(start[0]), int(start[1])), (int(end[0]), int(end[1]))
    pts = grid_line_core(start, end)
    if start != pts[0]:
        half = len(pts) // 2
        i, j = 0, len(pts) - 1
        while i < half:
            pts[i], pts[j] = pts[j], pts[i]
            i += 1
            j -= 1
    return pts


# ---------------------------------------------------------------------------------------------------- frequency_map.cpp:27-103
def beam_ends(rows, cols, resolution, offset, ranges, robot_pose, first_beam_angle, angular_step, laser_max_range,
              laser_pose=(0.0, 0.0, 0.0), max_range=-1.0, usable_range=-1.0, infinity_filling_range=-1.0):
    """What integrateScan decides per beam of ONE scan before it touches a cell: (start cell, the float point it was mapped from,
    beams), with per beam either None (the beam is skipped) or (end cell, cropped, the range it was cast with, the float point the
    end cell was mapped from).  ``integrate_scan`` is built on this; the case table's reach predicates read it."""
    resolution, offset = f32(resolution), (f32(offset[0]), f32(offset[1]))
    max_range, usable_range, infinity_filling_range = f32(max_range), f32(usable_range), f32(infinity_filling_range)
    if max_range < 0:
        max_range = f32(laser_max_range)
    if usable_range < 0:
        usable_range = max_range
    laser_center = se2_mul(tuple(float(v) for v in robot_pose), tuple(float(v) for v in laser_pose))
    rp = (f32(laser_center[0]), f32(laser_center[1]))
    start = world2map(rp[0], rp[1], offset, resolution)
    beams = []
    for i, r in enumerate(ranges):
        r = f32(r)
        cropped = False
        if r > usable_range:
            r = usable_range
            cropped = True
        if r >= max_range or r <= 0:
            if infinity_filling_range > 0.0:
                r = infinity_filling_range
                cropped = True
            else:
                beams.append(None)
                continue
        a = f32(first_beam_angle + i * angular_step)
        bp = (float(r * cosf(a)), float(r * sinf(a)))
        bp = se2_apply(laser_center, bp)
        bpf = (f32(bp[0]), f32(bp[1]))
        end = world2map(bpf[0], bpf[1], offset, resolution)
        beams.append((end, cropped, r, bpf))
    return start, rp, beams


def fill_robot_pose(misses, resolution, offset, robot_pose):
    rows, cols = misses.shape
    rgrid = world2map(f32(robot_pose[0]), f32(robot_pose[1]), (f32(offset[0]), f32(offset[1])), f32(resolution))
    for c in range(-SIZE_ROBOT, SIZE_ROBOT + 1):
        for r in range(-SIZE_ROBOT, SIZE_ROBOT + 1):
            cell = (rgrid[0] + r, rgrid[1] + c)
            if is_inside(cell, rows, cols):
                misses[cell] += 1
    return rgrid


def integrate_scan(hits, misses, resolution, offset, ranges, robot_pose, first_beam_angle, angular_step, laser_max_range,
                   laser_pose=(0.0, 0.0, 0.0), max_range=-1.0, usable_range=-1.0, infinity_filling_range=-1.0, gain=1, square_size=1):
    rows, cols = hits.shape
    start, _, beams = beam_ends(rows, cols, resolution, offset, ranges, robot_pose, first_beam_angle, angular_step, laser_max_range,
                             laser_pose, max_range, usable_range, infinity_filling_range)
    for b in beams:
        if b is None:
            continue
        end, cropped = b[0], b[1]
        for p in grid_line(start, end):
            if is_inside(p, rows, cols):
                misses[p] += 1
        if not is_inside(end, rows, cols):
            continue
        if not cropped:
            for c in range(-square_size, square_size + 1):
                for r in range(-square_size, square_size + 1):
                    sub = (end[0] + r, end[1] + c)
                    if is_inside(sub, rows, cols):
                        hits[sub] += gain
    fill_robot_pose(misses, resolution, offset, robot_pose)


def integrate(rows, cols, resolution, offset, scans, robot_poses, first_beam_angle, angular_step, laser_max_range,
              laser_pose=(0.0, 0.0, 0.0), max_range=-1.0, usable_range=-1.0, infinity_filling_range=-1.0, gain=1, square_size=1):
    """graph2occupancy.cpp:125-127: every scan into one map.  Returns (hits, misses), int64 [rows, cols]."""
    hits = np.zeros((rows, cols), dtype=np.int64)
    misses = np.zeros((rows, cols), dtype=np.int64)
    for ranges, pose in zip(scans, robot_poses):
        integrate_scan(hits, misses, resolution, offset, ranges, pose, first_beam_angle, angular_step, laser_max_range, laser_pose,
                       max_range, usable_range, infinity_filling_range, int(gain), int(square_size))
    return hits, misses


# ------------------------------------------------------------------------------------------------- graph2occupancy.cpp:128-147
def image(hits, misses, threshold, free_threshold):
    threshold, free_threshold = f32(threshold), f32(free_threshold)
    out = np.empty(hits.shape, dtype=np.uint8)
    for idx in np.ndindex(hits.shape):
        h, m = int(hits[idx]), int(misses[idx])
        if m == 0 and h == 0:
            out[idx] = UNKNOWN
            continue
        fraction = f32(h) / f32(h + m)
        if free_threshold != 0 and fraction < free_threshold:
            out[idx] = FREE
        elif threshold != 0 and fraction > threshold:
            out[idx] = OCCUPIED
        else:
            out[idx] = UNKNOWN
    return out


# ---------------------------------------------------------------------------------------- graph2occupancy.cpp:44-123, :153-162
def base_transform(angle):
    """SE2 baseTransform(0, 0, _angle) with ``float _angle`` (graph2occupancy.h:75; srslam.cpp:107 holds it as float too)."""
    return (0.0, 0.0, float(f32(angle)))


def geometry(poses, angle, usable_range, resolution, rows=0, cols=0, base=None):
    """(transformed poses [K, 3] float64, (size x, size y), (offset x, offset y) as float32): ``poses`` the estimates of the
    vertices that carry a laser, in id order; ``usable_range`` and ``resolution`` the float members.  ``base``: another base
    transform than the reference's, for a test that wants to know what a different one would give."""
    base = base_transform(angle) if base is None else base
    usable_range, resolution = f32(usable_range), f32(resolution)
    xmin = ymin = DBL_MAX
    xmax = ymax = DBL_MIN
    tposes = []
    for p in poses:
        t = se2_mul(base, (float(p[0]), float(p[1]), float(p[2])))
        tposes.append(t)
        x, y = t[0], t[1]
        ur = float(usable_range)                              # double + float: the float is widened
        xmax = xmax if xmax > x + ur else x + ur
        ymax = ymax if ymax > y + ur else y + ur
        xmin = xmin if xmin < x - ur else x - ur
        ymin = ymin if ymin < y - ur else y - ur
    if rows != 0 and cols != 0:
        size = (int(rows), int(cols))
    else:
        size = (int((xmax - xmin) / float(resolution)), int((ymax - ymin) / float(resolution)))   # Vector2i from doubles: truncation
    return np.array(tposes, dtype=np.float64).reshape(-1, 3), size, (f32(xmin), f32(ymin))


def map_center(poses, fixed, angle, offset, resolution, image_rows):
    """graph2occupancy.cpp:153-162 with the first fixed vertex's transformed estimate (:59-62); (0, 0) without one."""
    resolution, offset = f32(resolution), (f32(offset[0]), f32(offset[1]))
    origin = np.zeros(2, dtype=np.float32)
    for p, fx in zip(poses, fixed if fixed is not None else []):
        if fx:
            ip = se2_mul(base_transform(angle), (float(p[0]), float(p[1]), float(p[2])))
            om = world2map(f32(ip[0]), f32(ip[1]), offset, resolution)
            origin[0] = f32(float(-resolution * f32(om[1])) + ip[1])
            origin[1] = f32(-(float(resolution * f32(image_rows - om[0])) + ip[0]))
            break
    return origin
