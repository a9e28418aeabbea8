// The ray walk of one (scan, beam) thread, shared by every kernel that counts cells the way the occupancy map does
// (occupancy_kernels.hip: k_occ_integrate; scan_info_kernels.hip: the per-scan windows and their bounding boxes):
//   FrequencyMap::integrateScan + fillRobotPose   src/ros_map_publisher/frequency_map.cpp:27-103
//   GridLineTraversal::gridLineCore               src/ros_map_publisher/grid_line_traversal.cpp:31-140
// The walk resolves the beam's range rules, maps the end point with the reference's float arithmetic (float subtract /
// divide, round-half-even) and steps through the reference's Bresenham variant.  What happens at a cell is the caller's:
// `sink.miss(x, y)` for every visited cell inside the map, `sink.hit(x, y, gain)` for every stamped one.  One body, so a
// scan's own counts cannot drift from the map's.  Must be compiled with -ffp-contract=off (Makefile default): no FMA may
// replace a float op the reference rounds.
#ifndef CGMR_OCCUPANCY_WALK_H
#define CGMR_OCCUPANCY_WALK_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "occupancy_device.h"

namespace cgmr {

__device__ __forceinline__ bool occ_inside(const OccParams& P, int x, int y) {
  return x >= 0 && y >= 0 && x < P.rows && y < P.cols;
}
// FrequencyMap::world2map (frequency_map.h:46-49)
__device__ __forceinline__ int occ_w2m(float w, float off, float res) { return __float2int_rn((w - off) / res); }

// beam i of the scan S whose ranges start at `ranges`; beam_cs: cosf / sinf of the beam angles
template <class Sink>
__device__ __forceinline__ void occ_walk_beam(const OccParams& P, const OccScan& S, int i, const float* __restrict__ ranges,
                                              const float2* __restrict__ beam_cs, Sink& sink) {
  // fillRobotPose (frequency_map.cpp:89-103): the beams of a scan share out the 9 x 9 cells around the robot
  // (beam i marks cells i, i + n_beams, ...: all 81 whatever the beam count)
  for (int c = i; c < 81; c += P.n_beams) {
    const int rgx = occ_w2m((float)S.rx, P.off_x, P.resolution), rgy = occ_w2m((float)S.ry, P.off_y, P.resolution);
    const int cx = rgx + (c % 9) - 4, cy = rgy + (c / 9) - 4;
    if (occ_inside(P, cx, cy)) sink.miss(cx, cy);
  }
  float r = ranges[i];
  bool cropped = false;
  if (r > P.usable_range) { r = P.usable_range; cropped = true; }
  if (r >= P.max_range || r <= 0) {
    if (P.infinity_filling_range > 0.0f) { r = P.infinity_filling_range; cropped = true; }
    else return;
  }
  const float2 cs = beam_cs[i];
  const double bx = (double)(r * cs.x), by = (double)(r * cs.y);
  const double wx = (S.cl * bx - S.sl * by) + S.lx, wy = (S.sl * bx + S.cl * by) + S.ly;
  const int sx = occ_w2m((float)S.lx, P.off_x, P.resolution), sy = occ_w2m((float)S.ly, P.off_y, P.resolution);
  const int ex = occ_w2m((float)wx, P.off_x, P.resolution), ey = occ_w2m((float)wy, P.off_y, P.resolution);
  // gridLineCore: major axis steps by one from the smaller coordinate, minor axis follows the error term
  const int dx = abs(ex - sx), dy = abs(ey - sy);
  int x, y, d, incr1, incr2, n, step;
  bool xmajor = dy <= dx;
  if (xmajor) {
    d = 2 * dy - dx; incr1 = 2 * dy; incr2 = 2 * (dy - dx);
    int ydirflag;
    if (sx > ex) { x = ex; y = ey; ydirflag = -1; n = sx - ex; }
    else { x = sx; y = sy; ydirflag = 1; n = ex - sx; }
    step = ((ey - sy) * ydirflag) > 0 ? 1 : -1;
  } else {
    d = 2 * dx - dy; incr1 = 2 * dx; incr2 = 2 * (dx - dy);
    int xdirflag;
    if (sy > ey) { y = ey; x = ex; xdirflag = -1; n = sy - ey; }
    else { y = sy; x = sx; xdirflag = 1; n = ey - sy; }
    step = ((ex - sx) * xdirflag) > 0 ? 1 : -1;
  }
  n = min(n, 65535);                               // GRIDTRAVERSAL_MAXPOINTS (grid_line_traversal.h:6)
  if (occ_inside(P, x, y)) sink.miss(x, y);
  for (int k = 0; k < n; k++) {
    if (xmajor) x++; else y++;
    if (d < 0) d += incr1;
    else { if (xmajor) y += step; else x += step; d += incr2; }
    if (occ_inside(P, x, y)) sink.miss(x, y);
  }
  if (!occ_inside(P, ex, ey) || cropped) return;
  for (int c = -P.square_size; c <= P.square_size; c++)
    for (int q = -P.square_size; q <= P.square_size; q++)
      if (occ_inside(P, ex + q, ey + c)) sink.hit(ex + q, ey + c, P.gain);
}

}  // namespace cgmr
#endif
