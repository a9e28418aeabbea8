// What the host makes of a cgmr_occupancy_config before anything is queued, shared by cgmr_occupancy_map (occupancy_api.cpp)
// and the scan ranking (scan_info_host.cpp): the argument check, the resolved parameters, the per-scan laser centres and the
// beam table.  Host libm throughout, like the reference.
#pragma once
#include <cmath>
#include <cstring>

#include "cgmr_ctx.h"
#include "occupancy_device.h"

namespace cgmr {

// n_beams >= 1: the beam threads of a scan also carry its fillRobotPose cells (a scan without beams is not a scan)
inline bool occ_args_ok(const cgmr_occupancy_config* cfg, int n_scans, int n_beams, const float* ranges, const double* robot_poses_xyt) {
  return cfg && n_scans >= 0 && n_beams >= 1 && cfg->rows > 0 && cfg->cols > 0 && cfg->resolution > 0 &&
         !(n_scans > 0 && n_beams > 0 && (!ranges || !robot_poses_xyt)) && cfg->square_size >= 0;
}

inline OccParams occ_params(const cgmr_occupancy_config* cfg, int n_scans, int n_beams) {
  OccParams P;
  memset(&P, 0, sizeof P);
  P.rows = cfg->rows; P.cols = cfg->cols;
  P.resolution = cfg->resolution; P.off_x = cfg->offset_x; P.off_y = cfg->offset_y;
  P.max_range = cfg->max_range < 0 ? (float)cfg->laser_max_range : cfg->max_range;        // frequency_map.cpp:29-30
  P.usable_range = cfg->usable_range < 0 ? P.max_range : cfg->usable_range;
  P.infinity_filling_range = cfg->infinity_filling_range;
  P.gain = cfg->gain; P.square_size = cfg->square_size;
  P.n_scans = n_scans; P.n_beams = n_beams;
  return P;
}

inline double occ_normalize_theta(double t) {   // g2o::normalize_theta [g2o-recalled], as everywhere in this library
  const double pi = 3.14159265358979323846;
  if (t >= -pi && t < pi) return t;
  double m = std::floor((t + pi) / (2 * pi));
  return t - 2 * pi * m;
}

// per scan: laserCenter = robotPose * laserPose (frequency_map.cpp:32), its rotation as cos / sin (Eigen Rotation2D)
inline void occ_fill_scans(const cgmr_occupancy_config* cfg, int n_scans, const double* robot_poses_xyt, OccScan* hs) {
  for (int s = 0; s < n_scans; s++) {
    const double* rp = robot_poses_xyt + 3 * (size_t)s;
    const double cr = std::cos(rp[2]), sr = std::sin(rp[2]);
    hs[s].lx = (cr * cfg->laser_pose[0] - sr * cfg->laser_pose[1]) + rp[0];
    hs[s].ly = (sr * cfg->laser_pose[0] + cr * cfg->laser_pose[1]) + rp[1];
    const double lt = occ_normalize_theta(rp[2] + cfg->laser_pose[2]);
    hs[s].cl = std::cos(lt); hs[s].sl = std::sin(lt);
    hs[s].rx = rp[0]; hs[s].ry = rp[1];
  }
}

// beam table: cosf / sinf of the float beam angle (frequency_map.cpp:50-51), host libm like the reference
inline void occ_fill_beams(const cgmr_occupancy_config* cfg, int n_beams, float2* hb) {
  for (int i = 0; i < n_beams; i++) {
    const float a = (float)(cfg->first_beam_angle + i * cfg->angular_step);
    hb[i] = make_float2(cosf(a), sinf(a));
  }
}

}  // namespace cgmr
