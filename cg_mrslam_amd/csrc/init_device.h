// Chordal initialisation (init_kernels.hip; include/cgmr.h: cgmr_chordal_initialize): the two linear stages' linearisation, which
// writes the 33-double edge record of gn_kernels.hip, and the pass end that turns the solved (c, s) back into headings.
#pragma once
#include <hip/hip_runtime_api.h>

#include "gn_device.h"

namespace cgmr {

constexpr int kChordalRotation = 1, kChordalTranslation = 2;      // GnEdges::chordal_stage; the bits of cgmr_chordal_initialize's `stages`
constexpr int kChordalDegenerateWord = 3;                         // the word of GnDevice::status that counts the degenerate headings

// launch_linearize's branch for Ed.chordal_stage != 0 (never a batch, never robust, never GNC)
void launch_linearize_chordal(hipStream_t st, const GnDevice& D, const double* poses, const GnEdges& Ed);
// the rotation stage's pass end, in the place of launch_update
void launch_apply_rotation(hipStream_t st, const GnDevice& D, double* poses);

}  // namespace cgmr
