// design_device.h -- what the two tap designers (lcmv_design.hip, mvdr_design.hip) share on the device: which direction a slot of d_offsets names,
// and the constant of their phases.
#pragma once
#include <hip/hip_runtime.h>

namespace bf {

constexpr double kTwoPi = 6.283185307179586476925286766559;

// The tracker's rule (bf_fuse_boxes_device words it): a source iff >= 0, a multiple of offset_per_dir, and a direction of the table.
__device__ __forceinline__ int slot_direction(int off, int offset_per_dir, int dirs)
{
    if (off < 0 || off % offset_per_dir != 0) return -1;
    const int d = off / offset_per_dir;
    return d < dirs ? d : -1;
}

}  // namespace bf
