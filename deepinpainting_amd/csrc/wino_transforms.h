// wino_transforms.h — the 1-D transforms of F(4x4, 3x3) that more than one source file applies (winograd.hip: the transform
// kernels of the three-launch path; wino_fused.hip: the same arithmetic inside the one-launch kernel).  Interpolation points
// (0, +-1, +-2, inf); a 2-D transform is the 1-D one over the columns, then over the rows.
#pragma once

namespace ipsr {

__device__ __forceinline__ void wino_bt(const float d[6], float v[6])        // B^T d
{
    v[0] = 4.0f * d[0] - 5.0f * d[2] + d[4];
    v[1] = -4.0f * d[1] - 4.0f * d[2] + d[3] + d[4];
    v[2] = 4.0f * d[1] - 4.0f * d[2] - d[3] + d[4];
    v[3] = -2.0f * d[1] - d[2] + 2.0f * d[3] + d[4];
    v[4] = 2.0f * d[1] - d[2] - 2.0f * d[3] + d[4];
    v[5] = 4.0f * d[1] - 5.0f * d[3] + d[5];
}
__device__ __forceinline__ void wino_at(const float m[6], float y[4])        // A^T m
{
    y[0] = m[0] + m[1] + m[2] + m[3] + m[4];
    y[1] = m[1] - m[2] + 2.0f * m[3] - 2.0f * m[4];
    y[2] = m[1] + m[2] + 4.0f * m[3] + 4.0f * m[4];
    y[3] = m[1] - m[2] + 8.0f * m[3] - 8.0f * m[4] + m[5];
}

}  // namespace ipsr
