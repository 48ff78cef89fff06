// twoview_rows.hpp -- what the kernels over blocks of two-view rows (x1, y1, x2, y2) share: twoview.hip and relpose.hip
#pragma once

// THE residual test: scoring, list building and the mask all call this, so the length of a list and the sum of a mask row equal the
// model's count by construction.  False for a NaN F (an invalid hypothesis).
__device__ __forceinline__ bool twoview_inlier(const double (&F)[9], double x1, double y1, double x2, double y2, double t2)
{
    const double l0 = (F[0] * x1 + F[1] * y1) + F[2];
    const double l1 = (F[3] * x1 + F[4] * y1) + F[5];
    const double l2 = (F[6] * x1 + F[7] * y1) + F[8];
    const double m0 = (F[0] * x2 + F[3] * y2) + F[6];
    const double m1 = (F[1] * x2 + F[4] * y2) + F[7];
    const double e = (x2 * l0 + y2 * l1) + l2;
    const double d = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1;
    return e * e <= t2 * d;
}
__device__ __forceinline__ int clamp_count(int c, int stride) { return c < 0 ? 0 : (c > stride ? stride : c); }
