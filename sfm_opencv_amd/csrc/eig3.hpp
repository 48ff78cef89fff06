// eig3.hpp -- eigenvector of the smallest eigenvalue of a symmetric 3 x 3 matrix (cyclic Jacobi), shared by normals.hip and planes.hip.
// The text of eig3_min is the one normals.hip has always had: the contract with oracle/orc_normals.c (equal in every bit) rests on it.
#pragma once

__device__ __forceinline__ void eig3_min(const double Cin[9], double v[3])
{
    double A[3][3], V[3][3] = { { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 } };
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) A[i][j] = Cin[3 * i + j];
    for (int sweep = 0; sweep < 50; ++sweep) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        if (off == 0.0) break;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;      // (0,1) (0,2) (1,2)
            if (A[p][q] == 0.0) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
            const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
            for (int k = 0; k < 3; ++k) { const double x = A[k][p], y = A[k][q]; A[k][p] = c * x - s * y; A[k][q] = s * x + c * y; }
#pragma unroll
            for (int k = 0; k < 3; ++k) { const double x = A[p][k], y = A[q][k]; A[p][k] = c * x - s * y; A[q][k] = s * x + c * y; }
#pragma unroll
            for (int k = 0; k < 3; ++k) { const double x = V[k][p], y = V[k][q]; V[k][p] = c * x - s * y; V[k][q] = s * x + c * y; }
        }
    }
    v[0] = V[0][0]; v[1] = V[1][0]; v[2] = V[2][0];
    double best = A[0][0];
    if (A[1][1] < best) { best = A[1][1]; v[0] = V[0][1]; v[1] = V[1][1]; v[2] = V[2][1]; }
    if (A[2][2] < best) { best = A[2][2]; v[0] = V[0][2]; v[1] = V[1][2]; v[2] = V[2][2]; }
}
