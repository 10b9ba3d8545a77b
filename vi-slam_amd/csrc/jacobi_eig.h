// jacobi_eig.h -- the cyclic Jacobi eigen-decomposition shared by pose.hip (recoverPose's vote, triangulation, the homography's pose) and
// ftrack.hip (N-view triangulation).  One text, so every caller rotates in the same order and rounds the same way.
#ifndef VIS_JACOBI_EIG_H_
#define VIS_JACOBI_EIG_H_

#include <hip/hip_runtime.h>

// cyclic Jacobi eigen-decomposition of a symmetric N x N matrix (oracle/pose.cpp jacobi_eig: same rotations in the same order).
// N is a template parameter and every index a constant: the matrices stay in registers (the run-time-n form kept them in
// scratch memory and spent more instructions on addresses than on the rotations).
template <int N>
__device__ __forceinline__ void jacobi_eig(double (&A)[N * N], double (&V)[N * N], bool* zero_theta_last = nullptr) {
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++) V[i * N + j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; sweep++) {
        double off = 0;
#pragma unroll
        for (int i = 0; i < N; i++)
#pragma unroll
            for (int j = i + 1; j < N; j++) off += A[i * N + j] * A[i * N + j];
        if (off < 1e-300) break;
#pragma unroll
        for (int p = 0; p < N; p++)
#pragma unroll
            for (int q = p + 1; q < N; q++) {
                const double apq = A[p * N + q];
                if (fabs(apq) < 1e-300) continue;
                const double app = A[p * N + p], aqq = A[q * N + q];
                const double theta = (aqq - app) / (2.0 * apq);
                // (theta == +-0 takes t = +1 whatever the sign of apq: the one place where negating row / column N-1 of A does not
                // simply negate the matching entries of everything that follows -- see cheirality_pair)
                if (zero_theta_last && q == N - 1 && theta == 0.0) *zero_theta_last = true;
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < N; k++) {
                    const double akp = A[k * N + p], akq = A[k * N + q];
                    A[k * N + p] = c * akp - s * akq;
                    A[k * N + q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < N; k++) {
                    const double apk = A[p * N + k], aqk = A[q * N + k];
                    A[p * N + k] = c * apk - s * aqk;
                    A[q * N + k] = s * apk + c * aqk;
                }
#pragma unroll
                for (int k = 0; k < N; k++) {
                    const double vkp = V[k * N + p], vkq = V[k * N + q];
                    V[k * N + p] = c * vkp - s * vkq;
                    V[k * N + q] = s * vkp + c * vkq;
                }
            }
    }
}

#endif
