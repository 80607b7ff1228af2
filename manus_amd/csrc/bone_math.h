// Per-bone 4x4 arithmetic shared by k_bone_transforms (lbs_sh.hip) and the pose chain (pose.hip): one thread per matrix, fp32.
// Bit-equality between the two kernels needs more than the same source: the compiler contracts and packs these loops by what
// feeds them, so both kernels hand bone_mul_inverse a matrix IN MEMORY (global, or LDS behind a barrier in pose.hip) and store
// its result straight to global memory, as k_bone_transforms always did.
#pragma once
#include <hip/hip_runtime.h>

// a[r][0..3] = the matrix, a[r][4..7] = its inverse when this returns: Gauss-Jordan elimination with partial pivoting (the
// operation count and pivoting of the LU route torch.linalg.inv takes; results agree with it to fp32 roundoff).  A singular
// matrix gives non-finite entries, like the reference's inverse raising would stop the step.
__device__ __forceinline__ void bone_invert(const float* __restrict__ m, float (&a)[4][8]) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            a[r][c] = m[r * 4 + c];
            a[r][4 + c] = r == c ? 1.f : 0.f;
        }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int piv = c;
        float best = fabsf(a[c][c]);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r > c && fabsf(a[r][c]) > best) { best = fabsf(a[r][c]); piv = r; }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r == piv && r != c) {
#pragma unroll
                for (int k = 0; k < 8; ++k) { const float t = a[c][k]; a[c][k] = a[r][k]; a[r][k] = t; }
            }
        const float inv = 1.0f / a[c][c];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[c][k] *= inv;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r != c) {
                const float f = a[r][c];
#pragma unroll
                for (int k = 0; k < 8; ++k) a[r][k] -= f * a[c][k];
            }
    }
}

// o = p @ (the inverse half of a), both 4x4 row-major, summed over k = 0 .. 3 in that order
__device__ __forceinline__ void bone_mul_inverse(const float* __restrict__ p, const float (&a)[4][8], float* __restrict__ o) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc += p[r * 4 + k] * a[k][4 + c];
            o[r * 4 + c] = acc;
        }
}

__device__ __forceinline__ void bone_identity(float* __restrict__ o) {
#pragma unroll
    for (int k = 0; k < 16; ++k) o[k] = (k % 5 == 0) ? 1.f : 0.f;
}
