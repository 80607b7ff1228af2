// Pose chain on the device (manus_amd/pose.py: PoseRefiner): the per-frame, per-bone correction applied to the posed bone
// matrices of a step's views, the chain rule from dL/d(bone transforms) back to the correction, and its row Adam.
//
//   T[v,b] = (posed[v,b] @ [[exp(rotvec[f,b]), trans[f,b]], [0,0,0,1]]) @ inv(rest[b])        f = the frame view v shows
//
// fp32, one thread per small matrix, one or two workgroups per launch: these launches are bound by latency, not by any
// unit of the chip.  No matrix pipe, no atomics, no workspace.  The inverse and the last product are those of
// k_bone_transforms (bone_math.h), so a zero correction gives the bits of mgr_bone_transforms.
#include "bone_math.h"
#include "mgr_common.h"

#define POSE_BLOCK 256
#define POSE_SMALL 1e-6f      // |r|^2 below which exp and its derivative take their series (pose._exp_so3)

// Rodrigues coefficients of R = I + a K + b K^2, t = |r|^2, and their derivatives by t
__device__ __forceinline__ void pose_coeffs(float t, float& a, float& b, float& da, float& db) {
    if (t < POSE_SMALL) {
        a = 1.0f - t / 6.0f + t * t / 120.0f;
        b = 0.5f - t / 24.0f;
        da = -1.0f / 6.0f + t / 60.0f;
        db = -1.0f / 24.0f;
    } else {
        const float th = sqrtf(t);
        const float s = sinf(th), c = cosf(th), sh = sinf(0.5f * th);
        a = s / th;
        b = 2.0f * sh * sh / t;         // (1 - cos th) / t without the cancellation just above the threshold
        da = (c - a) / (2.0f * t);      // d(sin th / th)/dt
        db = (0.5f * a - b) / t;        // d((1 - cos th) / t)/dt
    }
}

// m (4x4 row-major) = p @ [[exp(r), tr], [0,0,0,1]]
__device__ __forceinline__ void pose_correct(const float* __restrict__ p, const float* __restrict__ r, const float* __restrict__ tr,
                                             float* __restrict__ m) {
    const float x = r[0], y = r[1], z = r[2];
    const float t = x * x + y * y + z * z;
    float a, b, da, db;
    pose_coeffs(t, a, b, da, db);
    // K = [[0,-z,y],[z,0,-x],[-y,x,0]];  K^2 = r r^T - t I, entry by entry as the product K @ K forms it
    float C[4][4];
    C[0][0] = 1.0f + b * (-z * z - y * y);
    C[0][1] = a * -z + b * (x * y);
    C[0][2] = a * y + b * (x * z);
    C[1][0] = a * z + b * (x * y);
    C[1][1] = 1.0f + b * (-z * z - x * x);
    C[1][2] = a * -x + b * (y * z);
    C[2][0] = a * -y + b * (x * z);
    C[2][1] = a * x + b * (y * z);
    C[2][2] = 1.0f + b * (-y * y - x * x);
    C[0][3] = tr[0];
    C[1][3] = tr[1];
    C[2][3] = tr[2];
    C[3][0] = C[3][1] = C[3][2] = 0.0f;
    C[3][3] = 1.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc += p[i * 4 + k] * C[k][j];
            m[i * 4 + j] = acc;
        }
}

// thread (k, b): position k of the step, bone b <= B (row B: the identity of the background).  The (corrected) posed matrix
// goes through LDS and a barrier, so that the last product reads it from memory and stores to global memory exactly as
// k_bone_transforms does (bone_math.h)
__global__ __launch_bounds__(POSE_BLOCK) void k_pose_apply(int V, int B, int F, const int32_t* __restrict__ view_rows,
                                                           const int32_t* __restrict__ frame_of_view, const float* __restrict__ posed,
                                                           const float* __restrict__ rest, const float* __restrict__ rotvec,
                                                           const float* __restrict__ trans, float* __restrict__ transforms,
                                                           float* __restrict__ gathered) {
    __shared__ float s_m[POSE_BLOCK * 16];
    const int gid = blockIdx.x * POSE_BLOCK + threadIdx.x;
    const bool live = gid < V * (B + 1);
    const int k = live ? gid / (B + 1) : 0, b = gid - k * (B + 1);
    const int v = live ? view_rows[k] : -1;
    float* m = s_m + threadIdx.x * 16;
    if (v >= 0 && b < B) {
        const int f = frame_of_view[k];
        const float* p = posed + ((size_t)v * B + b) * 16;
        if (f >= 0 && f < F) {
            const size_t fb = ((size_t)f * B + b) * 3;
            pose_correct(p, rotvec + fb, trans + fb, m);
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) m[q] = p[q];
        }
    }
    __syncthreads();
    if (v < 0) return;
    float* o = transforms + ((size_t)v * (B + 1) + b) * 16;
    if (b >= B) {
        bone_identity(o);
    } else {
        float a[4][8];
        bone_invert(rest + (size_t)b * 16, a);
        bone_mul_inverse(m, a, o);
    }
    if (gathered) {
        const float4* t4 = (const float4*)o;
        float4* g4 = (float4*)(gathered + (size_t)gid * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) g4[q] = t4[q];
    }
}

// thread (u, b): listed frame u, bone b; walks the V positions in ascending order and sums dC = posed^T dT inv(rest)^T (top
// three rows) of those that show the frame, then takes the vector-Jacobian product of exp once (it is linear in dC)
__global__ __launch_bounds__(POSE_BLOCK) void k_pose_backward(int V, int B, int F, int U, const int32_t* __restrict__ frames_listed,
                                                              const int32_t* __restrict__ view_rows,
                                                              const int32_t* __restrict__ frame_of_view, const float* __restrict__ posed,
                                                              const float* __restrict__ rest, const float* __restrict__ rotvec,
                                                              const float* __restrict__ d_transforms, float* __restrict__ d_rotvec,
                                                              float* __restrict__ d_trans) {
    const int gid = blockIdx.x * POSE_BLOCK + threadIdx.x;
    if (gid >= U * B) return;
    const int u = gid / B, b = gid - u * B;
    const int f = frames_listed[u];
    float dC[3][4];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) dC[i][j] = 0.f;
    float* o_r = d_rotvec + (size_t)gid * 3;
    float* o_t = d_trans + (size_t)gid * 3;
    if (f < 0 || f >= F) {
        o_r[0] = o_r[1] = o_r[2] = 0.f;
        o_t[0] = o_t[1] = o_t[2] = 0.f;
        return;
    }
    float a[4][8];
    bone_invert(rest + (size_t)b * 16, a);
    for (int k = 0; k < V; ++k) {
        if (frame_of_view[k] != f) continue;
        const int v = view_rows[k];
        if (v < 0) continue;
        const float* dT = d_transforms + ((size_t)k * (B + 1) + b) * 16;
        const float* p = posed + ((size_t)v * B + b) * 16;
        float X[4][4];      // dT @ inv(rest)^T: dL/d(corrected posed matrix)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float acc = 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q) acc += dT[i * 4 + q] * a[j][4 + q];
                X[i][j] = acc;
            }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float acc = 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q) acc += p[q * 4 + i] * X[q][j];
                dC[i][j] += acc;
            }
    }
    const float* r = rotvec + ((size_t)f * B + b) * 3;
    const float x = r[0], y = r[1], z = r[2];
    const float t = x * x + y * y + z * z;
    float ca, cb, da, db;
    pose_coeffs(t, ca, cb, da, db);
    // G = dL/dR = dC[:3,:3].  <G,K> and <G,K^2> with K^2 = r r^T - t I
    const float gk = x * (dC[2][1] - dC[1][2]) + y * (dC[0][2] - dC[2][0]) + z * (dC[1][0] - dC[0][1]);
    const float tr_g = dC[0][0] + dC[1][1] + dC[2][2];
    const float sx = (dC[0][0] + dC[0][0]) * x + (dC[0][1] + dC[1][0]) * y + (dC[0][2] + dC[2][0]) * z;      // ((G + G^T) r)
    const float sy = (dC[1][0] + dC[0][1]) * x + (dC[1][1] + dC[1][1]) * y + (dC[1][2] + dC[2][1]) * z;
    const float sz = (dC[2][0] + dC[0][2]) * x + (dC[2][1] + dC[1][2]) * y + (dC[2][2] + dC[2][2]) * z;
    const float gk2 = 0.5f * (x * sx + y * sy + z * sz) - t * tr_g;
    const float w = 2.0f * (da * gk + db * gk2);      // through t = |r|^2 in the coefficients
    o_r[0] = ca * (dC[2][1] - dC[1][2]) + cb * (sx - 2.0f * x * tr_g) + w * x;
    o_r[1] = ca * (dC[0][2] - dC[2][0]) + cb * (sy - 2.0f * y * tr_g) + w * y;
    o_r[2] = ca * (dC[1][0] - dC[0][1]) + cb * (sz - 2.0f * z * tr_g) + w * z;
    o_t[0] = dC[0][3];
    o_t[1] = dC[1][3];
    o_t[2] = dC[2][3];
}

// thread (u, b, c): element c of the correction of bone b of listed frame u, rotation vector and translation; the arithmetic
// of k_sg_adam (torch.optim.SparseAdam), no clamp
__device__ __forceinline__ void pose_adam_one(float g, float* __restrict__ x, float* __restrict__ m_, float* __restrict__ v_,
                                              float step_size, float omb1, float omb2, float eps) {
    const float m0 = *m_, v0 = *v_;
    const float m = m0 + (g - m0) * omb1;
    const float v = v0 + (g * g - v0) * omb2;
    *m_ = m;
    *v_ = v;
    *x = *x - step_size * (m / (sqrtf(v) + eps));
}

__global__ __launch_bounds__(POSE_BLOCK) void k_pose_adam(int U, int B, const int32_t* __restrict__ frames_listed,
                                                          const float* __restrict__ d_rotvec, const float* __restrict__ d_trans,
                                                          float* __restrict__ rotvec, float* __restrict__ trans,
                                                          float* __restrict__ m_r, float* __restrict__ v_r, float* __restrict__ m_t,
                                                          float* __restrict__ v_t, float step_rot, float step_trans, float omb1,
                                                          float omb2, float eps) {
    const int gid = blockIdx.x * POSE_BLOCK + threadIdx.x;
    const int row = B * 3;
    if (gid >= U * row) return;
    const int u = gid / row, e = gid - u * row;
    const int f = frames_listed[u];
    if (f < 0) return;
    const size_t o = (size_t)f * row + e;
    pose_adam_one(d_rotvec[gid], rotvec + o, m_r + o, v_r + o, step_rot, omb1, omb2, eps);
    pose_adam_one(d_trans[gid], trans + o, m_t + o, v_t + o, step_trans, omb1, omb2, eps);
}

// ---------------------------------------------------------------------------
// host entries: every refusal is decided on the arguments, before any launch
// ---------------------------------------------------------------------------
extern "C" int mgr_pose_apply(int V, int B, int F, const int32_t* view_rows, const int32_t* frame_of_view, const float* posed,
                              const float* rest, const float* rotvec, const float* trans, float* transforms, float* gathered,
                              void* stream_) {
    if (V < 1 || B < 1 || B > MGR_MAX_BONES || F < 1)
        return mgr_fail(MGR_EINVAL, "mgr_pose_apply: V and F must be at least 1, B 1 .. MGR_MAX_BONES");
    if (!view_rows || !frame_of_view || !posed || !rest || !rotvec || !trans || !transforms)
        return mgr_fail(MGR_EINVAL, "mgr_pose_apply: null pointer");
    if ((long long)V * (B + 1) > (1ll << 24)) return mgr_fail(MGR_EINVAL, "mgr_pose_apply: V * (B + 1) above 2^24");
    hipStream_t stream = (hipStream_t)stream_;
    const int n = V * (B + 1);
    {
        MGR_PROF("k_pose_apply", stream);
        hipLaunchKernelGGL(k_pose_apply, dim3((n + POSE_BLOCK - 1) / POSE_BLOCK), dim3(POSE_BLOCK), 0, stream, V, B, F, view_rows,
                           frame_of_view, posed, rest, rotvec, trans, transforms, gathered);
    }
    MGR_LAUNCH_CHECK("k_pose_apply", stream, 0);
    return MGR_OK;
}

extern "C" int mgr_pose_backward(int V, int B, int F, int U, const int32_t* frames_listed, const int32_t* view_rows,
                                 const int32_t* frame_of_view, const float* posed, const float* rest, const float* rotvec,
                                 const float* trans, const float* d_transforms, float* d_rotvec, float* d_trans, void* stream_) {
    if (V < 1 || B < 1 || B > MGR_MAX_BONES || F < 1 || U < 1)
        return mgr_fail(MGR_EINVAL, "mgr_pose_backward: V, F and U must be at least 1, B 1 .. MGR_MAX_BONES");
    if (!frames_listed || !view_rows || !frame_of_view || !posed || !rest || !rotvec || !trans || !d_transforms || !d_rotvec || !d_trans)
        return mgr_fail(MGR_EINVAL, "mgr_pose_backward: null pointer");
    if ((long long)V * (B + 1) > (1ll << 24) || (long long)U * B > (1ll << 24))
        return mgr_fail(MGR_EINVAL, "mgr_pose_backward: V * (B + 1) or U * B above 2^24");
    hipStream_t stream = (hipStream_t)stream_;
    const int n = U * B;
    {
        MGR_PROF("k_pose_backward", stream);
        hipLaunchKernelGGL(k_pose_backward, dim3((n + POSE_BLOCK - 1) / POSE_BLOCK), dim3(POSE_BLOCK), 0, stream, V, B, F, U, frames_listed,
                           view_rows, frame_of_view, posed, rest, rotvec, d_transforms, d_rotvec, d_trans);
    }
    MGR_LAUNCH_CHECK("k_pose_backward", stream, 0);
    return MGR_OK;
}

extern "C" int mgr_pose_adam(int U, int B, const int32_t* frames_listed, const float* d_rotvec, const float* d_trans, float* rotvec,
                             float* trans, float* m_r, float* v_r, float* m_t, float* v_t, double lr_rot, double lr_trans,
                             double beta1, double beta2, double eps, int step, void* stream_) {
    if (U < 1 || B < 1 || B > MGR_MAX_BONES) return mgr_fail(MGR_EINVAL, "mgr_pose_adam: U must be at least 1, B 1 .. MGR_MAX_BONES");
    if (step < 1) return mgr_fail(MGR_EINVAL, "mgr_pose_adam: step < 1");
    if (!frames_listed || !d_rotvec || !d_trans || !rotvec || !trans || !m_r || !v_r || !m_t || !v_t)
        return mgr_fail(MGR_EINVAL, "mgr_pose_adam: null pointer");
    if ((long long)U * B * 3 > (1ll << 24)) return mgr_fail(MGR_EINVAL, "mgr_pose_adam: U * B above 2^24 / 3");
    hipStream_t stream = (hipStream_t)stream_;
    // the bias corrections of the global step, in double as torch takes them (mgr_skin_grid_adam)
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    const double k = sqrt(bc2) / bc1;
    const int n = U * B * 3;
    {
        MGR_PROF("k_pose_adam", stream);
        hipLaunchKernelGGL(k_pose_adam, dim3((n + POSE_BLOCK - 1) / POSE_BLOCK), dim3(POSE_BLOCK), 0, stream, U, B, frames_listed, d_rotvec,
                           d_trans, rotvec, trans, m_r, v_r, m_t, v_t, (float)(lr_rot * k), (float)(lr_trans * k), (float)(1.0 - beta1),
                           (float)(1.0 - beta2), (float)eps);
    }
    MGR_LAUNCH_CHECK("k_pose_adam", stream, 0);
    return MGR_OK;
}
