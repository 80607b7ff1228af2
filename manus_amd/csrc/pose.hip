// Pose chain on the device (manus_amd/pose.py: PoseRefiner): the per-frame, per-bone correction applied to the posed bone
// matrices of a step's views, the chain rule from dL/d(bone transforms) back to the correction, and its row Adam.
//
//   T[v,b] = (posed[v,b] @ [[exp(rotvec[f,b]), trans[f,b]], [0,0,0,1]]) @ inv(rest[b])        f = the frame view v shows
//
// fp32, one thread per small matrix, one or two workgroups per launch: these launches are bound by latency, not by any
// unit of the chip.  No matrix pipe, no atomics; the one workspace is the per-thread fp64 shares of the priors' value
// (mgr_pose_backward_prior).  The inverse and the last product are those of k_bone_transforms (bone_math.h), so a zero
// correction gives the bits of mgr_bone_transforms.
//
// Priors on the corrections (magnitude, and smoothness along the frames of a take): k_pose_backward<true> is k_pose_backward<false>,
// the same body, with dE/dx of the listed rows added and E's share of those rows folded in fp64 by k_pose_prior_fold.  The tables
// are only read there; mgr_pose_adam is the launch behind, so every prior gradient of a step sees the tables from before it (Jacobi).
#include <cmath>

#include "bone_math.h"
#include "mgr_common.h"
#include "pose_adam.h"

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

// Prior on one table x (rotvec or trans) at bone b of frame f, E = w_mag sum |x_f|^2 + w_smooth sum_edges |x_f - x_next(f)|^2:
// adds dE/dx_f = 2 w_mag x_f + 2 w_smooth ((x_f - x_prev) + (x_f - x_next)) to g -- fp32, the differences first, their sum prev
// first, the two products (c_mag = 2 w_mag, c_smooth = 2 w_smooth), then the addition, none of it contracted -- and returns this
// thread's share of the value in fp64: the magnitude term, the edge to next, and the edge to prev when `count_prev` (prev is not
// listed, so no other thread counts it).  prev / next: -1 = none.  Both weights zero: g is left as it is, the share is 0
__device__ __forceinline__ double pose_prior_one(const float* x_tab, int B, int f, int prev, int next, int b,
                                                 bool count_prev, float c_mag, float c_smooth, double w_mag, double w_smooth,
                                                 float* g) {
    if (w_mag == 0.0 && w_smooth == 0.0) return 0.0;
    const float* x = x_tab + ((size_t)f * B + b) * 3;
    const float* xp = x_tab + ((size_t)(prev >= 0 ? prev : f) * B + b) * 3;
    const float* xn = x_tab + ((size_t)(next >= 0 ? next : f) * B + b) * 3;
    double mag = 0.0, e_prev = 0.0, e_next = 0.0;
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float xc = x[c];
            const float dp = xc - xp[c], dn = xc - xn[c];      // (0 where the neighbour is missing: it stands in for itself)
            const float s = prev >= 0 ? (next >= 0 ? dp + dn : dp) : (next >= 0 ? dn : 0.f);
            const float pm = c_mag * xc, ps = c_smooth * s;
            g[c] = g[c] + (pm + ps);
            mag += (double)xc * (double)xc;
            e_prev += (double)dp * (double)dp;
            e_next += (double)dn * (double)dn;
        }
    }
    const double edges = (prev >= 0 && count_prev ? e_prev : 0.0) + (next >= 0 ? e_next : 0.0);
    return w_mag * mag + w_smooth * edges;
}

// The weights of the priors and what they read and leave: w_* in double for the value, c_* = (float)(2 w_*) for the gradient
struct PosePrior {
    const float* trans;            // (F,B,3), read only (as rotvec is)
    const int32_t* neighbours;     // (F,2) prev, next; outside [0,F): none
    double* partial;               // (U * B) the threads' shares of the value
    double w_mag_r, w_smooth_r, w_mag_t, w_smooth_t;
    float c_mag_r, c_smooth_r, c_mag_t, c_smooth_t;
};

// thread (u, b): listed frame u, bone b; walks the V positions in ascending order and sums dC = posed^T dT inv(rest)^T (top
// three rows) of those that show the frame, then takes the vector-Jacobian product of exp once (it is linear in dC).
// ONE body for both instantiations, so the chain gradient is the same sums in the same order: PRIOR false is k_pose_backward
// as it always was (the body stays in the kernel itself: moved into an inlined function, the compiler contracts other
// products into its fused multiply-adds and the last bits move); PRIOR true adds dE/dx of the priors on both tables behind
// it and leaves one fp64 share of the value per thread in pr.partial[u * B + b].  The correction tables are only read.  A
// neighbour outside [0,F) counts as none; whether prev is listed is a walk over frames_listed (U is a step's views at most)
template <bool PRIOR>
__global__ __launch_bounds__(POSE_BLOCK) void k_pose_backward(int V, int B, int F, int U, const int32_t* __restrict__ frames_listed,
                                                              const int32_t* __restrict__ view_rows,
                                                              const int32_t* __restrict__ frame_of_view, const float* __restrict__ posed,
                                                              const float* __restrict__ rest, const float* __restrict__ rotvec,
                                                              const float* __restrict__ d_transforms, float* __restrict__ d_rotvec,
                                                              float* __restrict__ d_trans, PosePrior pr) {
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
        if (PRIOR) pr.partial[gid] = 0.0;
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
    float g_r[3], g_t[3];
    g_r[0] = ca * (dC[2][1] - dC[1][2]) + cb * (sx - 2.0f * x * tr_g) + w * x;
    g_r[1] = ca * (dC[0][2] - dC[2][0]) + cb * (sy - 2.0f * y * tr_g) + w * y;
    g_r[2] = ca * (dC[1][0] - dC[0][1]) + cb * (sz - 2.0f * z * tr_g) + w * z;
    g_t[0] = dC[0][3];
    g_t[1] = dC[1][3];
    g_t[2] = dC[2][3];
    if (PRIOR) {
        int prev = -1, next = -1;
        if (pr.neighbours) {
            prev = pr.neighbours[2 * (size_t)f];
            next = pr.neighbours[2 * (size_t)f + 1];
            if (prev < 0 || prev >= F) prev = -1;
            if (next < 0 || next >= F) next = -1;
        }
        bool prev_listed = false;
        if (prev >= 0)
            for (int q = 0; q < U; ++q) prev_listed = prev_listed || frames_listed[q] == prev;
        const double part_r = pose_prior_one(rotvec, B, f, prev, next, b, !prev_listed, pr.c_mag_r, pr.c_smooth_r, pr.w_mag_r, pr.w_smooth_r, g_r);
        const double part_t = pose_prior_one(pr.trans, B, f, prev, next, b, !prev_listed, pr.c_mag_t, pr.c_smooth_t, pr.w_mag_t, pr.w_smooth_t, g_t);
        pr.partial[gid] = part_r + part_t;
    }
    o_r[0] = g_r[0];
    o_r[1] = g_r[1];
    o_r[2] = g_r[2];
    o_t[0] = g_t[0];
    o_t[1] = g_t[1];
    o_t[2] = g_t[2];
}


// one workgroup over the n per-thread shares: thread t adds partial[t], partial[t + 256], ... in ascending order, the 256 sums
// meet in a fixed tree (k_sg_refine_fold)
__global__ __launch_bounds__(POSE_BLOCK) void k_pose_prior_fold(const double* __restrict__ partial, int n, double* __restrict__ prior_value) {
    __shared__ double s_sum[POSE_BLOCK];
    double acc = 0.0;
    for (int k = threadIdx.x; k < n; k += POSE_BLOCK) acc += partial[k];
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (int w = POSE_BLOCK / 2; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *prior_value = s_sum[0];
}

// thread (u, b, c): element c of the correction of bone b of listed frame u, rotation vector and translation; the arithmetic
// of k_sg_adam (torch.optim.SparseAdam), no clamp (pose_adam_one, pose_adam.h: shared with fk.hip)
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
        hipLaunchKernelGGL(k_pose_backward<false>, dim3((n + POSE_BLOCK - 1) / POSE_BLOCK), dim3(POSE_BLOCK), 0, stream, V, B, F, U,
                           frames_listed, view_rows, frame_of_view, posed, rest, rotvec, d_transforms, d_rotvec, d_trans, PosePrior{});
    }
    MGR_LAUNCH_CHECK("k_pose_backward", stream, 0);
    return MGR_OK;
}

extern "C" size_t mgr_pose_prior_workspace_bytes(int U, int B) {
    return (U < 1 || B < 1) ? 0 : (size_t)U * (size_t)B * sizeof(double);
}

extern "C" int mgr_pose_backward_prior(int V, int B, int F, int U, const int32_t* frames_listed, const int32_t* view_rows,
                                       const int32_t* frame_of_view, const float* posed, const float* rest, const float* rotvec,
                                       const float* trans, const float* d_transforms, float* d_rotvec, float* d_trans,
                                       const int32_t* neighbours, double w_mag_rot, double w_smooth_rot, double w_mag_trans,
                                       double w_smooth_trans, double* prior_value, void* workspace, size_t workspace_bytes,
                                       void* stream_) {
    if (V < 1 || B < 1 || B > MGR_MAX_BONES || F < 1 || U < 1)
        return mgr_fail(MGR_EINVAL, "mgr_pose_backward_prior: V, F and U must be at least 1, B 1 .. MGR_MAX_BONES");
    if (!frames_listed || !view_rows || !frame_of_view || !posed || !rest || !rotvec || !trans || !d_transforms || !d_rotvec || !d_trans)
        return mgr_fail(MGR_EINVAL, "mgr_pose_backward_prior: null pointer");
    if ((long long)V * (B + 1) > (1ll << 24) || (long long)U * B > (1ll << 24))
        return mgr_fail(MGR_EINVAL, "mgr_pose_backward_prior: V * (B + 1) or U * B above 2^24");
    const double w[4] = {w_mag_rot, w_smooth_rot, w_mag_trans, w_smooth_trans};
    for (int i = 0; i < 4; ++i)
        if (!(w[i] >= 0.0) || !std::isfinite(w[i]))
            return mgr_fail(MGR_EINVAL, "mgr_pose_backward_prior: the weights must be finite and >= 0");
    const bool smooth = w_smooth_rot != 0.0 || w_smooth_trans != 0.0;
    const bool prior = smooth || w_mag_rot != 0.0 || w_mag_trans != 0.0;
    if (smooth && !neighbours) return mgr_fail(MGR_EINVAL, "mgr_pose_backward_prior: a smoothness weight needs the neighbour table");
    if (prior && (!prior_value || !workspace))
        return mgr_fail(MGR_EINVAL, "mgr_pose_backward_prior: a prior needs prior_value and a workspace");
    if (prior && workspace_bytes < mgr_pose_prior_workspace_bytes(U, B))
        return mgr_fail(MGR_ENOMEM, "mgr_pose_backward_prior: workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    const int n = U * B;
    if (!prior) {      // mgr_pose_backward's own launch; the value of no prior is 0
        if (prior_value) MGR_HIP(hipMemsetAsync(prior_value, 0, sizeof(double), stream));
        {
            MGR_PROF("k_pose_backward", stream);
            hipLaunchKernelGGL(k_pose_backward<false>, dim3((n + POSE_BLOCK - 1) / POSE_BLOCK), dim3(POSE_BLOCK), 0, stream, V, B, F, U,
                               frames_listed, view_rows, frame_of_view, posed, rest, rotvec, d_transforms, d_rotvec, d_trans, PosePrior{});
        }
        MGR_LAUNCH_CHECK("k_pose_backward", stream, 0);
        return MGR_OK;
    }
    double* partial = (double*)workspace;
    const PosePrior pr = {trans, neighbours, partial, w_mag_rot, w_smooth_rot, w_mag_trans, w_smooth_trans, (float)(2.0 * w_mag_rot),
                          (float)(2.0 * w_smooth_rot), (float)(2.0 * w_mag_trans), (float)(2.0 * w_smooth_trans)};
    {
        MGR_PROF("k_pose_backward_prior", stream);
        hipLaunchKernelGGL(k_pose_backward<true>, dim3((n + POSE_BLOCK - 1) / POSE_BLOCK), dim3(POSE_BLOCK), 0, stream, V, B, F, U,
                           frames_listed, view_rows, frame_of_view, posed, rest, rotvec, d_transforms, d_rotvec, d_trans, pr);
    }
    MGR_LAUNCH_CHECK("k_pose_backward_prior", stream, 0);
    {
        MGR_PROF("k_pose_prior_fold", stream);
        hipLaunchKernelGGL(k_pose_prior_fold, dim3(1), dim3(POSE_BLOCK), 0, stream, partial, n, prior_value);
    }
    MGR_LAUNCH_CHECK("k_pose_prior_fold", stream, 0);
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
