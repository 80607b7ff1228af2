// Per-camera exposure: a learnt affine colour transform between the render and the image loss.
//
//   E (C,3,4) fp32, one row per camera: A = E[:, :, :3], b = E[:, :, 3].  View k uses the row r = cam_of_view[k]:
//     out'[k,c,p] = ((A[r,c,0] img[k,0,p] + A[r,c,1] img[k,1,p]) + A[r,c,2] img[k,2,p]) + b[r,c]          (mgr_exposure_apply)
//     g[k,j,p]    = (A[r,0,j] g'[k,0,p] + A[r,1,j] g'[k,1,p]) + A[r,2,j] g'[k,2,p]                        (mgr_exposure_backward)
//     dE[k,c,j]   = sum_p g'[k,c,p] img[k,j,p]   (j < 3),      dE[k,c,3] = sum_p g'[k,c,p]
//   r outside [0,C): the view is not corrected -- out' = img and g = g' bit for bit, dE[k] = 0.
// fp32, written in that order without contraction, so that a restatement in fp32 rounds the same way.
//
// No reference counterpart (brown-ivl/manus trains on the captured colours as they are); the definition is the per-image
// affine transform of upstream 3DGS' exposure option.
//
// Both image kernels are streaming kernels: planar (V,3,H,W), one grid row per view, EXP_BLOCK pixels per workgroup in a fixed
// assignment, the view's 12 coefficients wave-uniform (scalar loads).  VW = 4: 16-byte loads and stores, taken when H W is a
// multiple of 4 and the buffers are 16-byte aligned (then every plane is); VW = 1: the same walk one float at a time.  Nothing is
// read or written beyond H W.
//
// k_exposure_backward forms the 12 sums of its pixels in the same pass: products in fp32, added in fp64, per thread in
// ascending pixel order, across the wave by a fixed shuffle tree, across the four waves through LDS in wave order -- one record
// of 12 doubles per workgroup.  k_exposure_fold (one workgroup per view) adds the view's records in a fixed order.  No atomics:
// equal bits run to run (the convention of mgr_map_loss and mgr_pose_backward_prior).  A term that is not finite makes the
// whole dE[k] NaN; the records of the other views never see it.
#include "mgr_common.h"
#include "pose_adam.h"

#include <cmath>

#define EXP_T 256
#define EXP_PER 16
#define EXP_BLOCK (EXP_T * EXP_PER)
#define EXP_WAVES (EXP_T / MGR_WAVE)

template <int VW>
struct ExpVec {
    float v[VW];
};

template <int VW>
__device__ __forceinline__ ExpVec<VW> exp_ld(const float* p) {
    ExpVec<VW> r;
    if constexpr (VW == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}

template <int VW>
__device__ __forceinline__ void exp_st(float* p, const ExpVec<VW>& r) {
    if constexpr (VW == 4) *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else *p = r.v[0];
}

// the row of view k (wave-uniform: scalar loads); false: no correction
__device__ __forceinline__ bool exp_coef(const int32_t* __restrict__ cam_of_view, const float* __restrict__ E, int C, int k, float a[12]) {
    const int r = cam_of_view[k];
    if (r < 0 || r >= C) return false;
    const float* e = E + (size_t)r * 12;
#pragma unroll
    for (int i = 0; i < 12; ++i) a[i] = e[i];
    return true;
}

__device__ __forceinline__ float exp_dot3(float a0, float a1, float a2, float x, float y, float z) {
#pragma clang fp contract(off)
    return (a0 * x + a1 * y) + a2 * z;
}

template <int VW>
__global__ __launch_bounds__(EXP_T) void k_exposure_apply(int HW, int C, const int32_t* __restrict__ cam_of_view,
                                                         const float* __restrict__ E, const float* __restrict__ img,
                                                         float* __restrict__ out) {
    constexpr int UNITS = EXP_PER / VW, BATCH = VW == 4 ? 2 : 4;
    const int k = blockIdx.y, tid = threadIdx.x;
    float a[12];
    const bool on = exp_coef(cam_of_view, E, C, k, a);
    const size_t vo = (size_t)k * 3 * (size_t)HW;
    const float *x_ = img + vo, *y_ = x_ + HW, *z_ = y_ + HW;
    float *o0 = out + vo, *o1 = o0 + HW, *o2 = o1 + HW;
    const long long u0 = (long long)blockIdx.x * (EXP_BLOCK / VW) + tid;
#pragma unroll
    for (int kk = 0; kk < UNITS; kk += BATCH) {
        ExpVec<VW> x[BATCH], y[BATCH], z[BATCH];
        long long p[BATCH];
#pragma unroll
        for (int b = 0; b < BATCH; ++b) {
            p[b] = (u0 + (long long)(kk + b) * EXP_T) * VW;
            if (p[b] < HW) {
                x[b] = exp_ld<VW>(x_ + p[b]);
                y[b] = exp_ld<VW>(y_ + p[b]);
                z[b] = exp_ld<VW>(z_ + p[b]);
            }
        }
#pragma unroll
        for (int b = 0; b < BATCH; ++b) {
            if (p[b] >= HW) continue;
            if (on) {
#pragma clang fp contract(off)
                ExpVec<VW> r0, r1, r2;
#pragma unroll
                for (int i = 0; i < VW; ++i) {
                    r0.v[i] = exp_dot3(a[0], a[1], a[2], x[b].v[i], y[b].v[i], z[b].v[i]) + a[3];
                    r1.v[i] = exp_dot3(a[4], a[5], a[6], x[b].v[i], y[b].v[i], z[b].v[i]) + a[7];
                    r2.v[i] = exp_dot3(a[8], a[9], a[10], x[b].v[i], y[b].v[i], z[b].v[i]) + a[11];
                }
                exp_st<VW>(o0 + p[b], r0);
                exp_st<VW>(o1 + p[b], r1);
                exp_st<VW>(o2 + p[b], r2);
            } else {
                exp_st<VW>(o0 + p[b], x[b]);
                exp_st<VW>(o1 + p[b], y[b]);
                exp_st<VW>(o2 + p[b], z[b]);
            }
        }
    }
}

// 12 sums of the workgroup: the wave's by a fixed shuffle tree (lane 0 holds the total), then s_red[wave][i]; the caller adds
// the EXP_WAVES rows in wave order behind the barrier
__device__ __forceinline__ void exp_block_reduce(double acc[12], double (*s_red)[12], int tid) {
#pragma unroll
    for (int i = 0; i < 12; ++i) {
#pragma unroll
        for (int off = MGR_WAVE / 2; off > 0; off >>= 1) acc[i] += __shfl_down(acc[i], off, MGR_WAVE);
    }
    if ((tid & (MGR_WAVE - 1)) == 0) {
#pragma unroll
        for (int i = 0; i < 12; ++i) s_red[tid / MGR_WAVE][i] = acc[i];
    }
    __syncthreads();
}

__device__ __forceinline__ double exp_term(float t) {
    return (double)((fabsf(t) <= 3.402823466e38f) ? t : __int_as_float(0x7FC00000));      // (NaN and infinity fail the comparison)
}

// g_out may be g_in: every thread reads the elements it writes before it writes them, and no other thread touches them
template <int VW>
__global__ __launch_bounds__(EXP_T) void k_exposure_backward(int HW, int C, const int32_t* __restrict__ cam_of_view,
                                                            const float* __restrict__ E, const float* __restrict__ img,
                                                            const float* g_in, float* g_out, double* __restrict__ part) {
    constexpr int UNITS = EXP_PER / VW, BATCH = VW == 4 ? 2 : 4;
    __shared__ double s_red[EXP_WAVES][12];
    const int k = blockIdx.y, tid = threadIdx.x;
    float a[12];
    const bool on = exp_coef(cam_of_view, E, C, k, a);
    const size_t vo = (size_t)k * 3 * (size_t)HW;
    const float *x_ = img + vo, *y_ = x_ + HW, *z_ = y_ + HW;
    const float *g0_ = g_in + vo, *g1_ = g0_ + HW, *g2_ = g1_ + HW;
    float *o0 = g_out + vo, *o1 = o0 + HW, *o2 = o1 + HW;
    const long long u0 = (long long)blockIdx.x * (EXP_BLOCK / VW) + tid;
    if (!on) {      // the whole workgroup: g = g' (nothing to do in place), no record (k_exposure_fold writes the zeros)
        if (g_out == g_in) return;
#pragma unroll
        for (int kk = 0; kk < UNITS; ++kk) {
            const long long p = (u0 + (long long)kk * EXP_T) * VW;
            if (p >= HW) continue;
            const ExpVec<VW> g0 = exp_ld<VW>(g0_ + p), g1 = exp_ld<VW>(g1_ + p), g2 = exp_ld<VW>(g2_ + p);
            exp_st<VW>(o0 + p, g0);
            exp_st<VW>(o1 + p, g1);
            exp_st<VW>(o2 + p, g2);
        }
        return;
    }
    double acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 0.0;
#pragma unroll
    for (int kk = 0; kk < UNITS; kk += BATCH) {
        ExpVec<VW> x[BATCH], y[BATCH], z[BATCH], g0[BATCH], g1[BATCH], g2[BATCH];
        long long p[BATCH];
#pragma unroll
        for (int b = 0; b < BATCH; ++b) {
            p[b] = (u0 + (long long)(kk + b) * EXP_T) * VW;
            if (p[b] < HW) {
                x[b] = exp_ld<VW>(x_ + p[b]);
                y[b] = exp_ld<VW>(y_ + p[b]);
                z[b] = exp_ld<VW>(z_ + p[b]);
                g0[b] = exp_ld<VW>(g0_ + p[b]);
                g1[b] = exp_ld<VW>(g1_ + p[b]);
                g2[b] = exp_ld<VW>(g2_ + p[b]);
            }
        }
#pragma unroll
        for (int b = 0; b < BATCH; ++b) {
            if (p[b] >= HW) continue;
            ExpVec<VW> r0, r1, r2;
#pragma unroll
            for (int i = 0; i < VW; ++i) {
#pragma clang fp contract(off)
                const float xi = x[b].v[i], yi = y[b].v[i], zi = z[b].v[i];
                const float ga = g0[b].v[i], gb = g1[b].v[i], gc = g2[b].v[i];
                r0.v[i] = exp_dot3(a[0], a[4], a[8], ga, gb, gc);
                r1.v[i] = exp_dot3(a[1], a[5], a[9], ga, gb, gc);
                r2.v[i] = exp_dot3(a[2], a[6], a[10], ga, gb, gc);
                acc[0] += exp_term(ga * xi); acc[1] += exp_term(ga * yi); acc[2] += exp_term(ga * zi); acc[3] += exp_term(ga);
                acc[4] += exp_term(gb * xi); acc[5] += exp_term(gb * yi); acc[6] += exp_term(gb * zi); acc[7] += exp_term(gb);
                acc[8] += exp_term(gc * xi); acc[9] += exp_term(gc * yi); acc[10] += exp_term(gc * zi); acc[11] += exp_term(gc);
            }
            exp_st<VW>(o0 + p[b], r0);
            exp_st<VW>(o1 + p[b], r1);
            exp_st<VW>(o2 + p[b], r2);
        }
    }
    exp_block_reduce(acc, s_red, tid);
    if (tid < 12) {
        double t = s_red[0][tid];
#pragma unroll
        for (int w = 1; w < EXP_WAVES; ++w) t += s_red[w][tid];
        part[((size_t)k * gridDim.x + blockIdx.x) * 12 + tid] = t;
    }
}

// one workgroup per view: thread t adds the records t, t + EXP_T, ... in ascending order, then the tree of k_exposure_backward
__global__ __launch_bounds__(EXP_T) void k_exposure_fold(int nb, int C, const int32_t* __restrict__ cam_of_view,
                                                        const double* __restrict__ part, float* __restrict__ dE) {
    __shared__ double s_red[EXP_WAVES][12];
    __shared__ double s_tot[12];
    const int k = blockIdx.x, tid = threadIdx.x;
    const int r = cam_of_view[k];
    if (r < 0 || r >= C) {
        if (tid < 12) dE[(size_t)k * 12 + tid] = 0.0f;
        return;
    }
    double acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 0.0;
    const double* rec = part + (size_t)k * nb * 12;
    for (int b = tid; b < nb; b += EXP_T) {
#pragma unroll
        for (int i = 0; i < 12; ++i) acc[i] += rec[(size_t)b * 12 + i];
    }
    exp_block_reduce(acc, s_red, tid);
    if (tid < 12) {
        double t = s_red[0][tid];
#pragma unroll
        for (int w = 1; w < EXP_WAVES; ++w) t += s_red[w][tid];
        s_tot[tid] = t;
    }
    __syncthreads();
    if (tid < 12) {
        bool bad = false;
#pragma unroll
        for (int i = 0; i < 12; ++i) bad = bad || !(fabs(s_tot[i]) <= 1.7976931348623157e308);
        dE[(size_t)k * 12 + tid] = bad ? __int_as_float(0x7FC00000) : (float)s_tot[tid];
    }
}

// thread (u, e): element e of the (3,4) row of listed camera u; its gradient is the sum of the rows dE[k] of the positions that
// use the camera, in ascending k; the update is pose_adam_one (torch.optim.SparseAdam, no clamp)
__global__ __launch_bounds__(EXP_T) void k_exposure_adam(int C, int U, const int32_t* __restrict__ cams_listed, int V,
                                                        const int32_t* __restrict__ cam_of_view, const float* __restrict__ dE,
                                                        float* __restrict__ E, float* __restrict__ m, float* __restrict__ v,
                                                        float step_size, float omb1, float omb2, float eps) {
    const int gid = blockIdx.x * EXP_T + threadIdx.x;
    if (gid >= U * 12) return;
    const int u = gid / 12, e = gid - u * 12;
    const int c = cams_listed[u];
    if (c < 0 || c >= C) return;
    float g = 0.0f;
    for (int k = 0; k < V; ++k)
        if (cam_of_view[k] == c) g += dE[(size_t)k * 12 + e];
    const size_t o = (size_t)c * 12 + e;
    pose_adam_one(g, E + o, m + o, v + o, step_size, omb1, omb2, eps);
}

// ---------------------------------------------------------------------------
// host entries: every refusal is decided on the arguments, before any launch
// ---------------------------------------------------------------------------
extern "C" int mgr_exposure_block(void) { return EXP_BLOCK; }

static long long exp_blocks(int H, int W) { return ((long long)H * W + EXP_BLOCK - 1) / EXP_BLOCK; }

static const char* exp_sizes(int V, int H, int W, int C) {
    if (V < 1 || H < 1 || W < 1 || C < 1) return "V, H, W and C must be at least 1";
    if (V > 65535) return "more than 65535 views";
    if ((long long)H * W > 0x7FFFFFFFll - EXP_BLOCK) return "image too large";
    return nullptr;
}

static bool exp_vec_ok(int HW, const void* a, const void* b, const void* c) {
    return HW % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

extern "C" size_t mgr_exposure_workspace_bytes(int V, int H, int W) {
    if (V < 1 || H < 1 || W < 1) return 0;
    return mgr_align((size_t)V * (size_t)exp_blocks(H, W) * 12 * sizeof(double));
}

extern "C" int mgr_exposure_apply(int V, int H, int W, int C, const int32_t* cam_of_view, const float* E, const float* img, float* out,
                                  void* stream_) {
    if (const char* why = exp_sizes(V, H, W, C)) return mgr_fail(MGR_EINVAL, "mgr_exposure_apply: %s", why);
    if (!cam_of_view || !E || !img || !out) return mgr_fail(MGR_EINVAL, "mgr_exposure_apply: null pointer");
    if (out == img) return mgr_fail(MGR_EINVAL, "mgr_exposure_apply: out may not alias img");
    hipStream_t stream = (hipStream_t)stream_;
    const int HW = H * W;
    const dim3 grid((unsigned)exp_blocks(H, W), (unsigned)V);
    {
        MGR_PROF("k_exposure_apply", stream);
        if (exp_vec_ok(HW, img, out, out))
            hipLaunchKernelGGL(k_exposure_apply<4>, grid, dim3(EXP_T), 0, stream, HW, C, cam_of_view, E, img, out);
        else
            hipLaunchKernelGGL(k_exposure_apply<1>, grid, dim3(EXP_T), 0, stream, HW, C, cam_of_view, E, img, out);
    }
    MGR_LAUNCH_CHECK("k_exposure_apply", stream, 0);
    return MGR_OK;
}

extern "C" int mgr_exposure_backward(int V, int H, int W, int C, const int32_t* cam_of_view, const float* E, const float* img,
                                     const float* g_in, float* g_out, float* dE, void* workspace, size_t workspace_bytes,
                                     void* stream_) {
    if (const char* why = exp_sizes(V, H, W, C)) return mgr_fail(MGR_EINVAL, "mgr_exposure_backward: %s", why);
    if (!cam_of_view || !E || !img || !g_in || !g_out || !dE || !workspace)
        return mgr_fail(MGR_EINVAL, "mgr_exposure_backward: null pointer");
    if (g_out == img) return mgr_fail(MGR_EINVAL, "mgr_exposure_backward: g_out may not alias img");
    if (workspace_bytes < mgr_exposure_workspace_bytes(V, H, W))
        return mgr_fail(MGR_ENOMEM, "mgr_exposure_backward: workspace smaller than mgr_exposure_workspace_bytes");
    hipStream_t stream = (hipStream_t)stream_;
    const int HW = H * W, nb = (int)exp_blocks(H, W);
    const dim3 grid((unsigned)nb, (unsigned)V);
    double* part = (double*)workspace;
    {
        MGR_PROF("k_exposure_backward", stream);
        if (exp_vec_ok(HW, img, g_in, g_out))
            hipLaunchKernelGGL(k_exposure_backward<4>, grid, dim3(EXP_T), 0, stream, HW, C, cam_of_view, E, img, g_in, g_out, part);
        else
            hipLaunchKernelGGL(k_exposure_backward<1>, grid, dim3(EXP_T), 0, stream, HW, C, cam_of_view, E, img, g_in, g_out, part);
    }
    MGR_LAUNCH_CHECK("k_exposure_backward", stream, 0);
    {
        MGR_PROF("k_exposure_fold", stream);
        hipLaunchKernelGGL(k_exposure_fold, dim3((unsigned)V), dim3(EXP_T), 0, stream, nb, C, cam_of_view, (const double*)part, dE);
    }
    MGR_LAUNCH_CHECK("k_exposure_fold", stream, 0);
    return MGR_OK;
}

extern "C" int mgr_exposure_adam(int C, int U, const int32_t* cams_listed, int V, const int32_t* cam_of_view, const float* dE, float* E,
                                 float* m, float* v, double lr, double beta1, double beta2, double eps, int step, void* stream_) {
    if (C < 1 || U < 1 || V < 1) return mgr_fail(MGR_EINVAL, "mgr_exposure_adam: C, U and V must be at least 1");
    if (step < 1) return mgr_fail(MGR_EINVAL, "mgr_exposure_adam: step < 1");
    if (!std::isfinite(lr)) return mgr_fail(MGR_EINVAL, "mgr_exposure_adam: the rate must be finite");
    if (!cams_listed || !cam_of_view || !dE || !E || !m || !v) return mgr_fail(MGR_EINVAL, "mgr_exposure_adam: null pointer");
    if ((long long)U * 12 > (1ll << 24)) return mgr_fail(MGR_EINVAL, "mgr_exposure_adam: U above 2^24 / 12");
    hipStream_t stream = (hipStream_t)stream_;
    // the bias corrections of the global step, in double as torch takes them (mgr_pose_adam)
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    const double k = sqrt(bc2) / bc1;
    const int n = U * 12;
    {
        MGR_PROF("k_exposure_adam", stream);
        hipLaunchKernelGGL(k_exposure_adam, dim3((n + EXP_T - 1) / EXP_T), dim3(EXP_T), 0, stream, C, U, cams_listed, V, cam_of_view, dE, E, m,
                           v, (float)(lr * k), (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps);
    }
    MGR_LAUNCH_CHECK("k_exposure_adam", stream, 0);
    return MGR_OK;
}
