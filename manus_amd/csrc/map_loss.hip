// Map loss: the silhouette and depth terms on the maps of the feature render (mgr_raster_blend_features), value and gradient in
// one streaming pass (mgr_map_loss).
//
//   L_mask  = mean over V H W of |alpha - mask|
//   L_depth = mean over V H W of mask |depth - depth_target|          (depth: the EXPECTED depth sum_i w_i z_i, background 0)
//   dL/dalpha = grad_scale w_mask  sign(alpha - mask) / (V H W)
//   dL/ddepth = grad_scale w_depth mask sign(depth - depth_target) / (V H W)         sign(0) = 0
//
// No reference counterpart: brown-ivl/manus uses its segmentation masks for pruning only (get_points_outside_mask).
//
// k_map_loss: workgroup b takes the elements [b * ML_CHUNK, (b + 1) * ML_CHUNK) -- a fixed assignment, nothing is queued --,
// every thread adds its ML_PER terms in fp64 in ascending order, the workgroup folds its 256 sums over a fixed LDS tree and
// writes ONE fp64 pair to its slot of the caller's workspace.  k_map_loss_fold (one workgroup): thread t adds the slots t,
// t + 256, ... in ascending order, the same tree, three floats out.  No atomics, every order fixed by the sizes alone: the sums
// are bit-reproducible, and fp64 sums of fp32 terms are exact to ~1e-16 relative per addition.  A term that is not finite makes
// its sum (and the weighted sum) NaN, as k_image_loss reports a sum it cannot represent.
#include "mgr_common.h"

#define ML_T 256
#define ML_PER 16
#define ML_CHUNK (ML_T * ML_PER)

__device__ __forceinline__ double2 ml_block_sum(double a, double b, double2* s_red, int tid) {
    s_red[tid] = make_double2(a, b);
    __syncthreads();
#pragma unroll
    for (int h = ML_T / 2; h > 0; h >>= 1) {
        if (tid < h) {
            const double2 x = s_red[tid], y = s_red[tid + h];
            s_red[tid] = make_double2(x.x + y.x, x.y + y.y);
        }
        __syncthreads();
    }
    return s_red[0];
}

__global__ __launch_bounds__(ML_T) void k_map_loss(long long n, const float* __restrict__ alpha, const float* __restrict__ mask,
                                                   const float* __restrict__ depth, const float* __restrict__ depth_target,
                                                   float ca, float cd, float* __restrict__ dL_dalpha,
                                                   float* __restrict__ dL_ddepth, double2* __restrict__ part) {
    __shared__ double2 s_red[ML_T];
    const int tid = threadIdx.x;
    const long long base = (long long)blockIdx.x * ML_CHUNK;
    const float qnan = __int_as_float(0x7FC00000);
    double lm = 0.0, ld = 0.0;
#pragma unroll 4
    for (int k = 0; k < ML_PER; ++k) {
        const long long e = base + (long long)k * ML_T + tid;
        if (e >= n) break;
        const float m = mask[e];
        {
            const float d = alpha[e] - m;
            const float t = fabsf(d);
            lm += (double)((t <= 3.402823466e38f) ? t : qnan);          // (NaN and infinity fail the comparison)
            dL_dalpha[e] = ca * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
        }
        if (depth) {
            const float d = depth[e] - depth_target[e];
            const float t = m * fabsf(d);
            ld += (double)((t <= 3.402823466e38f) ? t : qnan);
            dL_ddepth[e] = (cd * m) * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
        }
    }
    const double2 tot = ml_block_sum(lm, ld, s_red, tid);
    if (tid == 0) part[blockIdx.x] = tot;
}

__global__ __launch_bounds__(ML_T) void k_map_loss_fold(int nb, const double2* __restrict__ part, double inv_n, float w_mask,
                                                        float w_depth, float* __restrict__ sums) {
    __shared__ double2 s_red[ML_T];
    const int tid = threadIdx.x;
    double lm = 0.0, ld = 0.0;
    for (int k = tid; k < nb; k += ML_T) {
        const double2 p = part[k];
        lm += p.x;
        ld += p.y;
    }
    const double2 tot = ml_block_sum(lm, ld, s_red, tid);
    if (tid == 0) {
        const double a = tot.x * inv_n, d = tot.y * inv_n;
        sums[0] = (float)a;
        sums[1] = (float)d;
        sums[2] = (float)((double)w_mask * a + (double)w_depth * d);
    }
}

static long long ml_blocks(int V, int H, int W) { return ((long long)V * H * W + ML_CHUNK - 1) / ML_CHUNK; }

extern "C" size_t mgr_map_loss_workspace_bytes(int V, int H, int W) {
    if (V <= 0 || H <= 0 || W <= 0) return 0;
    return mgr_align((size_t)ml_blocks(V, H, W) * sizeof(double2));
}

extern "C" int mgr_map_loss(int V, int H, int W, const float* alpha, const float* mask, const float* depth,
                            const float* depth_target, float w_mask, float w_depth, float grad_scale, float* dL_dalpha,
                            float* dL_ddepth, float* sums, void* workspace, size_t workspace_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (V <= 0 || H <= 0 || W <= 0) return mgr_fail(MGR_EINVAL, "mgr_map_loss: bad sizes");
    if (!alpha || !mask || !dL_dalpha || !sums || !workspace) return mgr_fail(MGR_EINVAL, "mgr_map_loss: null pointer");
    if ((depth != nullptr) != (depth_target != nullptr) || (depth && !dL_ddepth))
        return mgr_fail(MGR_EINVAL, "mgr_map_loss: the depth term takes depth, depth_target and dL_ddepth together");
    const long long n = (long long)V * H * W, nb = ml_blocks(V, H, W);
    if (nb > 0x7FFFFFFFll) return mgr_fail(MGR_EINVAL, "mgr_map_loss: maps too large");
    if (workspace_bytes < mgr_map_loss_workspace_bytes(V, H, W))
        return mgr_fail(MGR_ENOMEM, "mgr_map_loss: workspace smaller than mgr_map_loss_workspace_bytes");
    if (!depth) w_depth = 0.0f;
    // the factors of the two gradients, rounded to fp32 once: every element is this value times its sign (and its mask)
    const float ca = (float)((double)grad_scale * (double)w_mask / (double)n);
    const float cd = (float)((double)grad_scale * (double)w_depth / (double)n);
    double2* part = (double2*)workspace;
    {
        MGR_PROF("k_map_loss", stream);
        hipLaunchKernelGGL(k_map_loss, dim3((unsigned)nb), dim3(ML_T), 0, stream, n, alpha, mask, depth, depth_target, ca, cd,
                           dL_dalpha, dL_ddepth, part);
        MGR_LAUNCH_CHECK("k_map_loss", stream, 0);
        hipLaunchKernelGGL(k_map_loss_fold, dim3(1), dim3(ML_T), 0, stream, (int)nb, (const double2*)part, 1.0 / (double)n, w_mask,
                           w_depth, sums);
        MGR_LAUNCH_CHECK("k_map_loss_fold", stream, 0);
    }
    return MGR_OK;
}
