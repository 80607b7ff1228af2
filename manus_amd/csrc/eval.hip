// Validation metrics of rendered views for gfx950: masked squared error, "SSIM" map sum, ground-truth maximum and the
// render | ground truth | difference triptych, for images kept in the rasterizer's (V,3,H,W) layout.
//
// Replaces, forward only and for V views at once,
//     render * mask, gt * mask, psnr(render, gt), ssim(render, gt)      src/modules/base.py:138-147
//     psnr                                                              src/utils/loss_utils.py:100-108
//     the triptych of validation_step                                   src/modules/base.py:116-128
//     dump_image / concat_img_array                                     src/utils/extra.py:110-115,153-160
// of brown-ivl/manus.  The SSIM statistic is the one k_image_loss (image_loss.hip) computes and its header states: the
// reference calls ssim() on HWC images, so the 11x11 window slides over the (W,3) plane of every image row, zero padded:
//     E_s[w][c] = an 11-tap filter along w of the channel mix  sum_c' g[5+c'-c] s[w][c'],   s in {x, y, xx, yy, xy},
// here of the MASKED images x = pred * mask, y = target * mask.  There is no backward: no derivative maps, no gradient.
//
// k_eval_views: one 128-thread workgroup owns 256 consecutive w of TWO image rows (the two rows are the halves of packed
// fp32 registers, every filter tap one v_pk_fma_f32, each thread produces two neighbouring positions from a sliding
// window of 12 LDS reads -- the staging of k_image_loss without its derivative halo: 266 staged positions for 256
// outputs).  The pass that stages the channel mixes also takes the squared error, the maximum of the unmasked target
// and the "is anything not finite" test of the positions the workgroup owns.  Every workgroup writes ONE record
// (sq, ssim, max, flag); k_eval_fold adds the records of a view in a fixed order in fp64.  No atomics at all: two calls
// on the same inputs give the same bits, and a view's results depend on that view's pixels only.
#include "mgr_common.h"

#define EV_T 128                    // threads of k_eval_views
#define EV_W (2 * EV_T)             // 256 outputs per workgroup and row, two per thread
#define EV_H 5                      // half window
#define EV_NX (EV_W + 2 * EV_H)     // 266 staged positions
#define EV_MAXW 16384               // the width limit of mgr_image_loss
#define EVF_T 256                   // threads of k_eval_fold
#define EVT_T 256                   // threads of k_eval_triptych

struct EvWindow {
    float g[11];
};
struct __attribute__((aligned(16))) EvPartial {   // one per workgroup of k_eval_views
    float sq, ssim, gt_max;
    uint32_t bad;
};

typedef mgr_v2f ev2f;
__device__ __forceinline__ ev2f ev_v2(float a) { ev2f r = {a, a}; return r; }
__device__ __forceinline__ bool ev_nonfinite(float a) { return (__float_as_uint(a) & 0x7F800000u) == 0x7F800000u; }
// maximum that keeps a NaN once it has seen one (numpy's ndarray.max, which dump_image asks)
__device__ __forceinline__ float ev_max_nan(float a, float b) { return (b > a || b != b) ? b : a; }

// (pred * mask) - (target * mask): two rounded products and one rounded difference, as `render * mask`, `gt * mask` and
// `inputs - targets` are three torch kernels -- never a fused multiply-add, so that equal masked images differ by exactly 0
__device__ __forceinline__ void ev_masked(float p, float t, float m, float& x, float& y, float& d) {
#pragma clang fp contract(off)
    x = p * m;
    y = t * m;
    d = x - y;
}

__global__ __launch_bounds__(EV_T) void k_eval_views(int H, int W, const float* __restrict__ pred, const float* __restrict__ target,
                                                     const float* __restrict__ mask, EvWindow win, EvPartial* __restrict__ partial) {
    // channel-mixed statistics (5 x 3 rows of positions); .x = image row h0, .y = image row h0 + 1
    __shared__ ev2f s_mix[5][3][EV_NX];
    __shared__ float s_red[3][EV_T / 64];
    const int tid = threadIdx.x;
    const int v = blockIdx.z, h0 = blockIdx.y * 2, w0 = blockIdx.x * EV_W;
    const bool row1 = h0 + 1 < H;
    const size_t plane = (size_t)H * W;
    const float* px = pred + (size_t)v * 3 * plane + (size_t)h0 * W;
    const float* py = target + (size_t)v * 3 * plane + (size_t)h0 * W;
    const float* pm = mask ? mask + (size_t)v * plane + (size_t)h0 * W : nullptr;
    // channel mix matrix M[c][c'] = g[5 + c' - c]; g is symmetric
    const ev2f m0 = ev_v2(win.g[5]), m1 = ev_v2(win.g[4]), m2 = ev_v2(win.g[3]);

    ev2f sq_acc = ev_v2(0.f);
    float gmax = -INFINITY;
    bool bad = false;
    for (int t = tid; t < EV_NX; t += EV_T) {
        const int w = w0 - EV_H + t;
        ev2f x[3], y[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] = y[c] = ev_v2(0.f);
        if (w >= 0 && w < W) {
            const bool own = t >= EV_H && t < EV_H + EV_W;     // (the halo positions belong to the neighbouring workgroups)
            const float ma = pm ? pm[w] : 1.f, mb = (pm && row1) ? pm[W + w] : 1.f;
            if (own) bad |= ev_nonfinite(ma) || ev_nonfinite(mb);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float pa = px[c * plane + w], ta = py[c * plane + w];
                float xm, ym, d;
                ev_masked(pa, ta, ma, xm, ym, d);
                x[c].x = xm; y[c].x = ym;
                if (own) {
                    sq_acc.x += d * d;
                    gmax = ev_max_nan(gmax, ta);
                    bad |= ev_nonfinite(pa) || ev_nonfinite(ta);
                }
                if (row1) {
                    const float pb = px[c * plane + W + w], tb = py[c * plane + W + w];
                    ev_masked(pb, tb, mb, xm, ym, d);
                    x[c].y = xm; y[c].y = ym;
                    if (own) {
                        sq_acc.y += d * d;
                        gmax = ev_max_nan(gmax, tb);
                        bad |= ev_nonfinite(pb) || ev_nonfinite(tb);
                    }
                }
            }
        }
        const ev2f q[5][3] = {{x[0], x[1], x[2]},
                              {y[0], y[1], y[2]},
                              {x[0] * x[0], x[1] * x[1], x[2] * x[2]},
                              {y[0] * y[0], y[1] * y[1], y[2] * y[2]},
                              {x[0] * y[0], x[1] * y[1], x[2] * y[2]}};
#pragma unroll
        for (int s5 = 0; s5 < 5; ++s5) {
            s_mix[s5][0][t] = m0 * q[s5][0] + m1 * q[s5][1] + m2 * q[s5][2];
            s_mix[s5][1][t] = m1 * q[s5][0] + m0 * q[s5][1] + m1 * q[s5][2];
            s_mix[s5][2][t] = m2 * q[s5][0] + m1 * q[s5][1] + m0 * q[s5][2];
        }
    }
    __syncthreads();

    // statistics -> SSIM value at the two positions u0, u0 + 1 (w = w0 + u; taps at staged positions u .. u + 10)
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const int u0 = 2 * tid;
    ev2f ssim_acc = ev_v2(0.f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        ev2f e[2][5];
#pragma unroll
        for (int s5 = 0; s5 < 5; ++s5) {
            ev2f win12[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) win12[k] = s_mix[s5][c][u0 + k];   // (u0 + 11 <= EV_NX - 1)
            ev2f a = ev_v2(0.f), b = ev_v2(0.f);
#pragma unroll
            for (int i = 0; i < 11; ++i) {
                const ev2f gi = ev_v2(win.g[i]);
                a += gi * win12[i];
                b += gi * win12[i + 1];
            }
            e[0][s5] = a;
            e[1][s5] = b;
        }
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
            const int w = w0 + u0 + pp;
            const ev2f mu1 = e[pp][0], mu2 = e[pp][1];
            const ev2f s11 = e[pp][2] - mu1 * mu1, s22 = e[pp][3] - mu2 * mu2, s12 = e[pp][4] - mu1 * mu2;
            const ev2f A = 2.f * mu1 * mu2 + C1, B = 2.f * s12 + C2;
            const ev2f Cc = mu1 * mu1 + mu2 * mu2 + C1, Dd = s11 + s22 + C2;
            ev2f iC, iD;
            iC.x = __builtin_amdgcn_rcpf(Cc.x); iC.y = __builtin_amdgcn_rcpf(Cc.y);  // 1 ulp, as k_image_loss
            iD.x = __builtin_amdgcn_rcpf(Dd.x); iD.y = __builtin_amdgcn_rcpf(Dd.y);
            const ev2f S = A * B * (iC * iD);
            if (w < W) {                 // positions outside the image have no SSIM value (a NaN there must not count either)
                ssim_acc.x += S.x;
                if (row1) ssim_acc.y += S.y;
            }
        }
    }
    // workgroup results (fixed order)
    const float sq = mgr_wave_sum63(sq_acc.x + sq_acc.y), ss = mgr_wave_sum63(ssim_acc.x + ssim_acc.y);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) gmax = ev_max_nan(gmax, __shfl_xor(gmax, o, 64));
    if ((tid & 63) == 63) {
        s_red[0][tid >> 6] = sq;
        s_red[1][tid >> 6] = ss;
        s_red[2][tid >> 6] = gmax;
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if (tid == 0) {
        EvPartial r;
        r.sq = s_red[0][0] + s_red[0][1];
        r.ssim = s_red[1][0] + s_red[1][1];
        r.gt_max = ev_max_nan(s_red[2][0], s_red[2][1]);
        r.bad = any_bad ? 1u : 0u;
        partial[((size_t)v * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = r;
    }
}

// One workgroup per view: thread i adds records i, i + 256, ... of the view in fp64, the 256 sums are added pairwise in
// LDS -- the same order every call.  A view with anything not finite in its inputs, or whose totals are not finite,
// reports NaN for both metrics and raises its flag; the other views never see its records.
__global__ __launch_bounds__(EVF_T) void k_eval_fold(int per_view, const EvPartial* __restrict__ partial, float* __restrict__ sq_sum,
                                                     float* __restrict__ ssim_sum, float* __restrict__ gt_max, int32_t* __restrict__ flags) {
    __shared__ double s_a[EVF_T], s_b[EVF_T];
    __shared__ float s_m[EVF_T];
    const int tid = threadIdx.x, v = blockIdx.x;
    const EvPartial* p = partial + (size_t)v * per_view;
    double a = 0.0, b = 0.0;
    float m = -INFINITY;
    uint32_t bad = 0;
    for (int k = tid; k < per_view; k += EVF_T) {
        const EvPartial r = p[k];
        a += (double)r.sq;
        b += (double)r.ssim;
        m = ev_max_nan(m, r.gt_max);
        bad |= r.bad;
    }
    s_a[tid] = a; s_b[tid] = b; s_m[tid] = m;
    const int any_bad = __syncthreads_or((int)bad);
    for (int n = EVF_T / 2; n >= 1; n >>= 1) {
        if (tid < n) {
            s_a[tid] += s_a[tid + n];
            s_b[tid] += s_b[tid + n];
            s_m[tid] = ev_max_nan(s_m[tid], s_m[tid + n]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        const float fa = (float)s_a[0], fb = (float)s_b[0];
        const bool nf = any_bad != 0 || ev_nonfinite(fa) || ev_nonfinite(fb);
        const float qnan = __int_as_float(0x7FC00000);
        sq_sum[v] = nf ? qnan : fa;
        ssim_sum[v] = nf ? qnan : fb;
        gt_max[v] = s_m[0];
        if (flags) flags[v] = nf ? 1 : 0;
    }
}

// float -> byte as numpy's astype(np.uint8) does on the values the reference meets: truncation toward zero, then the low
// eight bits (negative and > 255 values wrap like a C conversion through int); NaN gives 0 (OUR definition: numpy's
// result for NaN is not defined).
__device__ __forceinline__ uint32_t ev_byte(float a) { return a != a ? 0u : ((uint32_t)(int)a & 0xFFu); }
__device__ __forceinline__ uint32_t ev_render_byte(float p) {      // uint8(clamp(pred, 0, 1) * 255.0f)
    return p != p ? 0u : (uint32_t)(int)(fminf(fmaxf(p, 0.f), 1.f) * 255.0f);
}

// Four neighbouring pixels per thread when the rows allow 16-byte loads and 4-byte stores (W % 4 == 0), else one.
// out (V, 3H, W, 3): rows [0, H) the render, [H, 2H) the ground truth, [2H, 3H) the difference bytes from the table.
template <bool VEC>
__global__ __launch_bounds__(EVT_T) void k_eval_triptych(int H, int W, const float* __restrict__ pred, const float* __restrict__ target,
                                                         const float* __restrict__ gt_max, const uint8_t* __restrict__ table,
                                                         uint8_t* __restrict__ out) {
    constexpr int PX = VEC ? 4 : 1;
    const int v = blockIdx.y;
    const size_t plane = (size_t)H * W;
    const size_t q = (size_t)blockIdx.x * EVT_T + threadIdx.x;      // pixel group of the view
    if (q * PX >= plane) return;
    const float scale = gt_max[v] <= 1.0f ? 255.0f : 1.0f;          // dump_image: `if img.max() <= 1.0: img = img * 255` (a NaN maximum: no scaling)
    const float* px = pred + (size_t)v * 3 * plane + q * PX;
    const float* py = target + (size_t)v * 3 * plane + q * PX;
    float p[3][PX], t[3][PX];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if constexpr (VEC) {
            const float4 a = *(const float4*)(px + c * plane), b = *(const float4*)(py + c * plane);
            p[c][0] = a.x; p[c][1] = a.y; p[c][2] = a.z; p[c][3] = a.w;
            t[c][0] = b.x; t[c][1] = b.y; t[c][2] = b.z; t[c][3] = b.w;
        } else {
            p[c][0] = px[c * plane];
            t[c][0] = py[c * plane];
        }
    }
    uint8_t r8[3 * PX], g8[3 * PX], d8[3 * PX];
#pragma unroll
    for (int k = 0; k < PX; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t rb = ev_render_byte(p[c][k]), gb = ev_byte(t[c][k] * scale);
            r8[3 * k + c] = (uint8_t)rb;
            g8[3 * k + c] = (uint8_t)gb;
            d8[3 * k + c] = table[gb * 256u + rb];      // (gt byte, render byte) -> uint8((gt / 255.0 - img / 255.0) * 255.0), built by the host
        }
    uint8_t* o = out + (size_t)v * 9 * plane + q * PX * 3;
    if constexpr (VEC) {
        uint32_t* o0 = (uint32_t*)o;
        uint32_t* o1 = (uint32_t*)(o + 3 * plane);
        uint32_t* o2 = (uint32_t*)(o + 6 * plane);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o0[k] = (uint32_t)r8[4 * k] | ((uint32_t)r8[4 * k + 1] << 8) | ((uint32_t)r8[4 * k + 2] << 16) | ((uint32_t)r8[4 * k + 3] << 24);
            o1[k] = (uint32_t)g8[4 * k] | ((uint32_t)g8[4 * k + 1] << 8) | ((uint32_t)g8[4 * k + 2] << 16) | ((uint32_t)g8[4 * k + 3] << 24);
            o2[k] = (uint32_t)d8[4 * k] | ((uint32_t)d8[4 * k + 1] << 8) | ((uint32_t)d8[4 * k + 2] << 16) | ((uint32_t)d8[4 * k + 3] << 24);
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            o[c] = r8[c];
            o[3 * plane + c] = g8[c];
            o[6 * plane + c] = d8[c];
        }
    }
}

static int64_t ev_blocks_per_view(int H, int W) { return (int64_t)((H + 1) / 2) * ((W + EV_W - 1) / EV_W); }

extern "C" size_t mgr_eval_workspace_bytes(int V, int H, int W) {
    if (V <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)V * (size_t)ev_blocks_per_view(H, W) * sizeof(EvPartial);
}

extern "C" int mgr_eval_views(int V, int H, int W, const float* pred, const float* target, const float* mask, float* sq_sum,
                              float* ssim_sum, float* gt_max, int32_t* flags, void* workspace, size_t workspace_bytes, void* stream_) {
    if (V <= 0 || H <= 0 || W <= 0) return mgr_fail(MGR_EINVAL, "mgr_eval_views: bad sizes");
    if (!pred || !target || !sq_sum || !ssim_sum || !gt_max || !workspace) return mgr_fail(MGR_EINVAL, "mgr_eval_views: null pointer");
    if (H > 65535 || V > 65535) return mgr_fail(MGR_EINVAL, "mgr_eval_views: H and V must fit a grid dimension");
    if (W > EV_MAXW) return mgr_fail(MGR_EINVAL, "mgr_eval_views: image wider than 16384");
    if (workspace_bytes < mgr_eval_workspace_bytes(V, H, W)) return mgr_fail(MGR_ENOMEM, "mgr_eval_views: workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    // the reference's window: gaussian(11, 1.5) in fp32, normalised (loss_utils.py:38-45), as mgr_image_loss builds it
    EvWindow win;
    float sum = 0.f;
    for (int i = 0; i < 11; ++i) {
        win.g[i] = (float)exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
        sum += win.g[i];
    }
    for (int i = 0; i < 11; ++i) win.g[i] /= sum;
    const dim3 grid((W + EV_W - 1) / EV_W, (H + 1) / 2, V);
    EvPartial* partial = (EvPartial*)workspace;
    {
        MGR_PROF("k_eval_views", stream);
        hipLaunchKernelGGL(k_eval_views, grid, dim3(EV_T), 0, stream, H, W, pred, target, mask, win, partial);
    }
    MGR_LAUNCH_CHECK("k_eval_views", stream, 0);
    hipLaunchKernelGGL(k_eval_fold, dim3(V), dim3(EVF_T), 0, stream, (int)ev_blocks_per_view(H, W), (const EvPartial*)partial, sq_sum,
                       ssim_sum, gt_max, flags);
    MGR_LAUNCH_CHECK("k_eval_fold", stream, 0);
    return MGR_OK;
}

extern "C" int mgr_eval_triptych(int V, int H, int W, const float* pred, const float* target, const float* gt_max,
                                 const uint8_t* diff_table, uint8_t* out, void* stream_) {
    if (V <= 0 || H <= 0 || W <= 0) return mgr_fail(MGR_EINVAL, "mgr_eval_triptych: bad sizes");
    if (!pred || !target || !gt_max || !diff_table || !out) return mgr_fail(MGR_EINVAL, "mgr_eval_triptych: null pointer");
    if (H > 65535 || V > 65535) return mgr_fail(MGR_EINVAL, "mgr_eval_triptych: H and V must fit a grid dimension");
    if (W > EV_MAXW) return mgr_fail(MGR_EINVAL, "mgr_eval_triptych: image wider than 16384");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t plane = (size_t)H * W;
    const bool vec = (W & 3) == 0 && ((((uintptr_t)pred) | ((uintptr_t)target)) & 15) == 0 && (((uintptr_t)out) & 3) == 0;
    MGR_PROF("k_eval_triptych", stream);
    if (vec) {
        const size_t groups = plane / 4;
        hipLaunchKernelGGL(k_eval_triptych<true>, dim3((unsigned)((groups + EVT_T - 1) / EVT_T), V), dim3(EVT_T), 0, stream, H, W, pred,
                           target, gt_max, diff_table, out);
    } else {
        hipLaunchKernelGGL(k_eval_triptych<false>, dim3((unsigned)((plane + EVT_T - 1) / EVT_T), V), dim3(EVT_T), 0, stream, H, W, pred,
                           target, gt_max, diff_table, out);
    }
    MGR_LAUNCH_CHECK("k_eval_triptych", stream, 0);
    return MGR_OK;
}
