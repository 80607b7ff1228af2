// Spatial image loss for gfx950: L1 + the standard 2-D SSIM, forward and backward in one pass (mgr_image_loss2d).
//
// image_loss.hip reproduces the reference's call of ssim() on HWC images (the window slides over the (W,3) plane of every
// image row).  This file computes SSIM as published, which is what the same ssim() gives on CHW images: an 11x11 Gaussian
// window G = g g^T, g = gaussian(11, 1.5) in fp32, sliding over H x W of every colour channel separately, zero padding 5, the
// mean over all 3 H W values.  With a mask, x = pred * m and y = target * m at load.  Per channel and statistic s in
// {x, y, xx, yy, xy}
//     E_s = G * s                                                                (zero outside the image)
//     S   = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s11 + s22 + C2))
// and the backward is the same symmetric filter applied to the three derivative maps of image_loss.hip
//     D1 = dS/dmu1 (total), D2 = dS/dE[xx], D3 = dS/dE[xy],      dS/dx[p] = (G*D1)[p] + 2 x[p] (G*D2)[p] + y[p] (G*D3)[p].
//
// One 256-thread workgroup owns a block of I2_BW x I2_BH = 32 x 16 pixels of one view and goes through its three channels one
// after the other, everything in LDS (45 KB: three workgroups per CU):
//     stage x, y on the block +-10 px (52 x 36)                     -- the derivative maps are needed 5 px beyond the outputs,
//     row pass    -> the five statistics filtered along w, 42 x 36     and they need the statistics 5 px beyond that
//     column pass -> E_s on the block +-5 px (42 x 26), S and D1..D3 there (registers; zero outside the image)
//     D1..D3 -> LDS, row pass (32 x 26), column pass (32 x 16), the gradient is written.
// Every thread produces two neighbouring outputs from a sliding window of 12 LDS reads.  Only the gradient is written; there is
// no per-pixel workspace apart from ONE BIT per pixel:
//
// Settled blocks.  k_ssim2d_diff marks every pixel whose masked difference x - y is not 0 in some channel (tested as
// !(d == 0): NaN and Inf - Inf count as different); k_ssim2d_list calls a block settled when no pixel of the block dilated by
// 10 px (clipped to the image) is marked: then every statistic pair under every window that reaches the block coincides, the
// SSIM map is 1 and at its maximum there, the gradient 0.  A settled block gets zeros as its gradient and contributes exactly
// its pixel count to sum S and 0 to sum L1; only the other blocks are listed for the heavy kernel.  MGR_IL2D_DENSE lists all.
//
// Sums.  A workgroup's two sums of a block are formed in a fixed order and added as 64-bit FIXED-POINT integers (2^-32) to one
// of I2_SLOTS slots of the block's view: integer addition is associative, so the totals do not depend on the order the blocks
// were listed or run in -- two runs give equal bits, and a view's sums do not depend on the other views of the call.  A block
// sum that is not finite, or beyond 2^31 / (blocks of a view), flags its view: that view's sums, and the totals, are NaN.
#include "mgr_common.h"

#define I2_BW 32
#define I2_BH 16
#define I2_R 5
#define I2_SW (I2_BW + 4 * I2_R)    // 52 staged columns
#define I2_SH (I2_BH + 4 * I2_R)    // 36 staged rows
#define I2_MW (I2_BW + 2 * I2_R)    // 42 columns of the statistics / derivative maps
#define I2_MH (I2_BH + 2 * I2_R)    // 26 rows
#define I2_T 256
#define I2_SLOTS 16                 // sum slots per view (same-address atomics are served one after the other)
#define I2_LIST_BLOCKS 32           // blocks classified by one workgroup of k_ssim2d_list (one returning atomic each)
#define I2_GRID (256 * 3)           // persistent workgroups of k_ssim2d: three of 45 KB LDS are resident per CU

struct I2Window {
    float g[11];
};

struct I2Acc {                      // one sum slot: fixed-point sums of |x - y| and of S, listed values, flagged blocks
    long long l1, ss;
    unsigned long long px, bad;
};

__device__ __forceinline__ int64_t i2_plane(int H, int W) { return (int64_t)H * (int64_t)W; }

// Pass 1: one bit per pixel, "x - y is not 0 in some channel".  A wave takes 64 consecutive columns of one image row and writes
// the two words of its ballot: every word of the bitmap is written, nothing is cleared beforehand.
__global__ __launch_bounds__(I2_T) void k_ssim2d_diff(int H, int W, int row_words, const float* __restrict__ pred,
                                                      const float* __restrict__ target, const float* __restrict__ mask,
                                                      uint32_t* __restrict__ bitmap) {
#pragma clang fp contract(off)
    const int w = blockIdx.x * I2_T + threadIdx.x, h = blockIdx.y, v = blockIdx.z;
    const int64_t plane = i2_plane(H, W);
    bool d = false;
    if (w < W) {
        const int64_t o = (int64_t)h * W + w;
        const float m = mask ? mask[(int64_t)v * plane + o] : 1.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float x = pred[((int64_t)v * 3 + c) * plane + o], y = target[((int64_t)v * 3 + c) * plane + o];
            if (mask) {
                x *= m;
                y *= m;
            }
            const float df = x - y;
            d |= !(df == 0.f);
        }
    }
    const unsigned long long b = __builtin_amdgcn_ballot_w64(d);
    const int base = (blockIdx.x * I2_T + (threadIdx.x & ~63));      // first column of the wave
    if ((threadIdx.x & 63) == 0 && base < W) {
        uint32_t* row = bitmap + ((int64_t)v * H + h) * row_words + (base >> 5);   // base < W: both words lie inside the row's 2 * ceil(W / 64)
        row[0] = (uint32_t)b;
        row[1] = (uint32_t)(b >> 32);
    }
}

// Pass 2: a wave per block, I2_LIST_BLOCKS blocks per workgroup.  Lane r looks at row h0 - 10 + r of the dilated block.
__global__ __launch_bounds__(I2_T) void k_ssim2d_list(int H, int W, int row_words, int gxb, int gyb, uint32_t nb,
                                                      const uint32_t* __restrict__ bitmap, float* __restrict__ dL_dpred,
                                                      uint32_t* __restrict__ work_list, uint32_t* __restrict__ work_count) {
    __shared__ uint32_t s_flag[I2_LIST_BLOCKS];
    __shared__ uint32_t s_n, s_base;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t plane = i2_plane(H, W);
    constexpr int per_wave = I2_LIST_BLOCKS / (I2_T / 64);
    for (int j = 0; j < per_wave; ++j) {
        const uint32_t b = blockIdx.x * I2_LIST_BLOCKS + wv * per_wave + j;
        uint32_t entry = 0xFFFFFFFFu;
        if (b < nb) {
            const int bxi = (int)(b % (uint32_t)gxb), byi = (int)((b / (uint32_t)gxb) % (uint32_t)gyb), v = (int)(b / (uint32_t)(gxb * gyb));
            const int w0 = bxi * I2_BW, h0 = byi * I2_BH;
            const int h = h0 - 2 * I2_R + lane;
            uint32_t any = 0;
            if (lane < I2_SH && h >= 0 && h < H) {
                const int lo = max(w0 - 2 * I2_R, 0), hi = min(w0 + I2_BW + 2 * I2_R, W);   // [lo, hi), not empty: w0 < W
                const uint32_t* row = bitmap + ((int64_t)v * H + h) * row_words;
                for (int k = lo >> 5; k <= (hi - 1) >> 5; ++k) {
                    uint32_t m = row[k];
                    const int base = k << 5;
                    if (lo > base) m &= ~0u << (lo - base);
                    if (hi < base + 32) m &= ~0u >> (base + 32 - hi);
                    any |= m;
                }
            }
            if (__builtin_amdgcn_ballot_w64(any != 0)) {
                entry = b;
            } else if (dL_dpred) {      // settled: zeros as its gradient
                for (int e = lane; e < 3 * I2_BH * I2_BW; e += 64) {
                    const int c = e / (I2_BH * I2_BW), r = (e / I2_BW) % I2_BH, q = e % I2_BW;
                    if (h0 + r < H && w0 + q < W) dL_dpred[((int64_t)v * 3 + c) * plane + (int64_t)(h0 + r) * W + (w0 + q)] = 0.f;
                }
            }
        }
        if (lane == 0) s_flag[wv * per_wave + j] = entry;
    }
    __syncthreads();
    if (tid == 0) {      // the listed blocks of the workgroup take ONE slot range of the list
        uint32_t n = 0;
        for (int k = 0; k < I2_LIST_BLOCKS; ++k) {
            const uint32_t e = s_flag[k];
            if (e != 0xFFFFFFFFu) s_flag[n++] = e;      // (n <= k: in place)
        }
        s_n = n;
        s_base = n ? atomicAdd(work_count, n) : 0u;
    }
    __syncthreads();
    if (tid < (int)s_n) work_list[s_base + tid] = s_flag[tid];
}

// two neighbouring outputs a, b of the 11-tap filter from 12 values
#define I2_FILTER2(a, b, v12)                 \
    do {                                      \
        a = 0.f;                              \
        b = 0.f;                              \
        _Pragma("unroll") for (int i_ = 0; i_ < 11; ++i_) { \
            a += win.g[i_] * (v12)[i_];       \
            b += win.g[i_] * (v12)[i_ + 1];   \
        }                                     \
    } while (0)

__global__ __launch_bounds__(I2_T) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_ssim2d(int H, int W, const float* __restrict__ pred, const float* __restrict__ target,
                                                 const float* __restrict__ mask, I2Window win, float w_l1, float w_ssim,
                                                 float grad_scale, float* __restrict__ dL_dpred,
                                                 const uint32_t* __restrict__ work_list, const uint32_t* __restrict__ work_count,
                                                 int gxb, int gyb, I2Acc* __restrict__ acc, uint32_t nb, float sum_lim) {
    __shared__ __attribute__((aligned(16))) float s_x[I2_SH * I2_SW];
    __shared__ __attribute__((aligned(16))) float s_y[I2_SH * I2_SW];
    // the five row-filtered statistics [5][I2_SH][I2_MW]; later the derivative maps [3][I2_MH][I2_MW] and, behind them, their
    // row-filtered form [3][I2_MH][I2_BW]
    __shared__ __attribute__((aligned(16))) float s_buf[5 * I2_SH * I2_MW];
    __shared__ float s_red[8];
    float* const s_d = s_buf;
    float* const s_dh = s_buf + 3 * I2_MH * I2_MW;
    static_assert(3 * I2_MH * I2_MW + 3 * I2_MH * I2_BW <= 5 * I2_SH * I2_MW, "derivative maps must fit the statistics' LDS");
    static_assert(I2_BW * (I2_BH / 2) == I2_T, "the last column pass is one item per thread");
    const int tid = threadIdx.x;
    const uint32_t n_work = work_list ? min(*work_count, nb) : nb;      // (dense: no list, every block)
    const int64_t plane = i2_plane(H, W);
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    for (uint32_t wi = blockIdx.x; wi < n_work; wi += gridDim.x) {
        const uint32_t bid = work_list ? work_list[wi] : wi;
        const int bxi = (int)(bid % (uint32_t)gxb), byi = (int)((bid / (uint32_t)gxb) % (uint32_t)gyb), v = (int)(bid / (uint32_t)(gxb * gyb));
        const int w0 = bxi * I2_BW, h0 = byi * I2_BH;
        const float* pm = mask ? mask + (int64_t)v * plane : nullptr;
        float l1_acc = 0.f, ss_acc = 0.f;
        for (int c = 0; c < 3; ++c) {
            const float* px = pred + ((int64_t)v * 3 + c) * plane;
            const float* py = target + ((int64_t)v * 3 + c) * plane;
            __syncthreads();      // LDS reuse across channels and blocks
            for (int t = tid; t < I2_SH * I2_SW; t += I2_T) {
                const int r = t / I2_SW, q = t - r * I2_SW;
                const int h = h0 - 2 * I2_R + r, w = w0 - 2 * I2_R + q;
                float x = 0.f, y = 0.f;
                if (h >= 0 && h < H && w >= 0 && w < W) {
                    const int64_t o = (int64_t)h * W + w;
                    x = px[o];
                    y = py[o];
                    if (pm) {
                        const float m = pm[o];
                        x *= m;
                        y *= m;
                    }
                }
                s_x[t] = x;
                s_y[t] = y;
            }
            __syncthreads();
            // row pass: statistics map column p (image w0 - 5 + p) takes the staged columns p .. p + 10
            for (int t = tid; t < I2_SH * (I2_MW / 2); t += I2_T) {
                const int r = t / (I2_MW / 2), p = (t - r * (I2_MW / 2)) * 2;
                float xs[12], ys[12], q12[12];
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const float2 a = *(const float2*)&s_x[r * I2_SW + p + 2 * k], b = *(const float2*)&s_y[r * I2_SW + p + 2 * k];
                    xs[2 * k] = a.x; xs[2 * k + 1] = a.y;
                    ys[2 * k] = b.x; ys[2 * k + 1] = b.y;
                }
                float a, b;
                float* o = s_buf + r * I2_MW + p;
                I2_FILTER2(a, b, xs);
                *(float2*)&o[0 * I2_SH * I2_MW] = make_float2(a, b);
                I2_FILTER2(a, b, ys);
                *(float2*)&o[1 * I2_SH * I2_MW] = make_float2(a, b);
#pragma unroll
                for (int k = 0; k < 12; ++k) q12[k] = xs[k] * xs[k];
                I2_FILTER2(a, b, q12);
                *(float2*)&o[2 * I2_SH * I2_MW] = make_float2(a, b);
#pragma unroll
                for (int k = 0; k < 12; ++k) q12[k] = ys[k] * ys[k];
                I2_FILTER2(a, b, q12);
                *(float2*)&o[3 * I2_SH * I2_MW] = make_float2(a, b);
#pragma unroll
                for (int k = 0; k < 12; ++k) q12[k] = xs[k] * ys[k];
                I2_FILTER2(a, b, q12);
                *(float2*)&o[4 * I2_SH * I2_MW] = make_float2(a, b);
            }
            __syncthreads();
            // column pass: map rows rp, rp + 1 (image h0 - 5 + rp) take the staged rows rp .. rp + 11; S and D1..D3 there
            constexpr int n_col_items = I2_MW * (I2_MH / 2);
            constexpr int n_rounds = (n_col_items + I2_T - 1) / I2_T;
            float dreg[n_rounds][2][3];
#pragma unroll
            for (int rd = 0; rd < n_rounds; ++rd) {
                const int t = tid + rd * I2_T;
#pragma unroll
                for (int pp = 0; pp < 2; ++pp) dreg[rd][pp][0] = dreg[rd][pp][1] = dreg[rd][pp][2] = 0.f;
                if (t < n_col_items) {
                    const int rq = t / I2_MW, q = t - rq * I2_MW, rp = 2 * rq;
                    float e[2][5];
#pragma unroll
                    for (int s5 = 0; s5 < 5; ++s5) {
                        float v12[12];
#pragma unroll
                        for (int k = 0; k < 12; ++k) v12[k] = s_buf[(s5 * I2_SH + rp + k) * I2_MW + q];
                        I2_FILTER2(e[0][s5], e[1][s5], v12);
                    }
                    const int w = w0 - I2_R + q;
#pragma unroll
                    for (int pp = 0; pp < 2; ++pp) {
                        const int h = h0 - I2_R + rp + pp;
                        if (h >= 0 && h < H && w >= 0 && w < W) {      // positions outside the image have no SSIM value
                            const float mu1 = e[pp][0], mu2 = e[pp][1];
                            const float s11 = e[pp][2] - mu1 * mu1, s22 = e[pp][3] - mu2 * mu2, s12 = e[pp][4] - mu1 * mu2;
                            const float A = 2.f * mu1 * mu2 + C1, B = 2.f * s12 + C2;
                            const float Cc = mu1 * mu1 + mu2 * mu2 + C1, Dd = s11 + s22 + C2;
                            const float iC = 1.f / Cc, iD = 1.f / Dd;
                            const float inv = iC * iD;
                            const float S = A * B * inv;
                            const bool own = rp + pp >= I2_R && rp + pp < I2_R + I2_BH && q >= I2_R && q < I2_R + I2_BW;
                            if (own) ss_acc += S;
                            dreg[rd][pp][0] = 2.f * mu2 * (B - A) * inv - S * 2.f * mu1 * iC + S * 2.f * mu1 * iD;
                            dreg[rd][pp][1] = -S * iD;
                            dreg[rd][pp][2] = 2.f * A * inv;
                        }
                    }
                }
            }
            // L1 over the block's own pixels (staged at + 10)
            for (int t = tid; t < I2_BH * I2_BW; t += I2_T) {
                const int r = t / I2_BW, q = t - r * I2_BW;
                if (h0 + r < H && w0 + q < W) {
                    const int o = (r + 2 * I2_R) * I2_SW + q + 2 * I2_R;
                    l1_acc += fabsf(s_x[o] - s_y[o]);
                }
            }
            if (!dL_dpred) continue;      // forward only (uniform)
            __syncthreads();              // everyone is done reading the statistics
#pragma unroll
            for (int rd = 0; rd < n_rounds; ++rd) {
                const int t = tid + rd * I2_T;
                if (t < n_col_items) {
                    const int rq = t / I2_MW, q = t - rq * I2_MW;
#pragma unroll
                    for (int pp = 0; pp < 2; ++pp)
#pragma unroll
                        for (int k = 0; k < 3; ++k) s_d[(k * I2_MH + 2 * rq + pp) * I2_MW + q] = dreg[rd][pp][k];
                }
            }
            __syncthreads();
            // row pass of the derivative maps: output column p (image w0 + p) takes the map columns p .. p + 10
            for (int t = tid; t < I2_MH * (I2_BW / 2); t += I2_T) {
                const int r = t / (I2_BW / 2), p = (t - r * (I2_BW / 2)) * 2;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    float v12[12];
#pragma unroll
                    for (int j = 0; j < 6; ++j) {
                        const float2 a = *(const float2*)&s_d[(k * I2_MH + r) * I2_MW + p + 2 * j];
                        v12[2 * j] = a.x; v12[2 * j + 1] = a.y;
                    }
                    float a, b;
                    I2_FILTER2(a, b, v12);
                    *(float2*)&s_dh[(k * I2_MH + r) * I2_BW + p] = make_float2(a, b);
                }
            }
            __syncthreads();
            // column pass: output rows rp, rp + 1 (image h0 + rp) take the map rows rp .. rp + 11
            {
                const int rq = tid / I2_BW, q = tid - rq * I2_BW, rp = 2 * rq;
                float f[2][3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    float v12[12];
#pragma unroll
                    for (int j = 0; j < 12; ++j) v12[j] = s_dh[(k * I2_MH + rp + j) * I2_BW + q];
                    I2_FILTER2(f[0][k], f[1][k], v12);
                }
                const int w = w0 + q;
#pragma unroll
                for (int pp = 0; pp < 2; ++pp) {
                    const int h = h0 + rp + pp;
                    if (h < H && w < W) {
                        const int o = (rp + pp + 2 * I2_R) * I2_SW + q + 2 * I2_R;
                        const float x = s_x[o], y = s_y[o];
                        const float dS = f[pp][0] + 2.f * x * f[pp][1] + y * f[pp][2];
                        const float df = x - y;
                        const float sgn = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);
                        float gr = grad_scale * (w_l1 * sgn - w_ssim * dS);
                        const int64_t go = (int64_t)h * W + w;
                        if (pm) gr = gr * pm[go];
                        dL_dpred[((int64_t)v * 3 + c) * plane + go] = gr;
                    }
                }
            }
        }
        // the block's two sums, in a fixed order
        const float l1_sum = mgr_wave_sum63(l1_acc), ss_sum = mgr_wave_sum63(ss_acc);
        __syncthreads();      // (s_red of the previous block has been read)
        if ((tid & 63) == 63) {
            s_red[tid >> 6] = l1_sum;
            s_red[4 + (tid >> 6)] = ss_sum;
        }
        __syncthreads();
        if (tid == 0) {
            const float pa = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]), pb = (s_red[4] + s_red[5]) + (s_red[6] + s_red[7]);
            I2Acc* sl = acc + (size_t)v * I2_SLOTS + ((uint32_t)(byi * gxb + bxi) & (I2_SLOTS - 1));
            if (!(fabsf(pa) <= sum_lim && fabsf(pb) <= sum_lim)) {      // (NaN fails the comparison)
                atomicAdd(&sl->bad, 1ull);
            } else {
                atomicAdd((unsigned long long*)&sl->l1, (unsigned long long)__double2ll_rn((double)pa * 4294967296.0));
                atomicAdd((unsigned long long*)&sl->ss, (unsigned long long)__double2ll_rn((double)pb * 4294967296.0));
            }
            atomicAdd(&sl->px, (unsigned long long)((min(w0 + I2_BW, W) - w0) * (min(h0 + I2_BH, H) - h0) * 3));
        }
    }
}

// Per view: its slots -> view_sums; the totals as a fixed tree of doubles over the views.  A flagged view reports NaN, and so
// do the totals; the other views' sums are what they would be without it.
__global__ __launch_bounds__(I2_T) void k_ssim2d_fold(int V, long long view_px3, const I2Acc* __restrict__ acc, float* __restrict__ sums,
                                                      float* __restrict__ view_sums, float ca, float cb, float cc) {
    __shared__ double s_a[I2_T], s_b[I2_T];
    const int tid = threadIdx.x;
    double ta = 0.0, tb = 0.0;
    for (int v = tid; v < V; v += I2_T) {
        long long l1 = 0, ss = 0;
        unsigned long long px = 0, bad = 0;
        for (int k = 0; k < I2_SLOTS; ++k) {
            const I2Acc a = acc[(size_t)v * I2_SLOTS + k];
            l1 += a.l1;
            ss += a.ss;
            px += a.px;
            bad += a.bad;
        }
        double a = (double)l1 * (1.0 / 4294967296.0);
        double b = (double)ss * (1.0 / 4294967296.0) + (double)((unsigned long long)view_px3 - px);   // settled: one per value
        if (bad) a = b = __longlong_as_double(0x7FF8000000000000ll);
        if (view_sums) {
            view_sums[2 * v] = (float)a;
            view_sums[2 * v + 1] = (float)b;
        }
        ta += a;
        tb += b;
    }
    s_a[tid] = ta;
    s_b[tid] = tb;
    __syncthreads();
    for (int n = I2_T / 2; n > 0; n >>= 1) {
        if (tid < n) {
            s_a[tid] += s_a[tid + n];
            s_b[tid] += s_b[tid + n];
        }
        __syncthreads();
    }
    if (tid == 0) {
        sums[0] = (float)s_a[0];
        sums[1] = (float)s_b[0];
        sums[2] = (float)((double)ca * s_a[0] + (double)cb * s_b[0] + (double)cc);   // the caller's loss value, no host-side arithmetic
    }
}

// workspace: 256 bytes of counters | sum slots | difference bitmap | work list
static int64_t i2_blocks(int V, int H, int W) { return (int64_t)V * ((H + I2_BH - 1) / I2_BH) * ((W + I2_BW - 1) / I2_BW); }
static int i2_row_words(int W) { return 2 * ((W + 63) / 64); }
static size_t i2_bitmap_offset(int V) { return 256 + (size_t)V * I2_SLOTS * sizeof(I2Acc); }
static size_t i2_list_offset(int V, int H, int W) {
    return (i2_bitmap_offset(V) + (size_t)V * (size_t)H * (size_t)i2_row_words(W) * sizeof(uint32_t) + 63) & ~(size_t)63;
}

extern "C" size_t mgr_image_loss2d_workspace_bytes(int V, int H, int W) {
    if (V <= 0 || H <= 0 || W <= 0) return 0;
    return i2_list_offset(V, H, W) + (size_t)i2_blocks(V, H, W) * sizeof(uint32_t);
}

extern "C" int mgr_image_loss2d_block(void) { return (I2_BW << 16) | I2_BH; }

extern "C" int mgr_image_loss2d(int V, int H, int W, const float* pred, const float* target, const float* mask, float w_l1,
                                float w_ssim, float grad_scale, float loss_offset, float* dL_dpred, float* sums, float* view_sums,
                                int flags, void* workspace, size_t workspace_bytes, void* stream_) {
    if (V <= 0 || H <= 0 || W <= 0) return mgr_fail(MGR_EINVAL, "mgr_image_loss2d: bad sizes");
    if (!pred || !target || !sums || !workspace) return mgr_fail(MGR_EINVAL, "mgr_image_loss2d: null pointer");
    if (H > 65535 || V > 65535) return mgr_fail(MGR_EINVAL, "mgr_image_loss2d: H and V must fit a grid dimension");
    if (3ll * H * W >= (1ll << 31)) return mgr_fail(MGR_EINVAL, "mgr_image_loss2d: a view's 3 H W values must stay below 2^31");
    const int64_t nb = i2_blocks(V, H, W);
    if (nb >= (1ll << 32)) return mgr_fail(MGR_EINVAL, "mgr_image_loss2d: image batch too large");
    if (flags & ~MGR_IL2D_DENSE) return mgr_fail(MGR_EINVAL, "mgr_image_loss2d: unknown flag");
    if (workspace_bytes < mgr_image_loss2d_workspace_bytes(V, H, W))
        return mgr_fail(MGR_ENOMEM, "mgr_image_loss2d: workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    // the window of image_loss_impl: gaussian(11, 1.5) in fp32, normalised (loss_utils.py:39-47)
    I2Window win;
    float sum = 0.f;
    for (int i = 0; i < 11; ++i) {
        win.g[i] = (float)exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
        sum += win.g[i];
    }
    for (int i = 0; i < 11; ++i) win.g[i] /= sum;
    const int gxb = (W + I2_BW - 1) / I2_BW, gyb = (H + I2_BH - 1) / I2_BH, row_words = i2_row_words(W);
    uint32_t* work_count = (uint32_t*)workspace;
    I2Acc* acc = (I2Acc*)((char*)workspace + 256);
    uint32_t* bitmap = (uint32_t*)((char*)workspace + i2_bitmap_offset(V));
    uint32_t* work_list = (uint32_t*)((char*)workspace + i2_list_offset(V, H, W));
    const bool dense = (flags & MGR_IL2D_DENSE) != 0;
    MGR_HIP(hipMemsetAsync(workspace, 0, i2_bitmap_offset(V), stream));      // list counter and sum slots
    if (!dense) {
        MGR_PROF("k_ssim2d_list", stream);
        hipLaunchKernelGGL(k_ssim2d_diff, dim3((W + I2_T - 1) / I2_T, H, V), dim3(I2_T), 0, stream, H, W, row_words, pred, target, mask,
                           bitmap);
        hipLaunchKernelGGL(k_ssim2d_list, dim3((unsigned)((nb + I2_LIST_BLOCKS - 1) / I2_LIST_BLOCKS)), dim3(I2_T), 0, stream, H, W,
                           row_words, gxb, gyb, (uint32_t)nb, (const uint32_t*)bitmap, dL_dpred, work_list, work_count);
    }
    {
        MGR_PROF("k_ssim2d", stream);
        const int64_t pb = nb < I2_GRID ? nb : I2_GRID;
        // (a hair below 2^31 / blocks of a view: the limit's rounding to fp32 cannot let that many sums at the limit reach 2^31)
        const float sum_lim = (float)(2147483648.0 * (1.0 - 1.0 / 1048576.0) / (double)(gxb * (int64_t)gyb));
        hipLaunchKernelGGL(k_ssim2d, dim3((unsigned)pb), dim3(I2_T), 0, stream, H, W, pred, target, mask, win, w_l1, w_ssim, grad_scale,
                           dL_dpred, dense ? (const uint32_t*)nullptr : (const uint32_t*)work_list, (const uint32_t*)work_count, gxb, gyb,
                           acc, (uint32_t)nb, sum_lim);
    }
    hipLaunchKernelGGL(k_ssim2d_fold, dim3(1), dim3(I2_T), 0, stream, V, 3ll * H * W, (const I2Acc*)acc, sums, view_sums,
                       grad_scale * w_l1, -grad_scale * w_ssim, loss_offset);
    MGR_LAUNCH_CHECK("k_ssim2d", stream, 0);
    return MGR_OK;
}
