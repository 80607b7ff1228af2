// Device frame store: the stored uint8 RGBA crops of a capture, decoded on the device into the float targets and masks of a
// step (mgr_frames_decode).  Restates SequenceDataset.fetch_images (dataset.py; brics_dynamic.py:343-373) with _area_resize for
// the factor 1/k, bit for bit:
//
//   source pixel   the crop's value inside its bbox, (0,0,0,0) outside -- the full frame is never built
//   block mean     per channel the integer sum s of the k x k block, m = (2 s + k^2) / (2 k^2) in integers = floor(s / k^2 + 0.5)
//   composite      c' = LUT[m_c], a' = LUT[m_a], LUT[i] = i / 255.0 in fp64;  target = fp32(c' a' + bg (1 - a')), every product and
//                  sum rounded on its own (no fma: numpy has none), one rounding to fp32;  mask = fp32(a')
//
// The LUT is a table of compile-time constants (the host compiler's i / 255.0, IEEE round-to-nearest like numpy's): no division
// on the device.  The view records travel as kernel arguments (at most MGR_FRAMES_MAX_VIEWS per launch): no copy, no allocation,
// no synchronisation in the call.
//
// k_frames_decode: one workgroup of 256 threads per (tile of FR_TILE_W x FR_TILE_H output pixels, view), the tiles laid over the
// view's own rectangle (its left edge rounded down to a multiple of 4, so that a lane's four pixels are one aligned float4);
// lane l of wave w takes the pixels x .. x + 3 of row w of the tile: a wave stores 1 KB of one row per plane.  The kernel is
// bound by its stores (16 B per output pixel); the fp64 arithmetic is a dozen operations per pixel.  Workgroups beyond the
// view's rectangle return at once (the grid is sized for the largest rectangle of the launch).
#include "mgr_common.h"

#include <algorithm>
#include <vector>

#define FR_T 256
#define FR_TILE_W 256      // 64 lanes x 4 pixels
#define FR_TILE_H 4        // one row per wave

struct FrLut {
    double v[256];
};
static constexpr FrLut fr_make_lut() {
    FrLut l{};
    for (int i = 0; i < 256; ++i) l.v[i] = (double)i / 255.0;
    return l;
}
__constant__ FrLut c_fr_lut = fr_make_lut();

struct FrArgs {
    MgrFrameView v[MGR_FRAMES_MAX_VIEWS];
};

// one rounding per operation, like the numpy expression img * alpha + bkgd * (1.0 - alpha) in float64
__device__ __forceinline__ float fr_composite(double c, double a, double bg) {
#pragma clang fp contract(off)
    const double fg = c * a;
    const double rest = 1.0 - a;
    const double back = bg * rest;
    return (float)(fg + back);
}

__global__ __launch_bounds__(FR_T) void k_frames_decode(const FrArgs args, int H, int W, int k, const uint8_t* __restrict__ pool,
                                                        float* __restrict__ targets, float* __restrict__ masks, int vec) {
    __shared__ double s_lut[256];
    const MgrFrameView& v = args.v[blockIdx.z];
    const int tid = threadIdx.x;
    const int xb = (v.rx0 & ~3) + (int)blockIdx.x * FR_TILE_W, yb = v.ry0 + (int)blockIdx.y * FR_TILE_H;
    if (xb >= v.rx1 || yb >= v.ry1) return;      // (the whole workgroup: in front of the barrier)
    s_lut[tid] = c_fr_lut.v[tid];
    __syncthreads();
    const int x = xb + (tid & 63) * 4, y = yb + (tid >> 6);
    if (y >= v.ry1 || x >= v.rx1 || x + 4 <= v.rx0) return;
    const int x0 = v.x0, y0 = v.y0, x1 = v.x1, y1 = v.y1;
    const long long cw = (long long)(x1 - x0);
    const uint8_t* crop = pool + v.offset;
    const uint32_t kk = (uint32_t)k * (uint32_t)k;
    const double bg[3] = {(double)v.bg[0], (double)v.bg[1], (double)v.bg[2]};
    float o[4][4];       // [pixel][r, g, b, mask]
    bool in[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int px = x + p;
        in[p] = px >= v.rx0 && px < v.rx1;
        uint32_t s[4] = {0u, 0u, 0u, 0u};
        if (in[p]) {
            for (int dy = 0; dy < k; ++dy) {
                const int sy = y * k + dy;
                if (sy < y0 || sy >= y1) continue;
                const uint8_t* row = crop + (long long)(sy - y0) * cw * 4;
                for (int dx = 0; dx < k; ++dx) {
                    const int sx = px * k + dx;
                    if (sx < x0 || sx >= x1) continue;
                    const uint32_t q = *(const uint32_t*)(row + (long long)(sx - x0) * 4);      // R | G << 8 | B << 16 | A << 24
                    s[0] += q & 255u;
                    s[1] += (q >> 8) & 255u;
                    s[2] += (q >> 16) & 255u;
                    s[3] += q >> 24;
                }
            }
            if (k > 1) {
#pragma unroll
                for (int c = 0; c < 4; ++c) s[c] = (2u * s[c] + kk) / (2u * kk);
            }
        }
        const double a = s_lut[s[3]];
#pragma unroll
        for (int c = 0; c < 3; ++c) o[p][c] = fr_composite(s_lut[s[c]], a, bg[c]);
        o[p][3] = (float)a;
    }
    const size_t plane = (size_t)H * (size_t)W, at = (size_t)y * (size_t)W + (size_t)x;
    float* t = targets + (size_t)v.slot * 3 * plane + at;
    float* m = masks ? masks + (size_t)v.slot * plane + at : nullptr;
    if (vec && in[0] && in[3]) {      // (x is a multiple of 4, W too, the tables are 16-byte aligned)
#pragma unroll
        for (int c = 0; c < 3; ++c) *(float4*)(t + (size_t)c * plane) = make_float4(o[0][c], o[1][c], o[2][c], o[3][c]);
        if (m) *(float4*)m = make_float4(o[0][3], o[1][3], o[2][3], o[3][3]);
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (!in[p]) continue;
#pragma unroll
            for (int c = 0; c < 3; ++c) t[(size_t)c * plane + p] = o[p][c];
            if (m) m[p] = o[p][3];
        }
    }
}

extern "C" int mgr_frames_decode(int V, int H, int W, int k, const uint8_t* pool, int64_t pool_bytes, const MgrFrameView* views_host,
                                 float* targets, float* masks, int64_t n_slots, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (V < 0 || H <= 0 || W <= 0 || n_slots < 0 || pool_bytes < 0) return mgr_fail(MGR_EINVAL, "mgr_frames_decode: bad sizes");
    if (k < 1) return mgr_fail(MGR_EINVAL, "mgr_frames_decode: k < 1");
    // the source frame is (H k) x (W k): its coordinates and the block sums (at most 511 k^2) stay within 32 bits
    if (H > FR_TILE_H * 65535) return mgr_fail(MGR_EINVAL, "mgr_frames_decode: image too tall for one grid");
    if (k > 1024 || (long long)W * k > 0x7FFFFFFFll || (long long)H * k > 0x7FFFFFFFll)
        return mgr_fail(MGR_EINVAL, "mgr_frames_decode: source frame too large (k <= 1024, W k and H k below 2^31)");
    if (V == 0) return MGR_OK;
    if (!views_host || !targets) return mgr_fail(MGR_EINVAL, "mgr_frames_decode: null pointer");
    const long long SW = (long long)W * k, SH = (long long)H * k;
    std::vector<int32_t> slots((size_t)V);
    for (int i = 0; i < V; ++i) {
        const MgrFrameView& v = views_host[i];
        if (v.x0 < 0 || v.y0 < 0 || v.x1 < v.x0 || v.y1 < v.y0 || v.x1 > SW || v.y1 > SH)
            return mgr_fail(MGR_EINVAL, "mgr_frames_decode: bbox outside the source frame or reversed");
        if (v.offset < 0 || (v.offset & 15) != 0) return mgr_fail(MGR_EINVAL, "mgr_frames_decode: offset is not a multiple of 16");
        const long long bytes = (long long)(v.x1 - v.x0) * (long long)(v.y1 - v.y0) * 4;
        if (bytes > 0 && !pool) return mgr_fail(MGR_EINVAL, "mgr_frames_decode: null pool with a non-empty crop");
        if (v.offset > pool_bytes || bytes > pool_bytes - v.offset)
            return mgr_fail(MGR_EINVAL, "mgr_frames_decode: crop ends beyond the pool");
        if (v.rx0 < 0 || v.ry0 < 0 || v.rx1 < v.rx0 || v.ry1 < v.ry0 || v.rx1 > W || v.ry1 > H)
            return mgr_fail(MGR_EINVAL, "mgr_frames_decode: rectangle outside the image");
        if (v.slot < 0 || (int64_t)v.slot >= n_slots) return mgr_fail(MGR_EINVAL, "mgr_frames_decode: slot outside the table");
        slots[(size_t)i] = v.slot;
    }
    std::sort(slots.begin(), slots.end());
    if (std::adjacent_find(slots.begin(), slots.end()) != slots.end())
        return mgr_fail(MGR_EINVAL, "mgr_frames_decode: two views name the same slot");
    const int vec = (W % 4 == 0 && ((uintptr_t)targets & 15) == 0 && ((uintptr_t)masks & 15) == 0) ? 1 : 0;
    MGR_PROF("k_frames_decode", stream);
    for (int base = 0; base < V; base += MGR_FRAMES_MAX_VIEWS) {
        const int n = std::min(V - base, (int)MGR_FRAMES_MAX_VIEWS);
        FrArgs args;
        memset(&args, 0, sizeof(args));
        int gw = 0, gh = 0;
        for (int i = 0; i < n; ++i) {
            const MgrFrameView& v = args.v[i] = views_host[base + i];
            if (v.rx1 == v.rx0 || v.ry1 == v.ry0) continue;
            gw = std::max(gw, (v.rx1 - (v.rx0 & ~3) + FR_TILE_W - 1) / FR_TILE_W);
            gh = std::max(gh, (v.ry1 - v.ry0 + FR_TILE_H - 1) / FR_TILE_H);
        }
        if (gw == 0 || gh == 0) continue;      // nothing to write in this chunk
        hipLaunchKernelGGL(k_frames_decode, dim3((unsigned)gw, (unsigned)gh, (unsigned)n), dim3(FR_T), 0, stream, args, H, W, k, pool,
                           targets, masks, vec);
        MGR_LAUNCH_CHECK("k_frames_decode", stream, 0);
    }
    return MGR_OK;
}
