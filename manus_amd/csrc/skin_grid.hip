// Skin-weight grid gradient for gfx950: the other half of k_skin_bwd's chain rule.  dL/dw (N,B) -> a SPARSE dL/d(grid): the
// sorted list of the voxels that at least one processed Gaussian touches and one gradient row per listed voxel; plus the row
// Adam that steps the grid on such a list.
//
// No reference kernel counterpart: in the reference the gradient falls out of autograd through F.grid_sample
// (src/utils/gaussian_utils.py:173) once grid_weights requires grad.
//
// With k_skin_bwd's notation, for a processed Gaussian n: corner weights t_c, raw samples s_b = sum_c t_c g[c][b], S = sum_b s_b,
// w_b = s_b / S, a = dL_dw[n], r_b = (a_b - sum_k a_k w_k) / S, and G[voxel(c)][b] += t_c r_b for every corner inside the grid.
// r needs S and sum_k a_k s_k only, so a Gaussian costs the same 8 row gathers as k_skin_bwd.
//
// The scatter is a gather, by the counting pattern of knn.hip / contact.hip:
//   k_sg_prep / k_sg_prep24   per list entry: S, r (kept, 32 floats per entry), the mask of its in-bounds corners; integer
//                             atomics count the contributors of every voxel into a D*H*W array
//   k_sg_scan_a/b/c           exclusive scan of the counts that also compacts the non-empty voxels: the ascending voxel list,
//                             the segment offsets, and per voxel the END of its segment left in the count array
//   k_sg_scatter              per list entry and corner: a slot of the voxel's segment (atomic decrement of that end)
//   k_sg_rank                 per slot: its rank in its segment by Gaussian index -- the slot order comes from atomics, the
//                             rank does not -- and the (entry, weight) pair moved to that rank
//   k_sg_reduce               one wave per listed voxel, a lane per channel: the ranked segment added in order
// No float atomics anywhere: the sums are fixed by the Gaussian indices alone, so any permutation of the same list gives the
// same bits.
//
// The refinement step on such a list (mgr_skin_grid_refine):
//   k_sg_refine<PRIOR>        32 lanes per listed row, 8 rows per workgroup: prior gradient towards a kept grid, the row Adam,
//                             clamp, the row divided by its sum, the row's share of the prior's value -- one pass
//   k_sg_refine_fold          the workgroups' fp64 partials of the prior's value added in a fixed tree
// The reference (HandGaussianModel.optimizing_skin_weights, src/models/hand_gaussian.py) would run a dense torch Adam over the
// whole grid_weights tensor and keeps grid_weights_init beside it; it has no kernel for any of this.
#include "skin_tri.h"

#define SG_RS 32        // floats per kept r row (MGR_MAX_BONES)
#define SG_CHUNK 2048   // voxels per workgroup of the scan: 256 threads x 8

struct SgLayout {
    size_t cnt, bsum, seg_off, mask, r, rec_n, rec_t, rec_w, srt_t, srt_w, total;
    size_t nvox, rows, pairs, nblk;
};

static inline SgLayout sg_layout(int D, int H, int W, int max_count) {
    SgLayout L;
    const size_t mc = (size_t)(max_count > 0 ? max_count : 0);
    L.nvox = (size_t)(D > 0 ? D : 0) * (size_t)(H > 0 ? H : 0) * (size_t)(W > 0 ? W : 0);
    L.pairs = 8 * mc;
    L.rows = L.pairs < L.nvox ? L.pairs : L.nvox;
    L.nblk = (L.nvox + SG_CHUNK - 1) / SG_CHUNK;
    size_t o = 0;
    L.cnt = o;      o += mgr_align(L.nvox * 4);          // contributors per voxel -> end of the voxel's segment
    L.bsum = o;     o += mgr_align((L.nblk + 1) * 8);    // per scan workgroup (pairs, non-empty voxels)
    L.seg_off = o;  o += mgr_align((L.rows + 1) * 4);    // first slot of every listed voxel, then the total
    L.mask = o;     o += mgr_align((mc + 1) * 4);        // per list entry the bits of its in-bounds corners, 0 = contributes nothing
    L.r = o;        o += mgr_align((mc + 1) * SG_RS * 4);
    L.rec_n = o;    o += mgr_align((L.pairs + 1) * 4);   // slots in scatter order: Gaussian, list entry, corner weight
    L.rec_t = o;    o += mgr_align((L.pairs + 1) * 4);
    L.rec_w = o;    o += mgr_align((L.pairs + 1) * 4);
    L.srt_t = o;    o += mgr_align((L.pairs + 1) * 4);   // the same slots ranked by Gaussian inside each segment
    L.srt_w = o;    o += mgr_align((L.pairs + 1) * 4);
    L.total = o;
    return L;
}

__device__ __forceinline__ bool sg_corner(const TriSetup& s, int k, int D, int H, int W, int& x, int& y, int& z) {
    x = s.x0 + (k & 1), y = s.y0 + ((k >> 1) & 1), z = s.z0 + (k >> 2);
    return x >= 0 && x < W && y >= 0 && y < H && z >= 0 && z < D;
}

// the entry's Gaussian, or -1 when the entry is past the list or names no articulated Gaussian
__device__ __forceinline__ int sg_entry(int t, int N, const uint32_t* __restrict__ index, const uint32_t* __restrict__ index_count) {
    if (!index) return t < N ? t : -1;
    if ((uint32_t)t >= *index_count) return -1;
    const uint32_t i = index[t];
    return i < (uint32_t)N ? (int)i : -1;
}

// S is settled, r written, the in-bounds corners counted
__device__ __forceinline__ void sg_prep_finish(int t, int i, int B, const TriSetup& s, int D, int H, int W, float S, float dS,
                                               const float* __restrict__ a_row, uint32_t* __restrict__ cnt,
                                               uint32_t* __restrict__ mask, float* __restrict__ rbuf) {
    if (S == 0.f || !isfinite(S)) {   // every corner outside, or every in-bounds corner zero: contributes nothing, lists nothing
        mask[t] = 0u;
        return;
    }
    const float invS = 1.0f / S, dot = dS * invS;
    float* r = rbuf + (size_t)t * SG_RS;
    for (int b = 0; b < B; ++b) r[b] = (a_row[b] - dot) * invS;
    uint32_t m = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int x, y, z;
        if (sg_corner(s, k, D, H, W, x, y, z)) {
            m |= 1u << k;
            atomicAdd(&cnt[((size_t)z * H + y) * W + x], 1u);
        }
    }
    mask[t] = m;
}

// generic layout: grid_stride == B, any alignment
__global__ __launch_bounds__(256) void k_sg_prep(int N, const float* __restrict__ xyz, const float* __restrict__ grid, int D, int H,
                                                 int W, int B, const float* __restrict__ center, const float* __restrict__ scale,
                                                 const float* __restrict__ dL_dw, const uint32_t* __restrict__ index,
                                                 const uint32_t* __restrict__ index_count, int max_count,
                                                 uint32_t* __restrict__ cnt, uint32_t* __restrict__ mask, float* __restrict__ rbuf) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= max_count) return;
    const int i = sg_entry(t, N, index, index_count);
    if (i < 0) { mask[t] = 0u; return; }
    const TriSetup s = tri_setup(xyz, i, center, scale, D, H, W);
    float Wk[8];
    tri_weights(s, Wk);
    const float* a = dL_dw + (size_t)i * B;
    float S = 0.f, dS = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int x, y, z;
        if (!sg_corner(s, k, D, H, W, x, y, z)) continue;   // zero padding
        const float* g = grid + (((size_t)z * H + y) * W + x) * B;
        float Pk = 0.f, Qk = 0.f;
        for (int b = 0; b < B; ++b) {
            const float c = g[b];
            Pk += a[b] * c;
            Qk += c;
        }
        S += Wk[k] * Qk;
        dS += Wk[k] * Pk;
    }
    sg_prep_finish(t, i, B, s, D, H, W, S, dS, a, cnt, mask, rbuf);
}

// padded layout: 24 floats per voxel on a 16-byte aligned base, every corner six float4 (the gathers of k_skin_bwd24)
__global__ __launch_bounds__(256) void k_sg_prep24(int N, const float* __restrict__ xyz, const float4* __restrict__ grid, int D,
                                                   int H, int W, int B, const float* __restrict__ center,
                                                   const float* __restrict__ scale, const float* __restrict__ dL_dw,
                                                   const uint32_t* __restrict__ index, const uint32_t* __restrict__ index_count,
                                                   int max_count, uint32_t* __restrict__ cnt, uint32_t* __restrict__ mask,
                                                   float* __restrict__ rbuf) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= max_count) return;
    const int i = sg_entry(t, N, index, index_count);
    if (i < 0) { mask[t] = 0u; return; }
    const TriSetup s = tri_setup(xyz, i, center, scale, D, H, W);
    float Wk[8];
    tri_weights(s, Wk);
    const float* row = dL_dw + (size_t)i * B;
    float a[SKIN_BP];
#pragma unroll
    for (int b = 0; b < SKIN_BP; ++b) a[b] = b < B ? row[b] : 0.f;
    float S = 0.f, dS = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {   // unconditional loads on clamped coordinates, an outside corner's sums set to zero
        int x, y, z;
        const float inb = sg_corner(s, k, D, H, W, x, y, z) ? 1.f : 0.f;
        const int xc = min(max(x, 0), W - 1), yc = min(max(y, 0), H - 1), zc = min(max(z, 0), D - 1);
        const float4* p = grid + (((size_t)zc * H + yc) * W + xc) * (SKIN_BP / 4);
        float Pk = 0.f, Qk = 0.f;
#pragma unroll
        for (int q = 0; q < SKIN_BP / 4; ++q) {
            const float4 c = p[q];
            Pk += a[4 * q] * c.x + a[4 * q + 1] * c.y + a[4 * q + 2] * c.z + a[4 * q + 3] * c.w;
            Qk += (c.x + c.y) + (c.z + c.w);     // pad channels are zero
        }
        S += Wk[k] * (Qk * inb);
        dS += Wk[k] * (Pk * inb);
    }
    sg_prep_finish(t, i, B, s, D, H, W, S, dS, row, cnt, mask, rbuf);
}

// ---------------------------------------------------------------------------
// scan of the counts: (slots, non-empty voxels) per workgroup, over the workgroups, then per voxel
// ---------------------------------------------------------------------------
__device__ __forceinline__ void sg_thread_counts(const uint32_t* __restrict__ cnt, size_t base, size_t nvox, uint32_t c[8],
                                                 uint32_t& p, uint32_t& q) {
    p = q = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        c[e] = base + e < nvox ? cnt[base + e] : 0u;
        p += c[e];
        q += c[e] != 0u;
    }
}

__device__ __forceinline__ uint32_t sg_wave_incl(uint32_t v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if ((int)(threadIdx.x & 63) >= d) v += o;
    }
    return v;
}

__global__ __launch_bounds__(256) void k_sg_scan_a(size_t nvox, const uint32_t* __restrict__ cnt, uint2* __restrict__ bsum) {
    __shared__ uint2 s_w[4];
    uint32_t c[8], p, q;
    sg_thread_counts(cnt, (size_t)blockIdx.x * SG_CHUNK + threadIdx.x * 8, nvox, c, p, q);
    p = sg_wave_incl(p);
    q = sg_wave_incl(q);
    if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = make_uint2(p, q);
    __syncthreads();
    if (threadIdx.x == 0)
        bsum[blockIdx.x] = make_uint2((s_w[0].x + s_w[1].x) + (s_w[2].x + s_w[3].x), (s_w[0].y + s_w[1].y) + (s_w[2].y + s_w[3].y));
}

// one workgroup: exclusive scan of the per-workgroup sums in place; the totals close the segment offsets and the row count
__global__ __launch_bounds__(1024) void k_sg_scan_b(int nblk, uint2* __restrict__ bsum, uint32_t* __restrict__ seg_off,
                                                    uint32_t* __restrict__ out_count, uint32_t rows_cap) {
    __shared__ uint2 s_part[1024];
    const int tid = threadIdx.x, per = (nblk + 1023) / 1024;
    const int b = min(nblk, tid * per), e = min(nblk, b + per);
    uint2 s = make_uint2(0u, 0u);
    for (int k = b; k < e; ++k) { s.x += bsum[k].x; s.y += bsum[k].y; }
    s_part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        uint2 run = make_uint2(0u, 0u);
        for (int k = 0; k < 1024; ++k) {
            const uint2 v = s_part[k];
            s_part[k] = run;
            run.x += v.x; run.y += v.y;
        }
        const uint32_t rows = min(run.y, rows_cap);   // (run.y <= rows_cap by the capacity rule; the min keeps a broken caller in bounds)
        seg_off[rows] = run.x;
        *out_count = rows;
    }
    __syncthreads();
    uint2 run = s_part[tid];
    for (int k = b; k < e; ++k) {
        const uint2 v = bsum[k];
        bsum[k] = run;
        run.x += v.x; run.y += v.y;
    }
}

__global__ __launch_bounds__(256) void k_sg_scan_c(size_t nvox, uint32_t* __restrict__ cnt, const uint2* __restrict__ bsum,
                                                   uint32_t* __restrict__ seg_off, int32_t* __restrict__ out_voxel,
                                                   uint32_t rows_cap) {
    __shared__ uint2 s_w[4];
    const size_t base = (size_t)blockIdx.x * SG_CHUNK + threadIdx.x * 8;
    uint32_t c[8], p, q;
    sg_thread_counts(cnt, base, nvox, c, p, q);
    const uint32_t pi = sg_wave_incl(p), qi = sg_wave_incl(q);
    if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = make_uint2(pi, qi);
    __syncthreads();
    uint2 run = bsum[blockIdx.x];
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) { run.x += s_w[w].x; run.y += s_w[w].y; }
    run.x += pi - p;
    run.y += qi - q;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        if (c[e] == 0u) continue;
        if (run.y < rows_cap) {
            out_voxel[run.y] = (int32_t)(base + e);
            seg_off[run.y] = run.x;
        }
        run.x += c[e];
        cnt[base + e] = run.x;     // the END of the segment: k_sg_scatter counts it down to the start
        run.y += 1u;
    }
}

__global__ __launch_bounds__(256) void k_sg_scatter(int N, const float* __restrict__ xyz, int D, int H, int W,
                                                    const float* __restrict__ center, const float* __restrict__ scale,
                                                    const uint32_t* __restrict__ index, int max_count,
                                                    const uint32_t* __restrict__ mask, uint32_t* __restrict__ cnt,
                                                    uint32_t* __restrict__ rec_n, uint32_t* __restrict__ rec_t,
                                                    float* __restrict__ rec_w, uint32_t pairs_cap) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= max_count) return;
    const uint32_t m = mask[t];
    if (!m) return;
    const int i = index ? (int)index[t] : t;     // (a non-zero mask: k_sg_prep found the entry inside the list and below N)
    const TriSetup s = tri_setup(xyz, i, center, scale, D, H, W);
    float Wk[8];
    tri_weights(s, Wk);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int x, y, z;
        if (!((m >> k) & 1u) || !sg_corner(s, k, D, H, W, x, y, z)) continue;
        const uint32_t slot = atomicSub(&cnt[((size_t)z * H + y) * W + x], 1u) - 1u;
        if (slot < pairs_cap) {
            rec_n[slot] = (uint32_t)i;
            rec_t[slot] = (uint32_t)t;
            rec_w[slot] = Wk[k];
        }
    }
}

// One thread per slot: its segment by bisection of the offsets, its rank by counting the smaller Gaussian indices of the segment.
// A Gaussian is in a voxel's segment once per time the list names it, and then with the same weight and the same r: ties move
// equal values, in whatever order.  A segment of L slots costs L threads L reads each, spread over the device.
__global__ __launch_bounds__(256) void k_sg_rank(const uint32_t* __restrict__ out_count, const uint32_t* __restrict__ seg_off,
                                                 const uint32_t* __restrict__ rec_n, const uint32_t* __restrict__ rec_t,
                                                 const float* __restrict__ rec_w, uint32_t* __restrict__ srt_t,
                                                 float* __restrict__ srt_w) {
    const uint32_t rows = *out_count, total = seg_off[rows];
    for (uint32_t p = blockIdx.x * 256 + threadIdx.x; p < total; p += gridDim.x * 256) {
        uint32_t lo = 0u, hi = rows;     // the last row whose offset is <= p
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (seg_off[mid] <= p) lo = mid; else hi = mid;
        }
        const uint32_t b = seg_off[lo], e = seg_off[lo + 1];
        const uint32_t key = rec_n[p];
        uint32_t rank = 0u;
        for (uint32_t j = b; j < e; ++j) {
            const uint32_t nj = rec_n[j];
            rank += (nj < key || (nj == key && j < p)) ? 1u : 0u;
        }
        srt_t[b + rank] = rec_t[p];
        srt_w[b + rank] = rec_w[p];
    }
}

// One wave per listed voxel; lane = (half, channel): a half adds every second slot of the ranked segment in ascending order, the
// two partial sums meet in one add.  The shape depends on the segment's length alone.
__global__ __launch_bounds__(256) void k_sg_reduce(const uint32_t* __restrict__ out_count, const uint32_t* __restrict__ seg_off,
                                                   const uint32_t* __restrict__ srt_t, const float* __restrict__ srt_w,
                                                   const float* __restrict__ rbuf, float* __restrict__ out_grad, int B,
                                                   int grid_stride) {
    const uint32_t rows = *out_count;
    const int lane = threadIdx.x & 63, h = lane >> 5, b = lane & 31;
    const int bb = b < B ? b : 0;     // (lanes past B read channel 0 and write zero: no divergence inside the wave)
    for (uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6); i < rows; i += gridDim.x * 4) {
        const uint32_t beg = seg_off[i], end = seg_off[i + 1];
        float acc = 0.f;
        uint32_t p = beg + h;
        for (; p + 6 < end; p += 8) {   // four slots of this half in flight
            const uint32_t t0 = srt_t[p], t1 = srt_t[p + 2], t2 = srt_t[p + 4], t3 = srt_t[p + 6];
            const float w0 = srt_w[p], w1 = srt_w[p + 2], w2 = srt_w[p + 4], w3 = srt_w[p + 6];
            const float r0 = rbuf[(size_t)t0 * SG_RS + bb], r1 = rbuf[(size_t)t1 * SG_RS + bb];
            const float r2 = rbuf[(size_t)t2 * SG_RS + bb], r3 = rbuf[(size_t)t3 * SG_RS + bb];
            acc += w0 * r0;
            acc += w1 * r1;
            acc += w2 * r2;
            acc += w3 * r3;
        }
        for (; p < end; p += 2) acc += srt_w[p] * rbuf[(size_t)srt_t[p] * SG_RS + bb];
        acc += __shfl_xor(acc, 32, 64);
        if (h == 0 && b < grid_stride) out_grad[(size_t)i * grid_stride + b] = b < B ? acc : 0.f;
    }
}

// ---------------------------------------------------------------------------
// row Adam (torch.optim.SparseAdam): one thread per (listed row, channel)
// ---------------------------------------------------------------------------
// One element's Adam step, shared by k_sg_adam and k_sg_refine: the moments are stored, the stepped (unclamped) value returned.
__device__ __forceinline__ float sg_adam_update(float x, float g, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq, size_t o,
                                                float step_size, float omb1, float omb2, float eps) {
    const float m0 = exp_avg[o], v0 = exp_avg_sq[o];
    const float m = m0 + (g - m0) * omb1;      // omb = 1 - beta, rounded once from double (1.0f - 0.999f is off by 5e-5 of itself: the hyper-parameters are doubles, as in mgr_adam_step)
    const float v = v0 + (g * g - v0) * omb2;
    exp_avg[o] = m;
    exp_avg_sq[o] = v;
    return x - step_size * (m / (sqrtf(v) + eps));
}

// the step size with the bias corrections of the global step, in double as torch takes them
static inline float sg_adam_step_size(double lr, double beta1, double beta2, int step) {
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    return (float)(lr * sqrt(bc2) / bc1);
}

__global__ __launch_bounds__(256) void k_sg_adam(const int32_t* __restrict__ voxel, const float* __restrict__ grad,
                                                 const uint32_t* __restrict__ count, int capacity, float* __restrict__ grid,
                                                 int grid_stride, int B, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                 float step_size, float omb1, float omb2, float eps, int clamp, float clamp_min) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t row = gid / (size_t)B;
    const int b = (int)(gid - row * (size_t)B);
    const uint32_t rows = min(*count, (uint32_t)capacity);
    if (row >= rows) return;
    const size_t o = (size_t)voxel[row] * grid_stride + b;
    const float g = grad[row * grid_stride + b];
    float x = sg_adam_update(grid[o], g, exp_avg, exp_avg_sq, o, step_size, omb1, omb2, eps);
    if (clamp) x = fmaxf(x, clamp_min);
    grid[o] = x;
}

// ---------------------------------------------------------------------------
// refinement step: prior gradient + row Adam + clamp + projection of the row onto sum 1 + the prior's value, one pass
// ---------------------------------------------------------------------------
// 32 lanes per listed row (lane = channel), 8 rows per workgroup: a row of the padded layout is one 96-byte access per array.
// The row sum and the row's fp64 prior partial meet by __shfl_xor 16 .. 1, which stays inside the half-wave; every lane of the
// half-wave ends with the same bits (a + b == b + a).  A workgroup walks the blocks of eight rows blk = blockIdx.x, blockIdx.x +
// gridDim.x, ... below the count (the capacity is min(8 * entries, D*H*W) rows, the count a fraction of it: one workgroup per
// block of the capacity would launch mostly workgroups that leave at once); a block's eight row partials are added in a fixed
// order and stored plainly at partial[blk], and k_sg_refine_fold adds the partials of the blocks below the count in a tree fixed
// by the count alone -- neither depends on the grid size.  No atomics.  PRIOR false: the instantiation has no prior arithmetic
// at all, the Adam sees the loaded gradient as in k_sg_adam.
#define SGR_ROWS 8          // rows per workgroup and pass of k_sg_refine
#define SGR_MAX_BLOCKS 4096 // workgroups of k_sg_refine at most (k_sg_rank, k_sg_reduce)

template <bool PRIOR>
__global__ __launch_bounds__(256) void k_sg_refine(const int32_t* __restrict__ voxel, const float* __restrict__ grad,
                                                   const uint32_t* __restrict__ count, int capacity, float* __restrict__ grid,
                                                   const float* __restrict__ grid0, int grid_stride, int B,
                                                   float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq, float step_size,
                                                   float omb1, float omb2, float eps, int clamp, float clamp_min, float w2,
                                                   int project, float min_sum, double* __restrict__ partial) {
    __shared__ double s_part[SGR_ROWS];
    const int sub = threadIdx.x >> 5, b = threadIdx.x & 31;
    const uint32_t rows = min(*count, (uint32_t)capacity);
    for (size_t blk = blockIdx.x; blk * SGR_ROWS < rows; blk += gridDim.x) {     // (uniform over the workgroup: the barriers below are met by all of it)
        const size_t row = blk * SGR_ROWS + sub;
        const bool live = row < rows && b < B;       // (lanes of the pad channels and of rows behind the count read and write nothing)
        size_t o = 0;
        float x = 0.f;
        double dd = 0.0;
        if (live) {
            o = (size_t)voxel[row] * grid_stride + b;
            float g = grad[row * grid_stride + b];
            const float x0 = grid[o];
            if (PRIOR) {
                const float d = x0 - grid0[o];
                g = g + w2 * d;
                dd = (double)d * (double)d;
            }
            x = sg_adam_update(x0, g, exp_avg, exp_avg_sq, o, step_size, omb1, omb2, eps);
            if (clamp) x = fmaxf(x, clamp_min);
        }
        if (project) {
            float S = x;
#pragma unroll
            for (int d = 16; d >= 1; d >>= 1) S += __shfl_xor(S, d, 64);
            if (S > min_sum) x = x / S;      // false for a NaN sum: the row stays as clamped, and no division ever creates a NaN
        }
        if (live) grid[o] = x;
        if (PRIOR) {
#pragma unroll
            for (int d = 16; d >= 1; d >>= 1) dd += __shfl_xor(dd, d, 64);
            if (b == 0) s_part[sub] = dd;
            __syncthreads();
            if (threadIdx.x == 0)
                partial[blk] = ((s_part[0] + s_part[1]) + (s_part[2] + s_part[3])) + ((s_part[4] + s_part[5]) + (s_part[6] + s_part[7]));
            __syncthreads();                 // (s_part is written again by the next pass)
        }
    }
}

// one workgroup over the partials of the row blocks below the count: thread t adds partial[t], partial[t + 256], ... in ascending
// order (eight loads in flight, the adds in that order), the 256 sums meet in a fixed tree
__global__ __launch_bounds__(256) void k_sg_refine_fold(const double* __restrict__ partial, const uint32_t* __restrict__ count,
                                                        int capacity, double prior_weight, double* __restrict__ prior_value) {
    __shared__ double s_sum[256];
    const uint32_t rows = min(*count, (uint32_t)capacity), nblk = rows / SGR_ROWS + (rows % SGR_ROWS != 0u ? 1u : 0u);
    double acc = 0.0;
    uint32_t k = threadIdx.x;
    for (; k + 7u * 256u < nblk; k += 8u * 256u) {
        double p[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) p[j] = partial[k + (uint32_t)j * 256u];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc += p[j];
    }
    for (; k < nblk; k += 256u) acc += partial[k];
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *prior_value = prior_weight * s_sum[0];
}

// ---------------------------------------------------------------------------
// host entries
// ---------------------------------------------------------------------------
extern "C" size_t mgr_skin_grid_bwd_workspace_bytes(int D, int H, int W, int max_count) {
    return sg_layout(D, H, W, max_count).total;
}

extern "C" int mgr_skin_grid_bwd(int N, const float* xyz, const float* grid, int D, int H, int W, int B, int grid_stride,
                                 const float* center3, const float* scale3, const float* dL_dw, const uint32_t* index,
                                 const uint32_t* index_count, int max_count, int32_t* out_voxel, float* out_grad,
                                 uint32_t* out_count, int capacity, void* workspace, size_t workspace_bytes, void* stream_) {
    if (N < 0 || D <= 0 || H <= 0 || W <= 0) return mgr_fail(MGR_EINVAL, "mgr_skin_grid_bwd: bad sizes");
    if (B <= 0 || B > MGR_MAX_BONES) return mgr_fail(MGR_EINVAL, "mgr_skin_grid_bwd: B must be 1 .. MGR_MAX_BONES");
    if (max_count < 0) return mgr_fail(MGR_EINVAL, "mgr_skin_grid_bwd: max_count < 0");
    if (index && !index_count) return mgr_fail(MGR_EINVAL, "mgr_skin_grid_bwd: index without index_count");
    if (!index) max_count = N;
    if (grid_stride != B && grid_stride != SKIN_BP) return mgr_fail(MGR_EINVAL, "mgr_skin_grid_bwd: grid_stride must be B or 24");
    const bool fast = grid_stride == SKIN_BP && B <= SKIN_BP && ((uintptr_t)grid & 15) == 0;
    if (!fast && grid_stride != B) return mgr_fail(MGR_EINVAL, "mgr_skin_grid_bwd: padded grid must be 16-byte aligned with B <= 24");
    const SgLayout L = sg_layout(D, H, W, max_count);
    if (L.nvox >= ((size_t)1 << 31) || (size_t)max_count >= ((size_t)1 << 27))
        return mgr_fail(MGR_EINVAL, "mgr_skin_grid_bwd: D*H*W must be below 2^31 and max_count below 2^27");
    if (capacity < 0 || (size_t)capacity < L.rows) return mgr_fail(MGR_EINVAL, "mgr_skin_grid_bwd: capacity below min(8 * max_count, D*H*W)");
    if (!out_count || !out_voxel || !out_grad) return mgr_fail(MGR_EINVAL, "mgr_skin_grid_bwd: null output");
    if (workspace_bytes < L.total || !workspace) return mgr_fail(MGR_ENOMEM, "mgr_skin_grid_bwd: workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    if (max_count == 0) {
        MGR_HIP(hipMemsetAsync(out_count, 0, 4, stream));
        return MGR_OK;
    }
    if (!xyz || !grid || !center3 || !scale3 || !dL_dw) return mgr_fail(MGR_EINVAL, "mgr_skin_grid_bwd: null pointer");
    char* ws = (char*)workspace;
    uint32_t* cnt = (uint32_t*)(ws + L.cnt);
    uint2* bsum = (uint2*)(ws + L.bsum);
    uint32_t* seg_off = (uint32_t*)(ws + L.seg_off);
    uint32_t* mask = (uint32_t*)(ws + L.mask);
    float* rbuf = (float*)(ws + L.r);
    uint32_t *rec_n = (uint32_t*)(ws + L.rec_n), *rec_t = (uint32_t*)(ws + L.rec_t), *srt_t = (uint32_t*)(ws + L.srt_t);
    float *rec_w = (float*)(ws + L.rec_w), *srt_w = (float*)(ws + L.srt_w);
    const int eblocks = (max_count + 255) / 256, nblk = (int)L.nblk;
    MGR_HIP(hipMemsetAsync(cnt, 0, L.nvox * 4, stream));
    if (fast) {
        MGR_PROF("k_sg_prep24", stream);
        hipLaunchKernelGGL(k_sg_prep24, dim3(eblocks), dim3(256), 0, stream, N, xyz, (const float4*)grid, D, H, W, B, center3, scale3,
                           dL_dw, index, index_count, max_count, cnt, mask, rbuf);
    } else {
        MGR_PROF("k_sg_prep", stream);
        hipLaunchKernelGGL(k_sg_prep, dim3(eblocks), dim3(256), 0, stream, N, xyz, grid, D, H, W, B, center3, scale3, dL_dw, index,
                           index_count, max_count, cnt, mask, rbuf);
    }
    { MGR_PROF("k_sg_scan_a", stream); hipLaunchKernelGGL(k_sg_scan_a, dim3(nblk), dim3(256), 0, stream, L.nvox, cnt, bsum); }
    { MGR_PROF("k_sg_scan_b", stream); hipLaunchKernelGGL(k_sg_scan_b, dim3(1), dim3(1024), 0, stream, nblk, bsum, seg_off, out_count, (uint32_t)L.rows); }
    { MGR_PROF("k_sg_scan_c", stream); hipLaunchKernelGGL(k_sg_scan_c, dim3(nblk), dim3(256), 0, stream, L.nvox, cnt, bsum, seg_off, out_voxel, (uint32_t)L.rows); }
    { MGR_PROF("k_sg_scatter", stream); hipLaunchKernelGGL(k_sg_scatter, dim3(eblocks), dim3(256), 0, stream, N, xyz, D, H, W, center3, scale3, index,
                         max_count, mask, cnt, rec_n, rec_t, rec_w, (uint32_t)L.pairs); }
    const size_t pblocks = (L.pairs + 255) / 256, rblocks = (L.rows + 3) / 4;
    { MGR_PROF("k_sg_rank", stream); hipLaunchKernelGGL(k_sg_rank, dim3((unsigned)(pblocks < 4096 ? pblocks : 4096)), dim3(256), 0, stream, out_count, seg_off,
                         rec_n, rec_t, rec_w, srt_t, srt_w); }
    { MGR_PROF("k_sg_reduce", stream); hipLaunchKernelGGL(k_sg_reduce, dim3((unsigned)(rblocks < 4096 ? rblocks : 4096)), dim3(256), 0, stream, out_count, seg_off,
                         srt_t, srt_w, rbuf, out_grad, B, grid_stride); }
    MGR_LAUNCH_CHECK("skin_grid_bwd", stream, 0);
    return MGR_OK;
}

extern "C" int mgr_skin_grid_adam(const int32_t* voxel, const float* grad, const uint32_t* count, int capacity, float* grid,
                                  int grid_stride, int B, float* exp_avg, float* exp_avg_sq, double lr, double beta1, double beta2,
                                  double eps, int step, int clamp, float clamp_min, void* stream_) {
    if (B <= 0 || B > MGR_MAX_BONES || (grid_stride != B && grid_stride != SKIN_BP) || grid_stride < B)
        return mgr_fail(MGR_EINVAL, "mgr_skin_grid_adam: B must be 1 .. MGR_MAX_BONES and grid_stride B or 24");
    if (capacity < 0 || step < 1) return mgr_fail(MGR_EINVAL, "mgr_skin_grid_adam: capacity < 0 or step < 1");
    if (capacity == 0) return MGR_OK;
    if (!voxel || !grad || !count || !grid || !exp_avg || !exp_avg_sq) return mgr_fail(MGR_EINVAL, "mgr_skin_grid_adam: null pointer");
    hipStream_t stream = (hipStream_t)stream_;
    const float step_size = sg_adam_step_size(lr, beta1, beta2, step);
    const size_t threads = (size_t)capacity * B;
    { MGR_PROF("k_sg_adam", stream); hipLaunchKernelGGL(k_sg_adam, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, voxel, grad, count, capacity,
                         grid, grid_stride, B, exp_avg, exp_avg_sq, step_size, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, clamp, clamp_min); }
    MGR_LAUNCH_CHECK("k_sg_adam", stream, 0);
    return MGR_OK;
}

static inline size_t sg_refine_blocks(int capacity) { return ((size_t)(capacity > 0 ? capacity : 0) + SGR_ROWS - 1) / SGR_ROWS; }

extern "C" size_t mgr_skin_grid_refine_workspace_bytes(int capacity) {
    const size_t nblk = sg_refine_blocks(capacity);
    return nblk ? mgr_align(nblk * sizeof(double)) : 0;       // one fp64 partial per workgroup
}

extern "C" int mgr_skin_grid_refine(const int32_t* voxel, const float* grad, const uint32_t* count, int capacity, float* grid,
                                    const float* grid0, int grid_stride, int B, float* exp_avg, float* exp_avg_sq, double lr,
                                    double beta1, double beta2, double eps, int step, int clamp, float clamp_min, double prior_weight,
                                    int project, float min_sum, double* prior_value, void* workspace, size_t workspace_bytes,
                                    void* stream_) {
    if (B <= 0 || B > MGR_MAX_BONES || (grid_stride != B && grid_stride != SKIN_BP) || grid_stride < B)
        return mgr_fail(MGR_EINVAL, "mgr_skin_grid_refine: B must be 1 .. MGR_MAX_BONES and grid_stride B or 24");
    if (capacity < 0 || step < 1) return mgr_fail(MGR_EINVAL, "mgr_skin_grid_refine: capacity < 0 or step < 1");
    if (!(prior_weight >= 0.0) || !std::isfinite(prior_weight)) return mgr_fail(MGR_EINVAL, "mgr_skin_grid_refine: prior_weight must be finite and >= 0");
    const bool prior = prior_weight != 0.0;
    if (prior && (!grid0 || !prior_value)) return mgr_fail(MGR_EINVAL, "mgr_skin_grid_refine: a prior needs grid0 and prior_value");
    if (!(min_sum >= 0.f)) return mgr_fail(MGR_EINVAL, "mgr_skin_grid_refine: min_sum < 0");
    if (capacity > 0 && (!voxel || !grad || !count || !grid || !exp_avg || !exp_avg_sq)) return mgr_fail(MGR_EINVAL, "mgr_skin_grid_refine: null pointer");
    const size_t need = mgr_skin_grid_refine_workspace_bytes(capacity);
    if (workspace_bytes < need || (need && !workspace)) return mgr_fail(MGR_ENOMEM, "mgr_skin_grid_refine: workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    if (capacity == 0 || !prior) {
        if (prior_value) MGR_HIP(hipMemsetAsync(prior_value, 0, sizeof(double), stream));
        if (capacity == 0) return MGR_OK;
    }
    const float step_size = sg_adam_step_size(lr, beta1, beta2, step);
    const float omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2), w2 = (float)(2.0 * prior_weight);
    const size_t cblk = sg_refine_blocks(capacity);
    const unsigned nblk = (unsigned)(cblk < SGR_MAX_BLOCKS ? cblk : SGR_MAX_BLOCKS);
    double* partial = (double*)workspace;
    if (prior) {
        { MGR_PROF("k_sg_refine", stream); hipLaunchKernelGGL(k_sg_refine<true>, dim3(nblk), dim3(256), 0, stream, voxel, grad, count, capacity, grid, grid0,
                             grid_stride, B, exp_avg, exp_avg_sq, step_size, omb1, omb2, (float)eps, clamp, clamp_min, w2, project, min_sum, partial); }
        { MGR_PROF("k_sg_refine_fold", stream); hipLaunchKernelGGL(k_sg_refine_fold, dim3(1), dim3(256), 0, stream, partial, count, capacity, prior_weight, prior_value); }
    } else {
        MGR_PROF("k_sg_refine", stream);
        hipLaunchKernelGGL(k_sg_refine<false>, dim3(nblk), dim3(256), 0, stream, voxel, grad, count, capacity, grid, grid0, grid_stride, B,
                           exp_avg, exp_avg_sq, step_size, omb1, omb2, (float)eps, clamp, clamp_min, w2, project, min_sum, partial);
    }
    MGR_LAUNCH_CHECK("k_sg_refine", stream, 0);
    return MGR_OK;
}

// mask[i] = 1 where row i of dL_dw (n,B) holds a non-zero entry (NaN != 0: a non-finite row is listed), else 0
__global__ __launch_bounds__(256) void k_sg_rows_mask(int n, int B, const float* __restrict__ dL_dw, uint8_t* __restrict__ mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* r = dL_dw + (size_t)i * B;
    bool any = false;
    for (int c = 0; c < B; ++c) any = any || (r[c] != 0.0f);
    mask[i] = any ? 1 : 0;
}

extern "C" int mgr_skin_rows_mask(int n, int B, const float* dL_dw, uint8_t* mask, void* stream_) {
    if (n < 0 || B <= 0 || B > MGR_MAX_BONES) return mgr_fail(MGR_EINVAL, "mgr_skin_rows_mask: n < 0 or B outside 1 .. MGR_MAX_BONES");
    if (n == 0) return MGR_OK;
    if (!dL_dw || !mask) return mgr_fail(MGR_EINVAL, "mgr_skin_rows_mask: null pointer");
    hipStream_t stream = (hipStream_t)stream_;
    { MGR_PROF("k_sg_rows_mask", stream); hipLaunchKernelGGL(k_sg_rows_mask, dim3((unsigned)n / 256u + ((unsigned)n % 256u != 0u ? 1u : 0u)), dim3(256), 0, stream, n, B, dL_dw, mask); }
    MGR_LAUNCH_CHECK("k_sg_rows_mask", stream, 0);
    return MGR_OK;
}
