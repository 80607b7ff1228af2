// Hand <-> object contact distance for gfx950: for every point of pt1 the distance to, and the index
// of, its nearest point of pt2.
//
// Replaces get_contact_dist (taichi kernel calculate_distances) and get_contact_map (chunked
// torch.cdist(...).min) of /root/reference/src/utils/gaussian_utils.py:514-549, used by get_cmap
// (:571-577) for the contact renders of src/modules/composite.py:143-214.
// Semantics of the reference loop, kept exactly: fp32, dist = sqrt(dx^2 + dy^2 + dz^2) summed in that
// order, a candidate replaces the running minimum only when its *rooted* distance is strictly
// smaller (so among equal distances the lowest index wins), min_dist starts at 1e9.
//
// Brute force, tiled: a workgroup holds 512 points of pt1 in registers (two per thread) and streams
// pt2 through LDS 1024 points at a time, every LDS read (one broadcast ds_read_b128) serving both
// points of all 256 threads.  The square root is only taken for candidates that already beat the
// running minimum of the squared distance (a necessary condition).  pt2 is split into S segments
// across workgroups to fill the chip; a second kernel merges the S partial results in segment
// order with the same strict comparison, which preserves the lowest-index rule.
#include "mgr_common.h"

#define CT_T 256
#define CT_TILE 1024

__device__ __forceinline__ void ct_try(float px, float py, float pz, const float4 q, uint32_t j, float& best2, float& best,
                                       uint32_t& idx) {
#pragma clang fp contract(off)   // the reference's sum is three rounded squares added in order, not FMAs
    const float dx = px - q.x, dy = py - q.y, dz = pz - q.z;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float d2 = (xx + yy) + zz;
    if (d2 < best2) {
        const float s = (float)sqrt((double)d2);  // correctly rounded fp32 root (v_sqrt_f32 alone is 1 ulp); rare path
        if (s < best) {
            best = s;
            idx = j;
        }
        best2 = d2;  // still necessary for any later strict improvement of the rooted distance
    }
}

__global__ __launch_bounds__(CT_T) void k_contact_partial(int N1, const float* __restrict__ pt1, int N2,
                                                          const float* __restrict__ pt2, int seg_len,
                                                          float* __restrict__ part_dist, uint32_t* __restrict__ part_idx) {
    __shared__ float4 s_pt[CT_TILE];
    const int tid = threadIdx.x;
    const int i0 = (blockIdx.x * CT_T + tid) * 2, i1 = i0 + 1;
    const int j_begin = blockIdx.y * seg_len, j_end = min(N2, j_begin + seg_len);
    float ax = 0.f, ay = 0.f, az = 0.f, bx = 0.f, by = 0.f, bz = 0.f;
    if (i0 < N1) { ax = pt1[3 * (size_t)i0]; ay = pt1[3 * (size_t)i0 + 1]; az = pt1[3 * (size_t)i0 + 2]; }
    if (i1 < N1) { bx = pt1[3 * (size_t)i1]; by = pt1[3 * (size_t)i1 + 1]; bz = pt1[3 * (size_t)i1 + 2]; }
    float a_best = 1e9f, a_best2 = 1e18f, b_best = 1e9f, b_best2 = 1e18f;
    uint32_t a_idx = 0, b_idx = 0;
    for (int j0 = j_begin; j0 < j_end; j0 += CT_TILE) {
        const int n = min(CT_TILE, j_end - j0);
        __syncthreads();
        for (int k = tid; k < n; k += CT_T) {
            const float* p = pt2 + 3 * (size_t)(j0 + k);
            s_pt[k] = make_float4(p[0], p[1], p[2], 0.f);
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < n; ++k) {
            const float4 q = s_pt[k];
            ct_try(ax, ay, az, q, (uint32_t)(j0 + k), a_best2, a_best, a_idx);
            ct_try(bx, by, bz, q, (uint32_t)(j0 + k), b_best2, b_best, b_idx);
        }
    }
    const size_t row = (size_t)blockIdx.y * N1;
    if (i0 < N1) { part_dist[row + i0] = a_best; part_idx[row + i0] = a_idx; }
    if (i1 < N1) { part_dist[row + i1] = b_best; part_idx[row + i1] = b_idx; }
}

__global__ __launch_bounds__(256) void k_contact_merge(int N1, int S, const float* __restrict__ part_dist,
                                                       const uint32_t* __restrict__ part_idx, float* __restrict__ out_dist,
                                                       int32_t* __restrict__ out_idx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N1) return;
    float best = 1e9f;
    uint32_t idx = 0;
    for (int s = 0; s < S; ++s) {  // ascending segments = ascending indices: strict < keeps the lowest index of a tie
        const float d = part_dist[(size_t)s * N1 + i];
        if (d < best) {
            best = d;
            idx = part_idx[(size_t)s * N1 + i];
        }
    }
    out_dist[i] = best;
    if (out_idx) out_idx[i] = (int32_t)idx;
}

static int ct_segments(int N1, int N2) {
    const long long blocks_i = ((long long)N1 + 2 * CT_T - 1) / (2 * CT_T);
    long long S = (2048 + blocks_i - 1) / blocks_i;            // aim at ~2k workgroups
    const long long max_s = ((long long)N2 + CT_TILE - 1) / CT_TILE;  // at least one LDS tile per segment
    if (S > max_s) S = max_s;
    if (S > 64) S = 64;
    if (S < 1) S = 1;
    return (int)S;
}

extern "C" size_t mgr_contact_workspace_bytes(int N1, int N2) {
    if (N1 <= 0 || N2 < 0) return 0;
    return (size_t)ct_segments(N1, N2) * (size_t)N1 * 8 + 256;
}

extern "C" int mgr_contact_dist(int N1, const float* pt1, int N2, const float* pt2, float* out_dist, int32_t* out_idx,
                                void* workspace, size_t workspace_bytes, void* stream_) {
    if (N1 < 0 || N2 < 0) return mgr_fail(MGR_EINVAL, "mgr_contact_dist: bad sizes");
    if (N1 == 0) return MGR_OK;
    if (!pt1 || !out_dist || (N2 > 0 && !pt2) || !workspace) return mgr_fail(MGR_EINVAL, "mgr_contact_dist: null pointer");
    if (workspace_bytes < mgr_contact_workspace_bytes(N1, N2)) return mgr_fail(MGR_ENOMEM, "mgr_contact_dist: workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    const int S = ct_segments(N1, N2);
    int seg_len = (N2 + S - 1) / S;
    seg_len = (seg_len + CT_TILE - 1) / CT_TILE * CT_TILE;
    if (seg_len < CT_TILE) seg_len = CT_TILE;
    float* pd = (float*)workspace;
    uint32_t* pi = (uint32_t*)((char*)workspace + (size_t)S * N1 * 4);
    {
        MGR_PROF("k_contact_partial", stream);
        hipLaunchKernelGGL(k_contact_partial, dim3((N1 + 2 * CT_T - 1) / (2 * CT_T), S), dim3(CT_T), 0, stream, N1, pt1, N2, pt2,
                           seg_len, pd, pi);
    }
    hipLaunchKernelGGL(k_contact_merge, dim3((N1 + 255) / 256), dim3(256), 0, stream, N1, S, (const float*)pd,
                       (const uint32_t*)pi, out_dist, out_idx);
    MGR_LAUNCH_CHECK("k_contact", stream, 0);
    return MGR_OK;
}

// ---------------------------------------------------------------------------------------------------
// Near search on a hashed uniform grid (mgr_contact_near) and the colour epilogue (mgr_contact_colors).
//
// A contact map (get_cmap, gaussian_utils.py:571-577) only needs distances below c_thresh: everything
// farther maps to the value 0.  pt2 is counting-sorted on the device into a hash table of cells of
// edge h slightly above c_thresh (the table is sized from N2, never from the extent: a far outlier
// costs one bucket), and every point of pt1 visits the cells its ball of radius r touches -- at
// most 3 per axis.  Same arithmetic as ct_try above; cells are not visited in index order, so the
// running minimum is the lexicographic minimum of (rooted distance, index), which is what the
// ascending loop with strict '<' yields, does not depend on the order in which the atomics filled a
// cell, and makes a bucket that is visited twice (two cells of one hash) harmless.
//
// Why no contact is missed: value > 0 needs the rooted fp32 distance d < c, and |fl(px - qx)| <= d
// (rounded squares and the rounded sum are monotone, and the correctly rounded root of fl(t*t) is |t|),
// hence |px - qx| < r = c * (1 + 1e-4) in real numbers.  Cell coordinates are floor(fl64(x * 1/h)),
// clamped, which is monotone in x, and fl64(px - r) <= qx <= fl64(px + r); so q's coordinate lies
// between those of px - r and px + r.  With h = 1.001 r that range has at most three cells.
// ---------------------------------------------------------------------------------------------------
#define CN_T 256
#define CN_COORD_MAX 1099511627776.0  // 2^40 cells from the origin; farther (and NaN) coordinates share the border cell

__device__ __forceinline__ long long cn_coord(double v, double inv_h) {
    const double c = floor(v * inv_h);
    return (long long)fmin(fmax(c, -CN_COORD_MAX), CN_COORD_MAX);  // fmax(NaN, x) = x: a NaN point gets a defined cell
}

__device__ __forceinline__ uint32_t cn_hash(long long cx, long long cy, long long cz, uint32_t mask) {
    return (((uint32_t)cx * 73856093u) ^ ((uint32_t)cy * 19349663u) ^ ((uint32_t)cz * 83492791u)) & mask;
}

__global__ __launch_bounds__(CN_T) void k_cn_count(int N2, const float* __restrict__ pt2, double inv_h, uint32_t mask,
                                                   uint32_t* __restrict__ cnt, uint32_t* __restrict__ bucket) {
    const int j = blockIdx.x * CN_T + threadIdx.x;
    if (j >= N2) return;
    const uint32_t b = cn_hash(cn_coord((double)pt2[3 * (size_t)j], inv_h), cn_coord((double)pt2[3 * (size_t)j + 1], inv_h),
                               cn_coord((double)pt2[3 * (size_t)j + 2], inv_h), mask);
    bucket[j] = b;
    atomicAdd(&cnt[b], 1u);
}

// Exclusive scan of the bucket counts, 1024 buckets (256 threads x uint4, coalesced) per workgroup: k_cn_blocksum leaves one sum
// per workgroup, k_cn_scan adds up the sums before its own (at most 4096 of them) and scans its 1024 buckets.
// start[ncells] = N2; the counts become the zeroed scatter cursors.  ncells is a power of two >= 1024.
__global__ __launch_bounds__(256) void k_cn_blocksum(const uint32_t* __restrict__ cnt, uint32_t* __restrict__ part) {
    __shared__ uint32_t s_w[4];
    const int tid = threadIdx.x;
    const uint4 v = ((const uint4*)cnt)[blockIdx.x * 256 + tid];
    uint32_t s = v.x + v.y + v.z + v.w;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
    if ((tid & 63) == 0) s_w[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) part[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ __launch_bounds__(256) void k_cn_scan(int ncells, int N2, uint32_t* __restrict__ cnt, const uint32_t* __restrict__ part,
                                                 uint32_t* __restrict__ start) {
    __shared__ uint32_t s_off[4], s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    uint32_t off = 0;
    for (int k = tid; k < (int)blockIdx.x; k += 256) off += part[k];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) off += __shfl_xor(off, d, 64);
    const uint4 v = ((const uint4*)cnt)[blockIdx.x * 256 + tid];
    const uint32_t s = v.x + v.y + v.z + v.w;
    uint32_t inc = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    if (lane == 0) s_off[w] = off;
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    uint32_t e = s_off[0] + s_off[1] + s_off[2] + s_off[3] + inc - s;
    for (int k = 0; k < w; ++k) e += s_w[k];
    ((uint4*)start)[blockIdx.x * 256 + tid] = make_uint4(e, e + v.x, e + v.x + v.y, e + v.x + v.y + v.z);
    ((uint4*)cnt)[blockIdx.x * 256 + tid] = make_uint4(0u, 0u, 0u, 0u);
    if (blockIdx.x == 0 && tid == 0) start[ncells] = (uint32_t)N2;
}

__global__ __launch_bounds__(CN_T) void k_cn_scatter(int N2, const float* __restrict__ pt2, const uint32_t* __restrict__ bucket,
                                                     const uint32_t* __restrict__ start, uint32_t* __restrict__ cursor,
                                                     float4* __restrict__ sorted) {
    const int j = blockIdx.x * CN_T + threadIdx.x;
    if (j >= N2) return;
    const uint32_t b = bucket[j];
    const uint32_t pos = start[b] + atomicAdd(&cursor[b], 1u);  // pos < start[b + 1] <= N2: cursor counts what k_cn_count counted
    sorted[pos] = make_float4(pt2[3 * (size_t)j], pt2[3 * (size_t)j + 1], pt2[3 * (size_t)j + 2], __uint_as_float((uint32_t)j));
}

__device__ __forceinline__ float cn_value(float dist, float c) {
#pragma clang fp contract(off)
    const float q = fminf(fmaxf(dist, 0.f), c) / c;  // IEEE division (hipcc rounds fp32 '/' correctly by default)
    return 1.0f - q;
}

__global__ __launch_bounds__(CN_T) void k_cn_query(int N1, const float* __restrict__ pt1, int N2, float c, double r, double inv_h,
                                                   uint32_t mask, const uint32_t* __restrict__ start,
                                                   const float4* __restrict__ sorted, float* __restrict__ out_value,
                                                   int32_t* __restrict__ out_idx, float* __restrict__ out_dist) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * CN_T + threadIdx.x;
    if (i >= N1) return;
    const float px = pt1[3 * (size_t)i], py = pt1[3 * (size_t)i + 1], pz = pt1[3 * (size_t)i + 2];
    float best = 1e9f;
    float lim2 = c * c * 1.000001f;  // d2 above it roots to >= c: value 0 whatever it is
    uint32_t idx = 0xFFFFFFFFu;
    if (N2 > 0) {
        const long long x0 = cn_coord((double)px - r, inv_h), y0 = cn_coord((double)py - r, inv_h), z0 = cn_coord((double)pz - r, inv_h);
        // at most three cells per axis (header comment); the min() only bounds the loops should that reasoning ever be broken
        const long long x1 = min(cn_coord((double)px + r, inv_h), x0 + 2), y1 = min(cn_coord((double)py + r, inv_h), y0 + 2),
                        z1 = min(cn_coord((double)pz + r, inv_h), z0 + 2);
        for (long long cz = z0; cz <= z1; ++cz)
            for (long long cy = y0; cy <= y1; ++cy)
                for (long long cx = x0; cx <= x1; ++cx) {
                    const uint32_t b = cn_hash(cx, cy, cz, mask);
                    const uint32_t s = start[b], e = start[b + 1];
                    for (uint32_t k = s; k < e; ++k) {
                        const float4 q = sorted[k];
                        const float dx = px - q.x, dy = py - q.y, dz = pz - q.z;
                        const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
                        const float d2 = (xx + yy) + zz;
                        if (d2 <= lim2) {  // false for NaN: a NaN point is nobody's neighbour
                            const float sq = (float)sqrt((double)d2);
                            const uint32_t j = __float_as_uint(q.w);
                            if (sq < best || (sq == best && j < idx)) {
                                best = sq;
                                idx = j;
                                // every d2 that roots to `best` is below best^2 (1 + 2^-22); the floor keeps denormal squares in
                                lim2 = fmaxf(sq * sq * 1.000001f, 1e-30f);
                            }
                        }
                    }
                }
    }
    const float v = cn_value(best, c);
    const bool hit = v > 0.f;
    out_value[i] = v;
    out_idx[i] = hit ? (int32_t)idx : -1;
    if (out_dist) out_dist[i] = hit ? best : 1e9f;
}

static uint32_t cn_cells(int N2) {
    uint32_t n = 1024;
    while (n < 2u * (uint32_t)(N2 > 0 ? N2 : 0) && n < (1u << 22)) n <<= 1;
    return n;
}

extern "C" size_t mgr_contact_near_workspace_bytes(int N1, int N2) {
    if (N1 <= 0 || N2 <= 0) return 0;
    const size_t nc = cn_cells(N2);
    return mgr_align(nc * 4) + mgr_align((nc + 1) * 4) + mgr_align(nc / 1024 * 4) + mgr_align((size_t)N2 * 4) + mgr_align((size_t)N2 * 16);
}

extern "C" int mgr_contact_near(int N1, const float* pt1, int N2, const float* pt2, float c_thresh, float* out_value,
                                int32_t* out_idx, float* out_dist, void* workspace, size_t workspace_bytes, void* stream_) {
    if (N1 < 0 || N2 < 0) return mgr_fail(MGR_EINVAL, "mgr_contact_near: bad sizes");
    if (!(c_thresh > 0.f) || !(c_thresh < 1e30f)) return mgr_fail(MGR_EINVAL, "mgr_contact_near: c_thresh must be positive and finite");
    if (N1 == 0) return MGR_OK;
    if (!pt1 || !out_value || !out_idx || (N2 > 0 && (!pt2 || !workspace))) return mgr_fail(MGR_EINVAL, "mgr_contact_near: null pointer");
    if (workspace_bytes < mgr_contact_near_workspace_bytes(N1, N2)) return mgr_fail(MGR_ENOMEM, "mgr_contact_near: workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    const uint32_t nc = cn_cells(N2);
    const double r = (double)c_thresh * 1.0001, inv_h = 1.0 / (r * 1.001);
    char* ws = (char*)workspace;
    size_t o = 0;
    uint32_t* cnt = (uint32_t*)(ws + o);     o += mgr_align((size_t)nc * 4);
    uint32_t* start = (uint32_t*)(ws + o);   o += mgr_align(((size_t)nc + 1) * 4);
    uint32_t* part = (uint32_t*)(ws + o);    o += mgr_align((size_t)nc / 1024 * 4);
    uint32_t* bucket = (uint32_t*)(ws + o);  o += mgr_align((size_t)N2 * 4);
    float4* sorted = (float4*)(ws + o);
    if (N2 > 0) {
        const int blocks2 = (N2 + CN_T - 1) / CN_T;
        MGR_HIP(hipMemsetAsync(cnt, 0, (size_t)nc * 4, stream));
        { MGR_PROF("k_cn_count", stream); hipLaunchKernelGGL(k_cn_count, dim3(blocks2), dim3(CN_T), 0, stream, N2, pt2, inv_h, nc - 1, cnt, bucket); }
        { MGR_PROF("k_cn_blocksum", stream); hipLaunchKernelGGL(k_cn_blocksum, dim3(nc / 1024), dim3(256), 0, stream, (const uint32_t*)cnt, part); }
        { MGR_PROF("k_cn_scan", stream); hipLaunchKernelGGL(k_cn_scan, dim3(nc / 1024), dim3(256), 0, stream, (int)nc, N2, cnt, (const uint32_t*)part, start); }
        { MGR_PROF("k_cn_scatter", stream); hipLaunchKernelGGL(k_cn_scatter, dim3(blocks2), dim3(CN_T), 0, stream, N2, pt2, (const uint32_t*)bucket, (const uint32_t*)start, cnt, sorted); }
    }
    {
        MGR_PROF("k_cn_query", stream);
        hipLaunchKernelGGL(k_cn_query, dim3((N1 + CN_T - 1) / CN_T), dim3(CN_T), 0, stream, N1, pt1, N2, c_thresh, r, inv_h, nc - 1,
                           (const uint32_t*)start, (const float4*)sorted, out_value, out_idx, out_dist);
    }
    MGR_LAUNCH_CHECK("k_cn", stream, 0);
    return MGR_OK;
}

// value = 1 - clamp(dist, 0, c_thresh) / c_thresh (get_cmap, gaussian_utils.py:573-574) with an IEEE fp32 division, for a
// distance that some other search produced (get_cmap on the brute-force search)
__global__ __launch_bounds__(256) void k_contact_values(int N, const float* __restrict__ dist, float c, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) out[i] = cn_value(dist[i], c);
}

extern "C" int mgr_contact_values(int N, const float* dist, float c_thresh, float* out_value, void* stream_) {
    if (N < 0) return mgr_fail(MGR_EINVAL, "mgr_contact_values: bad sizes");
    if (!(c_thresh > 0.f) || !(c_thresh < 1e30f)) return mgr_fail(MGR_EINVAL, "mgr_contact_values: c_thresh must be positive and finite");
    if (N == 0) return MGR_OK;
    if (!dist || !out_value) return mgr_fail(MGR_EINVAL, "mgr_contact_values: null pointer");
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(k_contact_values, dim3((N + 255) / 256), dim3(256), 0, stream, N, dist, c_thresh, out_value);
    MGR_LAUNCH_CHECK("k_contact_values", stream, 0);
    return MGR_OK;
}

// Colour epilogue: what matplotlib's Colormap.__call__ does with a float32 array on a 256-entry map
// (get_colors_from_cmap, src/utils/vis_util.py:22-25) and the blends of Composite.render_contacts
// (src/modules/composite.py:143-214), one thread per point.
__global__ __launch_bounds__(256) void k_contact_colors(int N, const float* __restrict__ value, const float* __restrict__ lut,
                                                        const float* __restrict__ base, float alpha, float one_minus_alpha,
                                                        const float* __restrict__ table, int M, const int32_t* __restrict__ idx_nn,
                                                        float* __restrict__ out) {
#pragma clang fp contract(off)   // rgb * alpha + (1 - alpha) * cmap is two rounded products and a rounded sum in the reference
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float v = value[n];
    float r = 0.f, g = 0.f, b = 0.f;
    if (table) {  // NOCS renders: the table's colour where there is contact, black elsewhere
        const int m = idx_nn ? idx_nn[n] : n;
        if (v > 0.f && m >= 0 && m < M) { r = table[3 * (size_t)m]; g = table[3 * (size_t)m + 1]; b = table[3 * (size_t)m + 2]; }
    } else {
        if (v == v) {  // NaN is matplotlib's "bad" colour (0,0,0)
            const float s = v * 256.0f;
            const int k = !(s > 0.f) ? 0 : (s >= 255.f ? 255 : (int)s);  // under -> entry 0, 1.0 and over (+inf) -> entry 255
            r = lut[3 * k]; g = lut[3 * k + 1]; b = lut[3 * k + 2];
        }
        if (base) {
            r = base[3 * (size_t)n] * alpha + one_minus_alpha * r;
            g = base[3 * (size_t)n + 1] * alpha + one_minus_alpha * g;
            b = base[3 * (size_t)n + 2] * alpha + one_minus_alpha * b;
        }
    }
    out[3 * (size_t)n] = r; out[3 * (size_t)n + 1] = g; out[3 * (size_t)n + 2] = b;
}

extern "C" int mgr_contact_colors(int N, const float* value, const float* lut, const float* base, float alpha, float one_minus_alpha,
                                  const float* table, int M, const int32_t* idx_nn, float* out, void* stream_) {
    if (N < 0 || M < 0) return mgr_fail(MGR_EINVAL, "mgr_contact_colors: bad sizes");
    if (N == 0) return MGR_OK;
    if (!value || !out || (!lut && !table)) return mgr_fail(MGR_EINVAL, "mgr_contact_colors: null pointer");
    if (table && !idx_nn && M < N) return mgr_fail(MGR_EINVAL, "mgr_contact_colors: table has fewer rows than there are points");
    hipStream_t stream = (hipStream_t)stream_;
    MGR_PROF("k_contact_colors", stream);
    hipLaunchKernelGGL(k_contact_colors, dim3((N + 255) / 256), dim3(256), 0, stream, N, value, lut, base, alpha, one_minus_alpha, table, M,
                       idx_nn, out);
    MGR_LAUNCH_CHECK("k_contact_colors", stream, 0);
    return MGR_OK;
}
