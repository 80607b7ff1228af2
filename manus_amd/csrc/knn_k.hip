// Exact k nearest neighbours of every point among the points themselves (k <= MGR_KNN_MAX_K) and the Local Outlier
// Probability (LoOP; Kriegel, Kroeger, Schubert, Zimek 2009) on those neighbourhoods: the device side of the reference's
// update_mask_based_on_outliers (src/utils/gaussian_utils.py:557-568, MeshLab's "select outliers" through pymeshlab).
//
// The search: the finite points are counting-sorted into a uniform grid whose cell edge follows k (about k / 16 points per
// cell), one wave answers one query, and the queries are taken in sorted-cell order, so the four waves of a workgroup read
// the same cell runs.  A wave walks Chebyshev rings of cells like k_knn_query (knn.hip); its 64 lanes load 64 consecutive
// points of a run, form the 64-bit key (d2 bits << 32 | index) -- non-negative floats order as unsigned integers, so key
// order is (d2, index) order -- and append the keys below the current bound to the wave's LDS buffer (ballot + popcount).
// When the buffer is nearly full, or a ring ends with at least k candidates, a wave-level radix select (8-bit digits, LDS
// histogram) keeps the k smallest keys and the k-th becomes the bound.  The walk stops when the k-th distance is provably
// final; the k keys are bitonic-sorted in LDS.  The buffer only ever holds a superset of the answer, so a cell with more
// points than the buffer (thousands of coincident points) just selects more often.  The order of the points inside a cell
// (an atomic cursor) decides when a select runs, never what survives it: results are the same bits run to run.
#include "mgr_common.h"

#define KK_WAVES 4

struct KKParams {
    uint32_t bmin[3], bmax[3];  // ordered-uint encoded bbox of the finite points
    float lo[3], h, inv_h;
    int dims[3];
    int ncells;
};

__device__ __forceinline__ uint32_t kk_f2ord(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float kk_ord2f(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}
__device__ __forceinline__ bool kk_finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

__global__ void k_kk_init(KKParams* P) {
    for (int k = 0; k < 3; ++k) {
        P->bmin[k] = 0xFFFFFFFFu;
        P->bmax[k] = 0u;
    }
}

__global__ __launch_bounds__(256) void k_kk_bbox(int N, const float* __restrict__ xyz, KKParams* P) {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) {
        const float v[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
        if (!kk_finite3(v[0], v[1], v[2])) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            mn[k] = fminf(mn[k], v[k]);
            mx[k] = fmaxf(mx[k], v[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            mn[k] = fminf(mn[k], __shfl_xor(mn[k], d, 64));
            mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], d, 64));
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (mn[k] <= mx[k]) {
                atomicMin(&P->bmin[k], kk_f2ord(mn[k]));
                atomicMax(&P->bmax[k], kk_f2ord(mx[k]));
            }
        }
    }
}

// cell edge from k: `per_cell` points per cell on average over the bounding box
__global__ void k_kk_setup(int N, float per_cell, int max_cells, KKParams* P) {
    float ext[3], vol = 1.f;
    for (int k = 0; k < 3; ++k) {
        const bool any = P->bmin[k] <= P->bmax[k];      // false: no finite point at all
        P->lo[k] = any ? kk_ord2f(P->bmin[k]) : 0.f;
        ext[k] = any ? kk_ord2f(P->bmax[k]) - P->lo[k] : 0.f;
        if (!(ext[k] > 0.f) || !isfinite(ext[k])) ext[k] = 0.f;
    }
    const float emax = fmaxf(ext[0], fmaxf(ext[1], ext[2]));
    for (int k = 0; k < 3; ++k) vol *= fmaxf(ext[k], 1e-3f * emax);
    const float target = fmaxf(1.f, (float)N / per_cell);
    float h = (vol > 0.f) ? cbrtf(vol / target) : 1.f;
    if (!(h > 0.f) || !isfinite(h)) h = 1.f;
    int d[3] = {1, 1, 1};
    for (int it = 0; it < 200; ++it) {
        long long tot = 1;
        for (int k = 0; k < 3; ++k) {
            const float c = floorf(ext[k] / h) + 1.f;
            d[k] = (int)fminf(fmaxf(c, 1.f), 2048.f);
            tot *= d[k];
        }
        if (tot <= max_cells) break;
        h *= 1.2f;
    }
    if ((long long)d[0] * d[1] * d[2] > max_cells) d[0] = d[1] = d[2] = 1, h = fmaxf(emax, 1e-30f) * 2.f;
    P->h = h;
    P->inv_h = 1.f / h;
    for (int k = 0; k < 3; ++k) P->dims[k] = d[k];
    P->ncells = d[0] * d[1] * d[2];
}

__device__ __forceinline__ int kk_cell(const KKParams* P, float x, float y, float z, int c[3]) {
    c[0] = min(P->dims[0] - 1, max(0, (int)((x - P->lo[0]) * P->inv_h)));
    c[1] = min(P->dims[1] - 1, max(0, (int)((y - P->lo[1]) * P->inv_h)));
    c[2] = min(P->dims[2] - 1, max(0, (int)((z - P->lo[2]) * P->inv_h)));
    return (c[2] * P->dims[1] + c[1]) * P->dims[0] + c[0];
}

__global__ __launch_bounds__(256) void k_kk_count(int N, const float* __restrict__ xyz, const KKParams* P,
                                                  uint32_t* __restrict__ cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
    if (!kk_finite3(x, y, z)) return;
    int c[3];
    atomicAdd(&cnt[kk_cell(P, x, y, z, c)], 1u);
}

// single-block exclusive scan; start[ncells] = number of finite points; cursor zeroed
__global__ __launch_bounds__(1024) void k_kk_scan(const KKParams* P, const uint32_t* __restrict__ cnt,
                                                  uint32_t* __restrict__ start, uint32_t* __restrict__ cursor) {
    __shared__ uint32_t s_part[1024];
    const int n = P->ncells, tid = threadIdx.x;
    const int per = (n + 1023) / 1024;
    const int b = min(n, tid * per), e = min(n, b + per);
    uint32_t s = 0;
    for (int k = b; k < e; ++k) s += cnt[k];
    s_part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int k = 0; k < 1024; ++k) {
            const uint32_t t = s_part[k];
            s_part[k] = run;
            run += t;
        }
        start[n] = run;
    }
    __syncthreads();
    uint32_t run = s_part[tid];
    for (int k = b; k < e; ++k) {
        start[k] = run;
        cursor[k] = 0;
        run += cnt[k];
    }
}

// finite points go to their cell; a point with a non-finite coordinate is nobody's neighbour and its own row is final here
__global__ __launch_bounds__(256) void k_kk_scatter(int N, int k, const float* __restrict__ xyz, const KKParams* P,
                                                    const uint32_t* __restrict__ start, uint32_t* __restrict__ cursor,
                                                    float4* __restrict__ sorted, float* __restrict__ out_d2,
                                                    int32_t* __restrict__ out_idx, float* __restrict__ out_sigma,
                                                    int32_t* __restrict__ out_count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
    if (!kk_finite3(x, y, z)) {
        for (int t = 0; t < k; ++t) {
            if (out_d2) out_d2[(size_t)i * k + t] = INFINITY;
            if (out_idx) out_idx[(size_t)i * k + t] = -1;
        }
        if (out_sigma) out_sigma[i] = __uint_as_float(0x7fc00000u);
        if (out_count) out_count[i] = 0;
        return;
    }
    int c[3];
    const int cell = kk_cell(P, x, y, z, c);
    const uint32_t pos = start[cell] + atomicAdd(&cursor[cell], 1u);
    sorted[pos] = make_float4(x, y, z, __int_as_float(i));
}

// LDS traffic between the lanes of ONE wave: the hardware serves a wave's LDS instructions in order; this keeps the compiler
// from moving memory accesses across the point and waits for the outstanding ones.
__device__ __forceinline__ void kk_wsync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned long long kk_wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// Keep the k smallest of the n distinct keys key[0 .. n) (k <= n), compacted to key[0 .. k) in unspecified order; returns
// the k-th smallest.  Radix select from the top byte down: per pass a 256-bin histogram of the keys that match the digits
// fixed so far; the pass stops early once a bucket's keys are all wanted.  Wave-uniform control flow throughout.
__device__ __forceinline__ unsigned long long kk_select(unsigned long long* key, uint32_t* hist, int n, int k, int lane) {
    unsigned long long prefix = 0ull;
    uint32_t want = (uint32_t)k;
    int shift = 56;
    for (;; shift -= 8) {
#pragma unroll
        for (int b = 0; b < 4; ++b) hist[4 * lane + b] = 0u;
        kk_wsync();
        for (int t = lane; t < n; t += 64) {
            const unsigned long long v = key[t];
            const bool match = shift == 56 || (v >> (shift + 8)) == prefix;
            if (match) atomicAdd(&hist[(uint32_t)(v >> shift) & 255u], 1u);
        }
        kk_wsync();
        const uint32_t c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
        const uint32_t tot = c0 + c1 + c2 + c3;
        const uint32_t incl = mgr_wave_incl_scan_u32(tot), excl = incl - tot;
        const unsigned long long hit = __ballot(excl < want && want <= incl);   // exactly one lane
        const int L = __builtin_ctzll(hit);
        uint32_t dig, before, cb;
        {
            uint32_t run = excl, d = 0u, bf = excl, cc = c0;
            const uint32_t cs[4] = {c0, c1, c2, c3};
            bool found = false;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (!found && want <= run + cs[b]) { d = (uint32_t)b; bf = run; cc = cs[b]; found = true; }
                run += cs[b];
            }
            dig = (uint32_t)__shfl((int)(4u * (uint32_t)lane + d), L, 64);
            before = (uint32_t)__shfl((int)bf, L, 64);
            cb = (uint32_t)__shfl((int)cc, L, 64);
        }
        prefix = (prefix << 8) | (unsigned long long)dig;
        want -= before;
        kk_wsync();                          // the histogram is read before the next pass clears it
        if (want == cb || shift == 0) break;   // the whole bucket is wanted (always true at shift 0: the keys are distinct)
    }
    int kept = 0;
    unsigned long long mx = 0ull;
    for (int base = 0; base < n; base += 64) {
        const int t = base + lane;
        const bool v = t < n;
        const unsigned long long key_t = v ? key[t] : ~0ull;
        const bool keep = v && (key_t >> shift) <= prefix;
        const unsigned long long bal = __ballot(keep);
        const int rank = __popcll(bal & ((1ull << lane) - 1ull));
        kk_wsync();                          // the chunk is read before any lane overwrites a slot of it
        if (keep) {
            key[kept + rank] = key_t;        // kept + rank <= t: never ahead of the unread part
            mx = key_t > mx ? key_t : mx;
        }
        kept += __popcll(bal);
    }
    kk_wsync();
    return kk_wave_max_u64(mx);
}

// one wave per finite point, in sorted-cell order
template <int KP>
__global__ __launch_bounds__(64 * KK_WAVES) void k_kk_query(int k, int include_self, const KKParams* P,
                                                           const uint32_t* __restrict__ start,
                                                           const float4* __restrict__ sorted, float* __restrict__ out_d2,
                                                           int32_t* __restrict__ out_idx, float* __restrict__ out_sigma,
                                                           int32_t* __restrict__ out_count) {
#pragma clang fp contract(off)
    constexpr int CAP = 3 * KP;
    __shared__ unsigned long long s_key[KK_WAVES][CAP];
    __shared__ uint32_t s_hist[KK_WAVES][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t q = blockIdx.x * KK_WAVES + wave;
    const uint32_t nfin = start[P->ncells];
    if (q >= nfin) return;                   // whole waves leave; no workgroup barrier below
    unsigned long long* key = s_key[wave];
    uint32_t* hist = s_hist[wave];
    const float4 me = sorted[q];
    const int i = __float_as_int(me.w);
    int c[3];
    kk_cell(P, me.x, me.y, me.z, c);
    const int dx_ = P->dims[0], dy_ = P->dims[1], dz_ = P->dims[2];
    const float h = P->h;
    unsigned long long bound = ~0ull;        // keys >= bound cannot be among the k smallest
    int cnt = 0;
    bool fresh = false;                      // the buffer holds exactly the k smallest so far and `bound` is the k-th
    const int rmax = max(dx_, max(dy_, dz_));
    for (int r = 0; r <= rmax; ++r) {
        const int z0 = max(0, c[2] - r), z1 = min(dz_ - 1, c[2] + r);
        const int y0 = max(0, c[1] - r), y1 = min(dy_ - 1, c[1] + r);
        const int x0 = max(0, c[0] - r), x1 = min(dx_ - 1, c[0] + r);
        for (int cz = z0; cz <= z1; ++cz)
            for (int cy = y0; cy <= y1; ++cy) {
                const bool shell_zy = (abs(cz - c[2]) == r) || (abs(cy - c[1]) == r);
                // on the shell the whole x-run belongs to ring r and is one run of `sorted`; otherwise its two end cells do
                const int nruns = shell_zy ? 1 : (r == 0 ? 1 : 2);
                for (int run = 0; run < nruns; ++run) {
                    int xa, xb;
                    if (shell_zy) { xa = x0; xb = x1; }
                    else { xa = xb = run == 0 ? c[0] - r : c[0] + r; if (xa < 0 || xa >= dx_) continue; }
                    const int row = (cz * dy_ + cy) * dx_;
                    const uint32_t s = start[row + xa], e = start[row + xb + 1];
                    for (uint32_t base = s; base < e; base += 64) {
                        const uint32_t p = base + (uint32_t)lane;
                        bool keep = false;
                        unsigned long long kv = 0ull;
                        if (p < e) {
                            const float4 o = sorted[p];
                            const float ddx = o.x - me.x, ddy = o.y - me.y, ddz = o.z - me.z;
                            const float d = (ddx * ddx + ddy * ddy) + ddz * ddz;
                            const int j = __float_as_int(o.w);
                            kv = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)(uint32_t)j;
                            keep = kv < bound && (include_self || j != i);
                        }
                        const unsigned long long bal = __ballot(keep);
                        if (bal == 0ull) continue;
                        if (keep) key[cnt + __popcll(bal & ((1ull << lane) - 1ull))] = kv;
                        cnt += __popcll(bal);
                        fresh = false;
                        if (cnt > CAP - 64) {      // the next chunk might not fit (cnt > 2 KP >= k here)
                            kk_wsync();
                            bound = kk_select(key, hist, cnt, k, lane);
                            cnt = k;
                            fresh = true;
                        }
                    }
                }
            }
        if (cnt >= k) {
            if (!fresh) {
                kk_wsync();
                bound = kk_select(key, hist, cnt, k, lane);
                cnt = k;
                fresh = true;
            }
            // every unvisited point lies at least r*h away along some axis, less the rounding of the cell assignment: a cell
            // coordinate below 2048 carries an absolute error below 1e-3 cells in fp32.  Ring 0 never proves anything (two
            // distinct points of different cells may still have d2 == 0 by underflow).
            const float lim = ((float)r - 0.01f) * h;
            if (r > 0 && __uint_as_float((uint32_t)(bound >> 32)) <= lim * lim) break;
        }
        if (x0 == 0 && y0 == 0 && z0 == 0 && x1 == dx_ - 1 && y1 == dy_ - 1 && z1 == dz_ - 1) break;   // every cell visited
    }
    // cnt <= k now (a buffer above k was selected at the end of its ring); pad and sort ascending
    kk_wsync();
    for (int t = cnt + lane; t < KP; t += 64) key[t] = ~0ull;
    for (int size = 2; size <= KP; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            kk_wsync();
            for (int t = lane; t < KP / 2; t += 64) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const unsigned long long a = key[lo], b = key[hi];
                if ((a > b) == up) { key[lo] = b; key[hi] = a; }
            }
        }
    kk_wsync();
    // S: the fp64 sum of the sorted row in a fixed order (lane-strided partials, then a butterfly)
    double S = 0.0;
    for (int t = lane; t < k; t += 64) {
        const unsigned long long v = key[t];
        const bool valid = t < cnt;
        const float d = __uint_as_float((uint32_t)(v >> 32));
        if (valid) S += (double)d;
        if (out_d2) out_d2[(size_t)i * k + t] = valid ? d : INFINITY;
        if (out_idx) out_idx[(size_t)i * k + t] = valid ? (int32_t)(uint32_t)v : -1;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) S += __shfl_xor(S, d, 64);
    if (lane == 0) {
        if (out_sigma) out_sigma[i] = cnt > 0 ? sqrtf((float)(S / (double)cnt)) : __uint_as_float(0x7fc00000u);
        if (out_count) out_count[i] = cnt;
    }
}

static inline int kk_max_cells(int N) {
    int m = N;
    if (m < 64) m = 64;
    if (m > (1 << 21)) m = 1 << 21;
    return m;
}

extern "C" size_t mgr_knn_self_workspace_bytes(int N, int k) {
    (void)k;
    const size_t mc = (size_t)kk_max_cells(N > 0 ? N : 1);
    return mgr_align(sizeof(KKParams)) + mgr_align(mc * 4) + mgr_align((mc + 1) * 4) + mgr_align(mc * 4) +
           mgr_align((size_t)(N > 0 ? N : 1) * 16);
}

// the launches of mgr_knn_self (arguments already checked)
static int kk_run(int N, const float* xyz, int k, int include_self, float* out_d2, int32_t* out_idx, float* out_sigma,
                  int32_t* out_count, void* workspace, hipStream_t stream) {
    const size_t mc = (size_t)kk_max_cells(N);
    char* ws = (char*)workspace;
    KKParams* P = (KKParams*)ws;
    size_t o = mgr_align(sizeof(KKParams));
    uint32_t* cnt = (uint32_t*)(ws + o);     o += mgr_align(mc * 4);
    uint32_t* start = (uint32_t*)(ws + o);   o += mgr_align((mc + 1) * 4);
    uint32_t* cursor = (uint32_t*)(ws + o);  o += mgr_align(mc * 4);
    float4* sorted = (float4*)(ws + o);
    MGR_HIP(hipMemsetAsync(cnt, 0, mc * 4, stream));
    const int blocks = (N + 255) / 256;
    const float per_cell = fmaxf(MGR_KNN_CELL_MIN_POINTS, (float)k / MGR_KNN_CELL_K_DIV);
    { MGR_PROF("k_kk_init", stream); hipLaunchKernelGGL(k_kk_init, dim3(1), dim3(1), 0, stream, P); }
    { MGR_PROF("k_kk_bbox", stream); hipLaunchKernelGGL(k_kk_bbox, dim3(blocks > 1024 ? 1024 : blocks), dim3(256), 0, stream, N, xyz, P); }
    { MGR_PROF("k_kk_setup", stream); hipLaunchKernelGGL(k_kk_setup, dim3(1), dim3(1), 0, stream, N, per_cell, (int)mc, P); }
    { MGR_PROF("k_kk_count", stream); hipLaunchKernelGGL(k_kk_count, dim3(blocks), dim3(256), 0, stream, N, xyz, P, cnt); }
    { MGR_PROF("k_kk_scan", stream); hipLaunchKernelGGL(k_kk_scan, dim3(1), dim3(1024), 0, stream, P, cnt, start, cursor); }
    { MGR_PROF("k_kk_scatter", stream); hipLaunchKernelGGL(k_kk_scatter, dim3(blocks), dim3(256), 0, stream, N, k, xyz, P, start, cursor, sorted, out_d2, out_idx, out_sigma, out_count); }
    {
        MGR_PROF("k_kk_query", stream);
        const dim3 grid((unsigned)((N + KK_WAVES - 1) / KK_WAVES)), block(64 * KK_WAVES);
        if (k <= 64) hipLaunchKernelGGL(k_kk_query<64>, grid, block, 0, stream, k, include_self, P, start, sorted, out_d2, out_idx, out_sigma, out_count);
        else if (k <= 128) hipLaunchKernelGGL(k_kk_query<128>, grid, block, 0, stream, k, include_self, P, start, sorted, out_d2, out_idx, out_sigma, out_count);
        else if (k <= 256) hipLaunchKernelGGL(k_kk_query<256>, grid, block, 0, stream, k, include_self, P, start, sorted, out_d2, out_idx, out_sigma, out_count);
        else hipLaunchKernelGGL(k_kk_query<512>, grid, block, 0, stream, k, include_self, P, start, sorted, out_d2, out_idx, out_sigma, out_count);
    }
    MGR_LAUNCH_CHECK("knn_self", stream, 0);
    return MGR_OK;
}

extern "C" int mgr_knn_self(int N, const float* xyz, int k, int include_self, float* out_d2, int32_t* out_idx,
                            float* out_sigma, int32_t* out_count, void* workspace, size_t workspace_bytes, void* stream_) {
    if (N < 0) return mgr_fail(MGR_EINVAL, "mgr_knn_self: bad sizes");
    if (k < 1 || k > MGR_KNN_MAX_K) return mgr_fail(MGR_EINVAL, "mgr_knn_self: k outside 1 .. MGR_KNN_MAX_K");
    if (N == 0) return MGR_OK;
    if (!xyz) return mgr_fail(MGR_EINVAL, "mgr_knn_self: null xyz");
    if (!workspace || workspace_bytes < mgr_knn_self_workspace_bytes(N, k))
        return mgr_fail(MGR_ENOMEM, "mgr_knn_self: workspace too small");
    return kk_run(N, xyz, k, include_self != 0, out_d2, out_idx, out_sigma, out_count, workspace, (hipStream_t)stream_);
}

// ---------------------------------------------------------------------------
// LoOP on the neighbourhoods (definition: include/manus_hip.h, mgr_outlier_scores)
// ---------------------------------------------------------------------------
// one wave per point: den = mean of the neighbours' sigma (fp64, the fixed order of the sorted row), plof = sigma / den - 1
__global__ __launch_bounds__(64 * KK_WAVES) void k_loop_plof(int N, int k, const int32_t* __restrict__ idx,
                                                            const int32_t* __restrict__ count,
                                                            const float* __restrict__ sigma, float* __restrict__ plof) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * KK_WAVES + (threadIdx.x >> 6);
    if (i >= N) return;
    const int n = count[i];
    double S = 0.0;
    for (int t = lane; t < n; t += 64) S += (double)sigma[idx[(size_t)i * k + t]];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) S += __shfl_xor(S, d, 64);
    if (lane == 0) {
        float v = __uint_as_float(0x7fc00000u);
        if (n > 0) {
            const float den = (float)(S / (double)n);
            v = den == 0.0f ? 0.0f : sigma[i] / den - 1.0f;
        }
        plof[i] = v;
    }
}

// per-workgroup fp64 partial of plof^2 over the valid points (+ their number), folded in a fixed order by k_loop_fold
__global__ __launch_bounds__(256) void k_loop_sq(int N, const int32_t* __restrict__ count, const float* __restrict__ plof,
                                                 double* __restrict__ part) {
    __shared__ double s_a[256], s_n[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double a = 0.0, n = 0.0;
    if (i < N && count[i] > 0) {
        const double p = (double)plof[i];
        a = p * p;
        n = 1.0;
    }
    s_a[threadIdx.x] = a;
    s_n[threadIdx.x] = n;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            s_a[threadIdx.x] += s_a[threadIdx.x + d];
            s_n[threadIdx.x] += s_n[threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[2 * (size_t)blockIdx.x] = s_a[0];
        part[2 * (size_t)blockIdx.x + 1] = s_n[0];
    }
}

// stats[0] = nplof, stats[1] = n_valid, stats[2] = 0 (k_loop_stats fills it); the flagged counter is cleared
__global__ __launch_bounds__(1024) void k_loop_fold(int nblk, const double* __restrict__ part, double* __restrict__ stats,
                                                   uint32_t* __restrict__ flagged) {
    __shared__ double s_a[1024], s_n[1024];
    const int tid = threadIdx.x;
    const int per = (nblk + 1023) / 1024;
    const int b = min(nblk, tid * per), e = min(nblk, b + per);
    double a = 0.0, n = 0.0;
    for (int j = b; j < e; ++j) {
        a += part[2 * (size_t)j];
        n += part[2 * (size_t)j + 1];
    }
    s_a[tid] = a;
    s_n[tid] = n;
    __syncthreads();
    for (int d = 512; d > 0; d >>= 1) {
        if (tid < d) {
            s_a[tid] += s_a[tid + d];
            s_n[tid] += s_n[tid + d];
        }
        __syncthreads();
    }
    if (tid == 0) {
        stats[0] = s_n[0] > 0.0 ? (double)MGR_LOOP_LAMBDA * sqrt(s_a[0] / s_n[0]) : 0.0;
        stats[1] = s_n[0];
        stats[2] = 0.0;
        *flagged = 0u;
    }
}

__global__ __launch_bounds__(256) void k_loop_score(int N, float prob, const float* __restrict__ plof,
                                                    const double* __restrict__ stats, float* __restrict__ score,
                                                    uint8_t* __restrict__ mask, float* __restrict__ out_plof,
                                                    uint32_t* __restrict__ flagged) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool flag = false;
    if (i < N) {
        const float p = plof[i], np = (float)stats[0];
        float s;
        if (p != p) s = p;
        else if (np == 0.0f) s = 0.0f;
        else s = fmaxf(0.0f, erff(p / (np * MGR_LOOP_SQRT2)));
        flag = s > prob;
        score[i] = s;
        if (mask) mask[i] = flag ? 1 : 0;
        if (out_plof) out_plof[i] = p;
    }
    const unsigned long long bal = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(flagged, (uint32_t)__popcll(bal));   // an integer count: order-free
}

__global__ void k_loop_stats(const uint32_t* __restrict__ flagged, double* __restrict__ stats, double* __restrict__ out_stats) {
    stats[2] = (double)*flagged;
    if (out_stats)
        for (int j = 0; j < 3; ++j) out_stats[j] = stats[j];
}

struct LoopLayout {
    size_t knn, idx, sigma, count, plof, part, stats, flagged, total;
};
static LoopLayout loop_layout(int N, int k) {
    LoopLayout L;
    const size_t n = (size_t)(N > 0 ? N : 1), kk = (size_t)(k > 0 ? k : 1);
    size_t o = 0;
    L.knn = o;     o += mgr_align(mgr_knn_self_workspace_bytes(N, k));
    L.idx = o;     o += mgr_align(n * kk * 4);
    L.sigma = o;   o += mgr_align(n * 4);
    L.count = o;   o += mgr_align(n * 4);
    L.plof = o;    o += mgr_align(n * 4);
    L.part = o;    o += mgr_align(((n + 255) / 256) * 16);
    L.stats = o;   o += mgr_align(3 * 8);
    L.flagged = o; o += mgr_align(4);
    L.total = o;
    return L;
}

extern "C" size_t mgr_outlier_scores_workspace_bytes(int N, int k) { return loop_layout(N, k).total; }

extern "C" int mgr_outlier_scores(int N, const float* xyz, int k, int include_self, float prob, float* out_score,
                                  uint8_t* out_mask, float* out_sigma, float* out_plof, double* out_stats,
                                  void* workspace, size_t workspace_bytes, void* stream_) {
    if (N < 0) return mgr_fail(MGR_EINVAL, "mgr_outlier_scores: bad sizes");
    if (k < 1 || k > MGR_KNN_MAX_K) return mgr_fail(MGR_EINVAL, "mgr_outlier_scores: k outside 1 .. MGR_KNN_MAX_K");
    if (N > 0 && (!xyz || !out_score)) return mgr_fail(MGR_EINVAL, "mgr_outlier_scores: null pointer");
    if (!workspace || workspace_bytes < mgr_outlier_scores_workspace_bytes(N, k))
        return mgr_fail(MGR_ENOMEM, "mgr_outlier_scores: workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    const LoopLayout L = loop_layout(N, k);
    char* ws = (char*)workspace;
    int32_t* idx = (int32_t*)(ws + L.idx);
    float* sigma = (float*)(ws + L.sigma);
    int32_t* count = (int32_t*)(ws + L.count);
    float* plof = (float*)(ws + L.plof);
    double* part = (double*)(ws + L.part);
    double* stats = (double*)(ws + L.stats);
    uint32_t* flagged = (uint32_t*)(ws + L.flagged);
    const int nblk = (N + 255) / 256;
    if (N > 0) {
        const int rc = kk_run(N, xyz, k, include_self != 0, nullptr, idx, sigma, count, ws + L.knn, stream);
        if (rc != MGR_OK) return rc;
        { MGR_PROF("k_loop_plof", stream); hipLaunchKernelGGL(k_loop_plof, dim3((unsigned)((N + KK_WAVES - 1) / KK_WAVES)), dim3(64 * KK_WAVES), 0, stream, N, k, idx, count, sigma, plof); }
        { MGR_PROF("k_loop_sq", stream); hipLaunchKernelGGL(k_loop_sq, dim3(nblk), dim3(256), 0, stream, N, count, plof, part); }
    }
    { MGR_PROF("k_loop_fold", stream); hipLaunchKernelGGL(k_loop_fold, dim3(1), dim3(1024), 0, stream, nblk, part, stats, flagged); }
    if (N > 0) {
        MGR_PROF("k_loop_score", stream);
        hipLaunchKernelGGL(k_loop_score, dim3(nblk), dim3(256), 0, stream, N, prob, plof, stats, out_score, out_mask, out_plof, flagged);
        if (out_sigma) MGR_HIP(hipMemcpyAsync(out_sigma, sigma, (size_t)N * 4, hipMemcpyDeviceToDevice, stream));
    }
    { MGR_PROF("k_loop_stats", stream); hipLaunchKernelGGL(k_loop_stats, dim3(1), dim3(1), 0, stream, flagged, stats, out_stats); }
    MGR_LAUNCH_CHECK("outlier_scores", stream, 0);
    return MGR_OK;
}
