// Feature render: composite caller channels, expected depth and accumulated opacity over the tile lists the last forward
// left in a workspace (mgr_raster_blend_features), and the gradients of a loss on those maps
// (mgr_raster_blend_features_backward).  The workspace is read and never written by either.
//
//   out[v, c, y, x] = sum_i w_i f[v, gid_i, c] + T_final bg[c],   w_i = alpha_i T_i
//   depth           = sum_i w_i z_i          (EXPECTED depth: not divided by the accumulated opacity, background 0)
//   alpha           = 1 - T_final
//
// The walk is the forward blend's (k_blend_fwd, raster_fwd.hip): one workgroup per 16x16 tile, one wave per 8x8 quadrant, lane =
// y * 8 + x, the list taken from the tile's queue record (tile_qrec: for a giant tile that is the regrouped, sorted list the
// forward blend read), 64 entries per batch, the batch culled against the box of the pixels that still accumulate (mgr_box_dead),
// the survivors staged pair-packed in LDS (mgr_pair_store) and evaluated by mgr_pair_alpha -- the arithmetic and the keep rule of
// the forward -- with its stop rule (an entry that would bring T below 1e-4 ends the pixel's walk and contributes nothing).  The
// set of (pixel, entry) contributions is therefore the forward's own; what differs is what is summed.
//
// Channels: a launch carries up to CG accumulators per lane (CG = 2, 4, 8); more channels are further launches, each walking the
// lists again.  Lane l of a wave fetches entry l of the batch -- its record, its CG feature values (a row is C floats at any
// 4-byte alignment: scalar loads), its depth -- and writes them to LDS; all 64 lanes then consume the staged entries.
//
// Backward (mgr_raster_blend_features_backward, second half of this file): gradients of a loss on those maps.  With g the upstream
// gradients of the maps at a pixel and s_i = f_i . g over the channels of a launch (the depth is the channel f = z, the alpha
// the channel f = 1, both on background 0),
//   dL/df_ic    = sum_pixels w_i g_c,      dL/dz_i = sum_pixels w_i g_depth,
//   dL/dalpha_i = T_i s_i - (suffix_i . g) / (1 - alpha_i),     suffix_i . g = (out . g) - (prefix through i) . g
// -- the colour backward's expression (k_blend_bwd, raster_bwd.hip) with the total taken from the forward's own output maps,
// walked FRONT TO BACK with the running prefix, the keep and stop rules of the walk above, the gradient passed through the
// 0.99 clamp as upstream.  k_blend_feat_bwd: one workgroup per tile, one wave per 8x8 quadrant, the walk of k_blend_feat; per
// contributing entry a wave reduces its 64 pixels' six geometry terms (v = G dL/dalpha: sum v dx, v dy, v dx^2, v dx dy, v dy^2,
// v) and the launch's channel terms (w g_c) with mgr_wave_reduce8, parks the totals in its LDS row of the entry, and after the
// batch (workgroup barrier) lane j of wave 0 adds the four quadrants' rows of entry j in quadrant order, applies the
// per-Gaussian factors of the colour backward's flush and writes ONE 64-byte record to the (tile, Gaussian) pair's private slot
// (slot base + by * rect width + bx of the grec) in the CALLER'S scratch, with the launch's tag.  The four waves leave the walk
// at different times, so the batch loop's trip count is made uniform by a workgroup vote: a finished wave still meets every
// barrier.  k_feat_gather: one thread per (view, Gaussian) sums its slots in slot order (tag == the launch's), writes the
// launch's dL/dfeatures columns, keeps the geometry sums in the scratch across the launches of a call (they add: the
// expression is linear in g) and, behind the last launch, applies project_backward and the depth's z row.  No atomics, fixed
// orders: bit-reproducible.  The workspace is only read; the tags of the scratch are CLEARED at the start of every call (a
// slot nobody wrote counts as zero because its tag is 0, the launches' tags are 1, 2, ...).
#include "instance_math.h"

#define FEAT_MAX_C 32
#define FEAT_GRID 4096

struct FeatArgs {
    int N, W, H, gx, gy, VT;
    uint32_t n_queue, n_busy, cap;   // positions of tile_qrec, non-empty tiles of tile_queue, pair capacity (list offsets are clamped to it)
    const uint32_t* tile_queue;
    const uint4* tile_qrec;
    const uint32_t* sorted_gid;
    const MgrGRec* grec;
    const float* depth;
    const float* feat;               // rows of C floats, view stride s_feat floats (0: shared by the views)
    long long s_feat;
    int C, c0, nc;                   // row length; this launch composites channels c0 .. c0 + nc - 1 ...
    int with_z;                      // ... and, in slot nc, the depth (output channel c0 + nc = the last one)
    const float* bg;                 // C floats or null (zeros)
    float* out;                      // (V, Cout, H, W)
    int Cout;
    float* out_alpha;                // (V, H, W) or null
};

template <int CG>
__global__ __launch_bounds__(256) void k_blend_feat(const FeatArgs a) {
    __shared__ __align__(16) float s_pair[4][32][MGR_PAIR_FLOATS];
    __shared__ __align__(16) float s_feat[4][64 + 1][CG];     // (+ 1: the zeroed partner of an odd batch's last entry)
    const int tid = threadIdx.x, lane = tid & 63;
    const int quad = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = a.N, W = a.W, H = a.H, gx = a.gx, T = a.gx * a.gy;
    const size_t P = (size_t)W * H;
    const int ns = a.nc + (a.with_z ? 1 : 0);                 // slots in use
    const unsigned long long lt = (1ull << lane) - 1ull;
    float* const slab = &s_pair[quad][0][0];
    float* const frow = &s_feat[quad][0][0];
    const uint32_t gid_max = (uint32_t)(N > 0 ? N - 1 : 0);
    // background of slot k (read where it is used: CG more scalars held across the walk cost the CG = 8 instantiation spills)
    auto bg_of = [&](int k) -> float { return (k < a.nc && a.bg) ? a.bg[a.c0 + k] : 0.0f; };

    // ---- tiles with a list, deepest first (the order of the forward's queue) ----
    for (uint32_t q = blockIdx.x; q < a.n_queue; q += gridDim.x) {
        const uint4 qrec = a.tile_qrec[q];
        const uint32_t vt = qrec.x;
        if (vt == MGR_HOLE || vt >= (uint32_t)a.VT) continue;
        const int v = (int)(vt / (uint32_t)T), t = (int)(vt % (uint32_t)T);
        const int bx = t % gx, by = t / gx;
        const uint32_t start = min(qrec.y, a.cap), nlist = min(qrec.z, a.cap - start);
        const int px = bx * 16 + (quad & 1) * 8 + (lane & 7);
        const int py = by * 16 + (quad >> 1) * 8 + (lane >> 3);
        const bool inside = px < W && py < H;
        const mgr_v2f fpx2 = {(float)px, (float)px}, fpy2 = {(float)py, (float)py};
        const float qx0 = (float)(bx * 16 + (quad & 1) * 8), qy0 = (float)(by * 16 + (quad >> 1) * 8);
        const MgrGRec* const gv = a.grec + (size_t)v * N;
        const float* const zv = a.depth + (size_t)v * N;
        const float* const fv = a.feat ? a.feat + (size_t)v * (size_t)a.s_feat + a.c0 : nullptr;
        const uint32_t* const sg = a.sorted_gid + start;
        const uint32_t lastidx = (nlist ? nlist : 1u) - 1u;

        float Tr = 1.0f, acc[CG];
#pragma unroll
        for (int k = 0; k < CG; ++k) acc[k] = 0.0f;
        bool done = !inside;
        // one batch of records ahead, two of indices (unconditional, clamped into the list)
        uint32_t gid = min(sg[min((uint32_t)lane, lastidx)], gid_max);
        uint32_t gid_n = sg[min(64u + lane, lastidx)];
        float4 ra = *(const float4*)(gv + gid), rb = *((const float4*)(gv + gid) + 1);
        for (uint32_t off = 0; off < nlist; off += 64) {
            int bx0, by0, bx1, by1;
            if (!mgr_quad_bbox(__builtin_amdgcn_ballot_w64(!done), bx0, by0, bx1, by1)) break;
            bool alive = false;
            if (off + lane < nlist)
                alive = !mgr_box_dead(ra.x, ra.y, ra.z, ra.w, rb.x, mgr_qmax(rb.y), qx0 + (float)bx0, qy0 + (float)by0,
                                      qx0 + (float)bx1, qy0 + (float)by1);
            const unsigned long long m = __ballot(alive);
            const int cnt = __popcll(m);
            __builtin_amdgcn_wave_barrier();      // (the reads of the batch before are done: one wave, LDS in order)
            if (alive) {
                const int rank = __popcll(m & lt);
                float f[CG];
#pragma unroll
                for (int k = 0; k < CG; ++k) f[k] = k < a.nc ? fv[(size_t)gid * a.C + k] : 0.0f;
                if (a.with_z) {
                    const float z = zv[gid];
#pragma unroll
                    for (int k = 0; k < CG; ++k) f[k] = k == a.nc ? z : f[k];
                }
                float* pb = slab + (rank >> 1) * MGR_PAIR_FLOATS;
                mgr_pair_store(pb, rank & 1, ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, 0.f, 0.f, 0.f, 0u);
                float* fr = frow + rank * CG;
#pragma unroll
                for (int k = 0; k < CG; ++k) fr[k] = f[k];
                if ((cnt & 1) && rank == cnt - 1) {   // the partner slot of an odd batch: opacity 0 -> never kept; zero features
                    mgr_pair_pad(pb);
#pragma unroll
                    for (int k = 0; k < CG; ++k) fr[CG + k] = 0.0f;
                }
            }
            {   // the next batch's records and the indices of the one after it: in flight during the blend below
                gid = min(gid_n, gid_max);
                ra = *(const float4*)(gv + gid);
                rb = *((const float4*)(gv + gid) + 1);
                gid_n = sg[min(off + 128u + lane, lastidx)];
            }
            __builtin_amdgcn_wave_barrier();
            const int npair = (cnt + 1) >> 1;
            for (int p = 0; p < npair; ++p) {
                const float4* pp = (const float4*)(slab + p * MGR_PAIR_FLOATS);
                const float4 R0 = pp[0], R1 = pp[1], R2 = pp[2];
                float fa[CG], fb[CG];
                const float* fp = frow + 2 * p * CG;
#pragma unroll
                for (int k = 0; k < CG; ++k) { fa[k] = fp[k]; fb[k] = fp[CG + k]; }
                mgr_v2f dx, dy, G, al;
                bool va, vb;
                mgr_pair_alpha(R0, R1, R2, fpx2, fpy2, dx, dy, G, al, va, vb);
                {   // entry a
                    const float al_a = (va && !done) ? al.x : 0.0f;
                    const float testT = Tr * (1.0f - al_a);
                    const bool stop = testT < 0.0001f;            // (al_a == 0 leaves testT = Tr >= 1e-4)
                    const float w = stop ? 0.0f : al_a * Tr;
#pragma unroll
                    for (int k = 0; k < CG; ++k) acc[k] += fa[k] * w;
                    Tr = stop ? Tr : testT;
                    done = done || stop;
                }
                {   // entry b
                    const float al_b = (vb && !done) ? al.y : 0.0f;
                    const float testT = Tr * (1.0f - al_b);
                    const bool stop = testT < 0.0001f;
                    const float w = stop ? 0.0f : al_b * Tr;
#pragma unroll
                    for (int k = 0; k < CG; ++k) acc[k] += fb[k] * w;
                    Tr = stop ? Tr : testT;
                    done = done || stop;
                }
                if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;
            }
        }
        if (inside) {
            const size_t pix = (size_t)py * W + px;
            if (ns > 0) {
                float* o = a.out + ((size_t)v * a.Cout + a.c0) * P + pix;
#pragma unroll
                for (int k = 0; k < CG; ++k)
                    if (k < ns) o[(size_t)k * P] = acc[k] + Tr * bg_of(k);
            }
            if (a.out_alpha) a.out_alpha[(size_t)v * P + pix] = 1.0f - Tr;
        }
    }
    // ---- empty tiles: background, alpha 0, depth 0 ----
    for (uint32_t q = a.n_busy + blockIdx.x; q < (uint32_t)a.VT; q += gridDim.x) {
        const uint32_t vt = a.tile_queue[q];
        if (vt >= (uint32_t)a.VT) continue;
        const int v = (int)(vt / (uint32_t)T), t = (int)(vt % (uint32_t)T);
        const int px = (t % gx) * 16 + (tid & 15), py = (t / gx) * 16 + (tid >> 4);
        if (px < W && py < H) {
            const size_t pix = (size_t)py * W + px;
            if (ns > 0) {
                float* o = a.out + ((size_t)v * a.Cout + a.c0) * P + pix;
#pragma unroll
                for (int k = 0; k < CG; ++k)
                    if (k < ns) o[(size_t)k * P] = bg_of(k);
            }
            if (a.out_alpha) a.out_alpha[(size_t)v * P + pix] = 0.0f;
        }
    }
}

// What the last forward left in a workspace: one blocking read of the header, then every refusal is the host's (nothing is
// launched).  `who` names the caller in the error text.
static int feat_read_state(const char* who, const char* ws, const MgrLayout& L, int V, int N, int W, int H, int64_t cap, int VT,
                           hipStream_t stream, MgrHeader& h) {
    const size_t head_bytes = offsetof(MgrHeader, qctr);
    MGR_HIP(hipMemcpyAsync(&h, ws + L.header, head_bytes, hipMemcpyDeviceToHost, stream));
    MGR_HIP(hipStreamSynchronize(stream));
    if (h.fwd_seq == 0u) return mgr_fail(MGR_ESTATE, "%s: no forward has run on this workspace", who);
    if (h.feat_seq != h.fwd_seq)
        return mgr_fail(MGR_ESTATE, "%s: the last forward on this workspace did not run its blend (MGR_FWD_NO_BLEND)", who);
    if (h.feat_dims[0] != (uint32_t)V || h.feat_dims[1] != (uint32_t)N || h.feat_dims[2] != (uint32_t)W ||
        h.feat_dims[3] != (uint32_t)H || h.feat_dims[4] != (uint32_t)cap)
        return mgr_fail(MGR_ESTATE, "%s: the last forward on this workspace was made for another V, N, W, H or pair capacity", who);
    if (h.feat_flags & MGR_FEAT_CUT)
        return mgr_fail(MGR_ESTATE, "%s: the last forward applied the depth cut (MGR_FWD_DEPTH_CUT): its lists are cut short", who);
    if (h.overflow != 0u)
        return mgr_fail(MGR_ESTATE, "%s: the last forward raised an overflow bit: its lists are incomplete", who);
    if (h.queue_len > (uint32_t)VT || h.queue_len_i > (uint32_t)VT)
        return mgr_fail(MGR_ESTATE, "%s: the header's queue lengths do not fit these sizes", who);
    return MGR_OK;
}

// Sequence number of the last forward binned on a workspace (MgrHeader::fwd_seq; 0: none yet), one blocking read: a caller that
// comes back to a forward's lists later (the feature backward under autograd) compares it with the number it noted.
extern "C" int mgr_raster_forward_seq_sync(const void* workspace, uint32_t* seq, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!workspace || !seq) return mgr_fail(MGR_EINVAL, "mgr_raster_forward_seq_sync: null pointer");
    MGR_HIP(hipMemcpyAsync(seq, (const char*)workspace + offsetof(MgrHeader, fwd_seq), 4, hipMemcpyDeviceToHost, stream));
    MGR_HIP(hipStreamSynchronize(stream));
    return MGR_OK;
}

extern "C" int mgr_raster_blend_features(int V, int N, int C, int W, int H, const float* features, int64_t stride_features,
                                         const float* bg_feat, int with_depth, float* out_feat, float* out_alpha,
                                         const void* workspace, size_t workspace_bytes, int64_t cap, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (V <= 0 || N < 0 || W <= 0 || H <= 0 || cap < 0 || cap > 0xFFFFFFF0ll)
        return mgr_fail(MGR_EINVAL, "mgr_raster_blend_features: bad sizes");
    if (C < 0 || C > FEAT_MAX_C) return mgr_fail(MGR_EINVAL, "mgr_raster_blend_features: C must be 0 .. 32");
    const int Cout = C + (with_depth ? 1 : 0);
    if (Cout == 0 && !out_alpha) return mgr_fail(MGR_EINVAL, "mgr_raster_blend_features: nothing to render (C = 0, no depth, no alpha)");
    if (!workspace || (Cout > 0 && !out_feat) || (C > 0 && N > 0 && !features))
        return mgr_fail(MGR_EINVAL, "mgr_raster_blend_features: null pointer");
    if (stride_features != 0 && stride_features < (int64_t)N * C)
        return mgr_fail(MGR_EINVAL, "mgr_raster_blend_features: view stride of the features smaller than N * C");
    const int gx = (W + 15) / 16, gy = (H + 15) / 16;
    if (gx > 65535 || gy > 65535) return mgr_fail(MGR_EINVAL, "mgr_raster_blend_features: image too large");
    const MgrLayout L = mgr_layout(V, N, W, H, cap);
    if (workspace_bytes < L.total) return mgr_fail(MGR_ENOMEM, "mgr_raster_blend_features: workspace too small for these sizes");
    const char* ws = (const char*)workspace;
    MgrHeader h;
    const int VT = V * gx * gy;
    {
        const int rc = feat_read_state("mgr_raster_blend_features", ws, L, V, N, W, H, cap, VT, stream, h);
        if (rc != MGR_OK) return rc;
    }

    FeatArgs a;
    a.N = N; a.W = W; a.H = H; a.gx = gx; a.gy = gy; a.VT = VT;
    a.n_queue = h.queue_len_i; a.n_busy = h.queue_len; a.cap = (uint32_t)cap;
    a.tile_queue = (const uint32_t*)(ws + L.tile_queue);
    a.tile_qrec = (const uint4*)(ws + L.tile_qrec);
    a.sorted_gid = (const uint32_t*)(ws + L.sorted_gid);
    a.grec = (const MgrGRec*)(ws + L.grec);
    a.depth = (const float*)(ws + L.depth);
    a.feat = features; a.s_feat = (long long)stride_features; a.C = C;
    a.bg = bg_feat; a.out = out_feat; a.Cout = Cout;
    // groups of 8, 4 or 2 slots; the first launch also writes alpha
    int c0 = 0;
    bool first = true;
    MGR_PROF("k_blend_feat", stream);
    do {
        const int rem = Cout - c0, g = rem > 4 ? 8 : (rem > 2 ? 4 : 2), n = rem < g ? rem : g;
        a.c0 = c0;
        a.with_z = (with_depth && c0 + n == Cout) ? 1 : 0;
        a.nc = n - a.with_z;
        a.out_alpha = first ? out_alpha : nullptr;
        if (g == 8) hipLaunchKernelGGL(k_blend_feat<8>, dim3(FEAT_GRID), dim3(256), 0, stream, a);
        else if (g == 4) hipLaunchKernelGGL(k_blend_feat<4>, dim3(FEAT_GRID), dim3(256), 0, stream, a);
        else hipLaunchKernelGGL(k_blend_feat<2>, dim3(FEAT_GRID), dim3(256), 0, stream, a);
        MGR_LAUNCH_CHECK("k_blend_feat", stream, 0);
        c0 += n;
        first = false;
    } while (c0 < Cout);
    return MGR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward
// ---------------------------------------------------------------------------------------------------------------------
#define FEAT_REC 16                   // floats per pair record of the scratch: [0..5] geometry, [6 ..] the launch's channel slots
#define FEAT_GEO 8                    // floats per (view, Gaussian) kept across the launches: geometry, dL/dz, records seen

struct FeatScratch {
    size_t tag, rec, geo, total;
};
static inline FeatScratch feat_scratch_layout(int V, int N, int64_t cap) {
    FeatScratch S;
    const size_t c = (size_t)(cap > 0 ? cap : 1), VN = (size_t)V * (size_t)(N > 0 ? N : 1);
    size_t o = 0;
    S.tag = o; o += mgr_align(c * 4);
    S.rec = o; o += mgr_align(c * FEAT_REC * 4);
    S.geo = o; o += mgr_align(VN * FEAT_GEO * 4);
    S.total = o;
    return S;
}

extern "C" size_t mgr_raster_feat_backward_workspace_bytes(int V, int N, int C, int W, int H, int64_t cap) {
    (void)C; (void)W; (void)H;        // (a record carries one launch's channels, whatever C; nothing is kept per pixel)
    if (V <= 0 || N < 0 || cap < 0) return 0;
    return feat_scratch_layout(V, N, cap).total;
}

struct FeatBwdArgs {
    int N, W, H, gx, gy, VT;
    uint32_t n_queue, cap;
    const uint4* tile_qrec;
    const uint32_t* sorted_gid;
    const MgrGRec* grec;
    const float* depth;
    const float* feat;
    long long s_feat;
    int C, c0, nc, with_z;           // as FeatArgs
    const float* out;                // (V, Cout, H, W): what the forward call produced
    const float* g_out;              // its upstream gradient
    int Cout;
    const float* out_alpha;          // (V, H, W) and its upstream gradient: the launch that carries the alpha, null otherwise
    const float* g_alpha;
    float* rec;                      // scratch: FEAT_REC floats per pair slot
    uint32_t* tag;
    uint32_t tagval;
};

// The 64 pixels' terms of one entry -> the wave's LDS row of the entry: [Sx, Sy, Sxx, Sxy, Syy, sum v, sum w g_0, ...].
// mgr_wave_reduce8 leaves the total of x[MGR_R8_SLOT(lane >> 3)] in the 8 lanes of group lane >> 3: a fixed tree.
template <int CG>
__device__ __forceinline__ void feat_bwd_reduce(float v, float w, float dx, float dy, const float gk[CG], float* arow, int lane) {
    const float vx = v * dx, vy = v * dy;
    const int k = MGR_R8_SLOT(lane >> 3);
    const float t0 = mgr_wave_reduce8(vx, vy, vx * dx, vx * dy, vy * dy, v, w * gk[0], w * gk[1], lane);
    if ((lane & 7) == 0) arow[k] = t0;
    if (CG > 2) {
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = j + 2 < CG ? w * gk[j + 2 < CG ? j + 2 : 0] : 0.0f;
        const float t1 = mgr_wave_reduce8(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], lane);
        if ((lane & 7) == 0) arow[8 + k] = t1;
    }
}

template <int CG>
__global__ __launch_bounds__(256) void k_blend_feat_bwd(const FeatBwdArgs a) {
    constexpr int NV = CG == 2 ? 8 : 16;                      // floats of a record in use
    __shared__ __align__(16) float s_pair[4][32][MGR_PAIR_FLOATS];
    __shared__ __align__(16) float s_feat[4][64 + 1][CG];
    __shared__ float s_acc[4][64][NV + 1];                    // (+ 1: rows of an odd stride)
    __shared__ uint32_t s_flag[4][64];                        // entry j of the batch has a row in quadrant q
    __shared__ uint32_t s_alive[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int quad = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = a.N, W = a.W, H = a.H, gx = a.gx, T = a.gx * a.gy;
    const size_t P = (size_t)W * H;
    const int ns = a.nc + (a.with_z ? 1 : 0);
    const unsigned long long lt = (1ull << lane) - 1ull;
    float* const slab = &s_pair[quad][0][0];
    float* const frow = &s_feat[quad][0][0];
    const uint32_t gid_max = (uint32_t)(N > 0 ? N - 1 : 0);

    for (uint32_t q = blockIdx.x; q < a.n_queue; q += gridDim.x) {
        const uint4 qrec = a.tile_qrec[q];
        const uint32_t vt = qrec.x;
        if (vt == MGR_HOLE || vt >= (uint32_t)a.VT) continue;             // (uniform over the workgroup)
        const int v = (int)(vt / (uint32_t)T), t = (int)(vt % (uint32_t)T);
        const int bx = t % gx, by = t / gx;
        const uint32_t start = min(qrec.y, a.cap), nlist = min(qrec.z, a.cap - start);
        const int px = bx * 16 + (quad & 1) * 8 + (lane & 7);
        const int py = by * 16 + (quad >> 1) * 8 + (lane >> 3);
        const bool inside = px < W && py < H;
        const mgr_v2f fpx2 = {(float)px, (float)px}, fpy2 = {(float)py, (float)py};
        const float qx0 = (float)(bx * 16 + (quad & 1) * 8), qy0 = (float)(by * 16 + (quad >> 1) * 8);
        const MgrGRec* const gv = a.grec + (size_t)v * N;
        const float* const zv = a.depth + (size_t)v * N;
        const float* const fv = a.feat ? a.feat + (size_t)v * (size_t)a.s_feat + a.c0 : nullptr;
        const uint32_t* const sg = a.sorted_gid + start;
        const uint32_t lastidx = (nlist ? nlist : 1u) - 1u;

        // the pixel's upstream gradients and (forward output) . g = everything the walk will sum, background included
        float gk[CG], ga = 0.0f, Og = 0.0f;
#pragma unroll
        for (int k = 0; k < CG; ++k) gk[k] = 0.0f;
        if (inside) {
            const size_t pix = (size_t)py * W + px;
            if (ns > 0) {
                const size_t o = ((size_t)v * a.Cout + a.c0) * P + pix;
#pragma unroll
                for (int k = 0; k < CG; ++k)
                    if (k < ns) {
                        gk[k] = a.g_out[o + (size_t)k * P];
                        Og += a.out[o + (size_t)k * P] * gk[k];
                    }
            }
            if (a.g_alpha) {
                ga = a.g_alpha[(size_t)v * P + pix];
                Og += a.out_alpha[(size_t)v * P + pix] * ga;
            }
        }
        float Tr = 1.0f, pg = 0.0f;       // transmittance in front of the next entry, (prefix through the last one) . g
        bool done = !inside;

        for (uint32_t off = 0; off < nlist; off += 64) {
            // the vote: the batch is walked while any of the four quadrants has a pixel that still accumulates
            const unsigned long long live = __builtin_amdgcn_ballot_w64(!done);
            if (lane == 0) s_alive[quad] = live != 0ull ? 1u : 0u;
            __syncthreads();
            if ((s_alive[0] | s_alive[1] | s_alive[2] | s_alive[3]) == 0u) break;
            // lane l: entry l of the batch (every wave: wave 0 writes the records from these)
            const uint32_t gid = min(sg[min(off + (uint32_t)lane, lastidx)], gid_max);
            const float4 ra = *(const float4*)(gv + gid), rb = *((const float4*)(gv + gid) + 1), rcz = *((const float4*)(gv + gid) + 2);
            s_flag[quad][lane] = 0u;
            int bx0, by0, bx1, by1;
            if (mgr_quad_bbox(live, bx0, by0, bx1, by1)) {
                bool alive = false;
                if (off + lane < nlist)
                    alive = !mgr_box_dead(ra.x, ra.y, ra.z, ra.w, rb.x, mgr_qmax(rb.y), qx0 + (float)bx0, qy0 + (float)by0,
                                          qx0 + (float)bx1, qy0 + (float)by1);
                const unsigned long long m = __ballot(alive);
                const int cnt = __popcll(m);
                __builtin_amdgcn_wave_barrier();
                if (alive) {
                    const int rank = __popcll(m & lt);
                    float f[CG];
#pragma unroll
                    for (int k = 0; k < CG; ++k) f[k] = k < a.nc ? fv[(size_t)gid * a.C + k] : 0.0f;
                    if (a.with_z) {
                        const float z = zv[gid];
#pragma unroll
                        for (int k = 0; k < CG; ++k) f[k] = k == a.nc ? z : f[k];
                    }
                    float* pb = slab + (rank >> 1) * MGR_PAIR_FLOATS;
                    mgr_pair_store(pb, rank & 1, ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, 0.f, 0.f, 0.f, (uint32_t)lane);   // pos = place in the batch
                    float* fr = frow + rank * CG;
#pragma unroll
                    for (int k = 0; k < CG; ++k) fr[k] = f[k];
                    if ((cnt & 1) && rank == cnt - 1) {
                        mgr_pair_pad(pb);
#pragma unroll
                        for (int k = 0; k < CG; ++k) fr[CG + k] = 0.0f;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                const int npair = (cnt + 1) >> 1;
                for (int p = 0; p < npair; ++p) {
                    const float4* pp = (const float4*)(slab + p * MGR_PAIR_FLOATS);
                    const float4 R0 = pp[0], R1 = pp[1], R2 = pp[2], R4 = pp[4];
                    float fa[CG], fb[CG];
                    const float* fp = frow + 2 * p * CG;
#pragma unroll
                    for (int k = 0; k < CG; ++k) { fa[k] = fp[k]; fb[k] = fp[CG + k]; }
                    mgr_v2f dx, dy, G, al;
                    bool va, vb;
                    mgr_pair_alpha(R0, R1, R2, fpx2, fpy2, dx, dy, G, al, va, vb);
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const float al_e = ((e ? vb : va) && !done) ? (e ? al.y : al.x) : 0.0f;
                        const float oma = 1.0f - al_e;
                        const float testT = Tr * oma;
                        const bool stop = testT < 0.0001f;
                        const bool valid = al_e > 0.0f && !stop;             // the forward's contribution set
                        if (__builtin_amdgcn_ballot_w64(valid) != 0ull) {    // (wave-uniform)
                            const float* f = e ? fb : fa;
                            float s = ga;
#pragma unroll
                            for (int k = 0; k < CG; ++k) s += f[k] * gk[k];
                            const float w = valid ? al_e * Tr : 0.0f;
                            pg += w * s;
                            const float da = valid ? Tr * s - (Og - pg) * __builtin_amdgcn_rcpf(oma) : 0.0f;
                            const uint32_t j = __float_as_uint(e ? R4.w : R4.z) & 63u;
                            feat_bwd_reduce<CG>((e ? G.y : G.x) * da, w, e ? dx.y : dx.x, e ? dy.y : dy.x, gk, &s_acc[quad][j][0], lane);
                            if (lane == 0) s_flag[quad][j] = 1u;
                        }
                        Tr = stop ? Tr : testT;
                        done = done || stop;
                    }
                    if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;
                }
            }
            __syncthreads();
            // lane j of wave 0: the record of entry j, the quadrants' rows added in quadrant order
            if (tid < 64 && off + (uint32_t)tid < nlist) {
                const uint32_t f0 = s_flag[0][tid], f1 = s_flag[1][tid], f2 = s_flag[2][tid], f3 = s_flag[3][tid];
                const int32_t slot = __float_as_int(rcz.y) + by * __float_as_int(rcz.z) + bx;
                if ((f0 | f1 | f2 | f3) != 0u && slot >= 0 && (uint32_t)slot < a.cap) {
                    float r[NV];
#pragma unroll
                    for (int k = 0; k < NV; ++k) {
                        float x = 0.0f;
                        if (f0) x += s_acc[0][tid][k];
                        if (f1) x += s_acc[1][tid][k];
                        if (f2) x += s_acc[2][tid][k];
                        if (f3) x += s_acc[3][tid][k];
                        r[k] = x;
                    }
                    // the per-Gaussian factors of the colour backward's flush (k_blend_bwd): q = opacity v,
                    // dL/dmean2D = -W/2 (A Sx + B Sy), -H/2 (C Sy + B Sx), dL/dconic = -1/2 (Sxx, Sxy, Syy), dL/dopacity = sum v
#pragma unroll
                    for (int c = 0; c < 5; ++c) r[c] *= rb.y;
                    const float cA = ra.z, cB = ra.w, cC = rb.x;
                    const float mx = (-0.5f * (float)W) * (cA * r[0] + cB * r[1]);
                    const float my = (-0.5f * (float)H) * (cC * r[1] + cB * r[0]);
                    float4* o = (float4*)(a.rec + (size_t)slot * FEAT_REC);
                    o[0] = make_float4(mx, my, -0.5f * r[2], -0.5f * r[3]);
                    o[1] = make_float4(-0.5f * r[4], r[5], r[6], r[7]);
                    if (NV > 8) {
                        o[2] = make_float4(r[8 % NV], r[9 % NV], r[10 % NV], r[11 % NV]);
                        o[3] = make_float4(r[12 % NV], r[13 % NV], r[14 % NV], r[15 % NV]);
                    }
                    a.tag[slot] = a.tagval;
                }
            }
            __syncthreads();
        }
        __syncthreads();      // (a wave that left on the vote must not post the next tile's vote before the others have read this one)
    }
}

// One thread per (view, Gaussian): the records of its slots, in slot order.  `first`: the geometry sums start here, otherwise they
// add to what the launches before left in geo; `last`: the chain to the caller's outputs.
__global__ __launch_bounds__(256) void k_feat_gather(int N, int W, int H, const float* __restrict__ cams,
                                                     const float* __restrict__ means3D, int64_t s_means,
                                                     const float* __restrict__ cov3D, int64_t s_cov,
                                                     const ushort4* __restrict__ rect, const uint32_t* __restrict__ pair_off,
                                                     const uint32_t* __restrict__ tag, const float* __restrict__ rec, uint32_t cap,
                                                     uint32_t tagval, int C, int c0, int nc, int with_z, int wide, int first, int last,
                                                     float* __restrict__ geo, float* __restrict__ dL_dmeans3D,
                                                     float* __restrict__ dL_dmeans2D, float* __restrict__ dL_dopacity,
                                                     float* __restrict__ dL_dcov3D, float* __restrict__ dL_dfeatures) {
    const int v = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const size_t vi = (size_t)v * N + i;
    const ushort4 rc = rect[vi];
    uint32_t cnt = (uint32_t)((rc.z - rc.x) * (rc.w - rc.y));
    const uint32_t off = pair_off[vi];
    float g[FEAT_GEO], f[8];
#pragma unroll
    for (int k = 0; k < FEAT_GEO; ++k) g[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = 0.0f;
    if (cnt > 0 && off < cap) {
        cnt = min(cnt, cap - off);
        for (uint32_t s = 0; s < cnt; ++s) {
            if (tag[off + s] != tagval) continue;
            const float4* r = (const float4*)(rec + (size_t)(off + s) * FEAT_REC);
            const float4 r0 = r[0], r1 = r[1];
            g[0] += r0.x; g[1] += r0.y; g[2] += r0.z; g[3] += r0.w; g[4] += r1.x; g[5] += r1.y;
            f[0] += r1.z; f[1] += r1.w;
            if (wide) {
                const float4 r2 = r[2], r3 = r[3];
                f[2] += r2.x; f[3] += r2.y; f[4] += r2.z; f[5] += r2.w;
                f[6] += r3.x; f[7] += r3.y;
            }
            g[7] += 1.0f;
        }
    }
    if (dL_dfeatures) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < nc) dL_dfeatures[vi * (size_t)C + c0 + k] = f[k];
    }
    if (with_z) {
#pragma unroll
        for (int k = 0; k < 8; ++k) g[6] += k == nc ? f[k] : 0.0f;
    }
    float* gp = geo + vi * FEAT_GEO;
    if (!first) {
#pragma unroll
        for (int k = 0; k < FEAT_GEO; ++k) g[k] += gp[k];
    }
    if (!last) {
#pragma unroll
        for (int k = 0; k < FEAT_GEO; ++k) gp[k] = g[k];
        return;
    }
    float dm[3] = {0.f, 0.f, 0.f}, dc6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (g[7] > 0.0f) {                 // some launch of the call wrote a record for this (view, Gaussian)
        MgrCam cam;
        mgr_load_cam(cams, v, cam);
        const float* mp = means3D + (size_t)v * s_means + (size_t)i * 3;
        const float p[3] = {mp[0], mp[1], mp[2]};
        const float* cp = cov3D + (size_t)v * s_cov + (size_t)i * 6;
        const float c6[6] = {cp[0], cp[1], cp[2], cp[3], cp[4], cp[5]};
        const float acc[9] = {g[0], g[1], g[2], g[3], g[4], g[5], 0.f, 0.f, 0.f};
        project_backward(cam, W, H, p, c6, acc, dm, dc6);
        // z = view row 2 . (p, 1) (project_gaussian): the expected depth's own path to the mean
        dm[0] += cam.view[2] * g[6]; dm[1] += cam.view[6] * g[6]; dm[2] += cam.view[10] * g[6];
    }
    float* o3 = dL_dmeans3D + vi * 3;
    o3[0] = dm[0]; o3[1] = dm[1]; o3[2] = dm[2];
    float* o2 = dL_dmeans2D + vi * 3;
    o2[0] = g[0]; o2[1] = g[1]; o2[2] = 0.f;
    dL_dopacity[vi] = g[5];
    float* ov = dL_dcov3D + vi * 6;
#pragma unroll
    for (int j = 0; j < 6; ++j) ov[j] = dc6[j];
}

extern "C" int mgr_raster_blend_features_backward(int V, int N, int C, int W, int H, const float* cams, const float* means3D,
                                                  int64_t s_means, const float* cov3D, int64_t s_cov, const float* features,
                                                  int64_t stride_features, const float* bg_feat, int with_depth,
                                                  const float* out_feat, const float* out_alpha, const float* dL_dout_feat,
                                                  const float* dL_dalpha, float* dL_dmeans3D, float* dL_dmeans2D,
                                                  float* dL_dopacity, float* dL_dcov3D, float* dL_dfeatures, const void* workspace,
                                                  size_t workspace_bytes, int64_t cap, void* scratch, size_t scratch_bytes, int flags,
                                                  void* stream_) {
    static const char* const who = "mgr_raster_blend_features_backward";
    (void)bg_feat;                    // (the background's share of a pixel is in out_feat already)
    hipStream_t stream = (hipStream_t)stream_;
    if (V <= 0 || N < 0 || W <= 0 || H <= 0 || cap < 0 || cap > 0xFFFFFFF0ll) return mgr_fail(MGR_EINVAL, "%s: bad sizes", who);
    if (C < 0 || C > FEAT_MAX_C) return mgr_fail(MGR_EINVAL, "%s: C must be 0 .. 32", who);
    if (!dL_dout_feat && !dL_dalpha) return mgr_fail(MGR_EINVAL, "%s: no upstream gradient (dL_dout_feat and dL_dalpha are both NULL)", who);
    const int Cout = C + (with_depth ? 1 : 0);
    if (dL_dout_feat && Cout == 0) return mgr_fail(MGR_EINVAL, "%s: dL_dout_feat given for C = 0 without depth", who);
    if (!workspace || !scratch || !cams || (dL_dout_feat && !out_feat) || (dL_dalpha && !out_alpha))
        return mgr_fail(MGR_EINVAL, "%s: null pointer", who);
    if (N > 0 && (!means3D || !cov3D || !dL_dmeans3D || !dL_dmeans2D || !dL_dopacity || !dL_dcov3D || (C > 0 && (!features || !dL_dfeatures))))
        return mgr_fail(MGR_EINVAL, "%s: null pointer", who);
    if (stride_features != 0 && stride_features < (int64_t)N * C)
        return mgr_fail(MGR_EINVAL, "%s: view stride of the features smaller than N * C", who);
    const int gx = (W + 15) / 16, gy = (H + 15) / 16;
    if (gx > 65535 || gy > 65535 || V > 65535) return mgr_fail(MGR_EINVAL, "%s: image too large or too many views", who);
    const MgrLayout L = mgr_layout(V, N, W, H, cap);
    if (workspace_bytes < L.total) return mgr_fail(MGR_ENOMEM, "%s: workspace too small for these sizes", who);
    const FeatScratch S = feat_scratch_layout(V, N, cap);
    if (scratch_bytes < S.total) return mgr_fail(MGR_ENOMEM, "%s: scratch smaller than mgr_raster_feat_backward_workspace_bytes", who);
    const char* ws = (const char*)workspace;
    MgrHeader h;
    const int VT = V * gx * gy;
    {
        const int rc = feat_read_state(who, ws, L, V, N, W, H, cap, VT, stream, h);
        if (rc != MGR_OK) return rc;
    }
    if (N == 0) return MGR_OK;
    char* sc = (char*)scratch;
    // a slot nobody writes must count as zero: the tags are cleared once per call, the launches tag with 1, 2, ...
    MGR_HIP(hipMemsetAsync(sc + S.tag, 0, (size_t)(cap > 0 ? cap : 1) * 4, stream));
    const int Cw = dL_dout_feat ? Cout : 0;          // channels that carry a gradient (none: one launch for the alpha alone)
    if (C > 0 && !dL_dout_feat) MGR_HIP(hipMemsetAsync(dL_dfeatures, 0, (size_t)V * N * C * sizeof(float), stream));

    FeatBwdArgs a;
    a.N = N; a.W = W; a.H = H; a.gx = gx; a.gy = gy; a.VT = VT;
    a.n_queue = h.queue_len_i; a.cap = (uint32_t)cap;
    a.tile_qrec = (const uint4*)(ws + L.tile_qrec);
    a.sorted_gid = (const uint32_t*)(ws + L.sorted_gid);
    a.grec = (const MgrGRec*)(ws + L.grec);
    a.depth = (const float*)(ws + L.depth);
    a.feat = features; a.s_feat = (long long)stride_features; a.C = C;
    a.out = out_feat; a.g_out = dL_dout_feat; a.Cout = Cout;
    a.rec = (float*)(sc + S.rec); a.tag = (uint32_t*)(sc + S.tag);
    int c0 = 0;
    uint32_t launch = 0;
    do {   // the forward's groups: 8, 4 or 2 slots, the depth in the last group's last slot, the alpha with the first group
        const int rem = Cw - c0, g = rem > 4 ? 8 : (rem > 2 ? 4 : 2), n = rem < g ? rem : g;
        a.c0 = c0;
        a.with_z = (with_depth && Cw > 0 && c0 + n == Cw) ? 1 : 0;
        a.nc = n - a.with_z;
        a.out_alpha = launch == 0 && dL_dalpha ? out_alpha : nullptr;
        a.g_alpha = launch == 0 ? dL_dalpha : nullptr;
        a.tagval = ++launch;
        {
            MGR_PROF("k_blend_feat_bwd", stream);
            if (g == 8) hipLaunchKernelGGL(k_blend_feat_bwd<8>, dim3(FEAT_GRID), dim3(256), 0, stream, a);
            else if (g == 4) hipLaunchKernelGGL(k_blend_feat_bwd<4>, dim3(FEAT_GRID), dim3(256), 0, stream, a);
            else hipLaunchKernelGGL(k_blend_feat_bwd<2>, dim3(FEAT_GRID), dim3(256), 0, stream, a);
        }
        MGR_LAUNCH_CHECK("k_blend_feat_bwd", stream, flags & MGR_BWD_CHECK);
        c0 += n;
        {
            MGR_PROF("k_feat_gather", stream);
            hipLaunchKernelGGL(k_feat_gather, dim3((N + 255) / 256, V), dim3(256), 0, stream, N, W, H, cams, means3D, s_means, cov3D, s_cov,
                               (const ushort4*)(ws + L.rect), (const uint32_t*)(ws + L.pair_off), (const uint32_t*)a.tag,
                               (const float*)a.rec, (uint32_t)cap, a.tagval, C, a.c0, a.nc, a.with_z, g > 2 ? 1 : 0, launch == 1 ? 1 : 0,
                               c0 >= Cw ? 1 : 0, (float*)(sc + S.geo), dL_dmeans3D, dL_dmeans2D, dL_dopacity, dL_dcov3D,
                               C > 0 && dL_dout_feat ? dL_dfeatures : (float*)nullptr);
        }
        MGR_LAUNCH_CHECK("k_feat_gather", stream, flags & MGR_BWD_CHECK);
    } while (c0 < Cw);
    return MGR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Map backward of the fused route (mgr_views_maps_backward): gradients of a loss on the alpha and depth maps, rendered over the
// lists of a mgr_views_forward, to the CANONICAL leaves.  The fused forward never writes posed means or covariances to memory,
// which k_feat_gather reads; here the walk is the same k_blend_feat_bwd<2> (C = 0: the depth in slot 0, the alpha beside it,
// ONE launch, tag 1) and the gather is k_views_feat_gather, laid out like k_inst_bwd without run lists (raster_bwd.hip):
//   * lane = Gaussian_local * G + view_local, G = 1 / 2 / 4 / 8 views of a group in adjacent lanes, cameras and bone transforms of
//     the group's views in LDS (one padded slab per view);
//   * every lane sums the records of its (view, Gaussian) in slot order, recomputes the posed mean and covariance from the
//     canonical parameters with the forward's own functions (blend_tf, lbs_apply: the rounding of the forward's records), and
//     runs project_backward, the depth's z row of the view matrix, lbs_backward_view and the bone-weight products in registers;
//   * the views are summed over the group with DPP (grp_sum: a fixed tree, ascending lanes), lane 0 of the group applies the
//     quaternion backward and the sigmoid and writes the Gaussian's rows.  V > 8: groups of eight, in group order, the later ones
//     adding.  No atomics: bit-reproducible.
// EVERY Gaussian has a lane group (no active list: nothing of the workspace is written).  accumulate = 0: every row is written,
// zeros where no view holds a record; accumulate = 1: rows with a record are added to, all others are not touched.
// ---------------------------------------------------------------------------------------------------------------------
#define VM_THREADS 256
#define VM_TSTRIDE(B) ((B) * 16 + 4)      // LDS words per view of bone transforms (+4: the slabs of a group fall in distinct banks)

template <int G>
__global__ __launch_bounds__(VM_THREADS) void k_views_feat_gather(
    int v_first, int v_count, int N, int B, int n_art, int W, int H, const float* __restrict__ cams,
    const float* __restrict__ xyz, const float* __restrict__ log_scale, const float* __restrict__ rot,
    const float* __restrict__ op_logit, const float* __restrict__ skin_w, const float* __restrict__ transforms,
    const ushort4* __restrict__ rect, const uint32_t* __restrict__ pair_off, const uint32_t* __restrict__ tag,
    const float* __restrict__ rec, uint32_t cap, int with_z, int accumulate, float* __restrict__ d_xyz, float* __restrict__ d_ls,
    float* __restrict__ d_rot, float* __restrict__ d_op, float* __restrict__ d_w) {
    constexpr int IPB = VM_THREADS / G;
    extern __shared__ __align__(16) float s_vm[];        // G x (camera 40 | transforms VM_TSTRIDE(B))
    const int tid = threadIdx.x, vl = tid & (G - 1), il = tid / G;
    const int i_raw = blockIdx.x * IPB + il;
    const int i = min(i_raw, N - 1);
    const bool ok = i_raw < N;                           // (all lanes stay for the DPP sums)
    const bool any_tf = skin_w != nullptr;               // workgroup-uniform: the pose slabs are staged
    const bool has_tf = any_tf && i < n_art;             // uniform over the lane group
    const int tstride = VM_TSTRIDE(B), vstride = MGR_CAM_FLOATS + (any_tf ? tstride : 0);
    for (int k = tid; k < G * MGR_CAM_FLOATS; k += VM_THREADS) {
        const int g = k / MGR_CAM_FLOATS, e = k % MGR_CAM_FLOATS;
        s_vm[g * vstride + e] = g < v_count ? cams[(size_t)(v_first + g) * MGR_CAM_FLOATS + e] : 0.f;
    }
    if (any_tf)
        for (int k = tid; k < G * B * 16; k += VM_THREADS) {
            const int g = k / (B * 16), e = k % (B * 16);
            s_vm[g * vstride + MGR_CAM_FLOATS + e] = g < v_count ? transforms[(size_t)(v_first + g) * B * 16 + e] : 0.f;
        }
    __syncthreads();
    const float* const Tp = s_vm + vl * vstride + MGR_CAM_FLOATS;

    // the records of this (view, Gaussian), in slot order: [mean2D.x, .y, conic A, B, C, opacity] and dL/dz
    // TWIN: k_views_feat_gather_pose below repeats this record walk, the camera unpack and the chain down to dtf by copy (the
    // reason is at its head).  A change here to the record layout, the tag value, the slot clamp or the depth path goes there too;
    // what would notice a drift is tests/test_gpu_map_pose.py's comparison of d_transforms with the operator route.
    float acc[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float gz = 0.f;
    bool any = false;
    if (ok && vl < v_count) {
        const size_t vi = (size_t)(v_first + vl) * N + i;
        const ushort4 rc = rect[vi];
        uint32_t cnt = (uint32_t)((rc.z - rc.x) * (rc.w - rc.y));
        const uint32_t off = pair_off[vi];
        if (cnt > 0 && off < cap) {
            cnt = min(cnt, cap - off);
            for (uint32_t s = 0; s < cnt; ++s) {
                if (tag[off + s] != 1u) continue;
                const float4* r = (const float4*)(rec + (size_t)(off + s) * FEAT_REC);
                const float4 r0 = r[0], r1 = r[1];
                acc[0] += r0.x; acc[1] += r0.y; acc[2] += r0.z; acc[3] += r0.w; acc[4] += r1.x; acc[5] += r1.y;
                gz += r1.z;
                any = true;
            }
        }
    }
    if (!with_z) gz = 0.f;
    const bool grp_any = grp_sum<G>(any ? 1.0f : 0.0f) > 0.0f;

    GaussCano g;
    cano_load(xyz, log_scale, rot, i, g);
    float dxyz[3] = {0.f, 0.f, 0.f}, ds[3] = {0.f, 0.f, 0.f};
    float dR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float dw[MGR_MAX_BONES];
#pragma unroll
    for (int b = 0; b < MGR_MAX_BONES; ++b) dw[b] = 0.f;
    float dop = 0.f;
    if (any) {
        MgrCam cam;
        {
            const float* p = s_vm + vl * vstride;
            cam.tanfovx = p[0];
            cam.tanfovy = p[1];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                cam.view[k] = p[2 + k];
                cam.proj[k] = p[18 + k];
            }
            cam.campos[0] = p[34]; cam.campos[1] = p[35]; cam.campos[2] = p[36];
        }
        float tf[12], p3[3], c6[6], dm[3], dc6[6], dtf[12];
        blend_tf(has_tf ? skin_w + (size_t)i * B : nullptr, Tp, B, tf);
        lbs_apply(tf, g, p3, c6);
        project_backward(cam, W, H, p3, c6, acc, dm, dc6);
        // z = view row 2 . (p, 1) (project_gaussian): the expected depth's own path to the posed mean
        dm[0] += cam.view[2] * gz; dm[1] += cam.view[6] * gz; dm[2] += cam.view[10] * gz;
        lbs_backward_view<false>(tf, g, dm, dc6, nullptr, dxyz, ds, dR, dtf);
        if (has_tf) {
#pragma unroll
            for (int b = 0; b < MGR_MAX_BONES; ++b) {
                if (b < B) {
                    const float* T = Tp + b * 16;
                    float a = 0.f;
#pragma unroll
                    for (int k = 0; k < 12; ++k) a += dtf[k] * T[k];
                    dw[b] = a;
                }
            }
        }
        dop = acc[5];
    }
    const bool acc_out = accumulate != 0;
    const bool lead = ok && vl == 0 && (grp_any || !acc_out);     // the lane that writes this Gaussian's rows
    if (any_tf && d_w) {      // (workgroup-uniform branch around the DPP sums; only articulated rows own a d_w row)
#pragma unroll
        for (int b = 0; b < MGR_MAX_BONES; ++b) {
            if (b < B) {
                const float t = grp_sum<G>(dw[b]);
                if (lead && has_tf) {
                    float* o = d_w + (size_t)i * B + b;
                    *o = acc_out ? *o + t : t;
                }
            }
        }
    }
    {
        const float sg = 1.0f / (1.0f + expf(-op_logit[i]));
        const float o7[7] = {dxyz[0], dxyz[1], dxyz[2], ds[0] * g.s[0], ds[1] * g.s[1], ds[2] * g.s[2], dop * sg * (1.0f - sg)};
        float t7[7], tR[9];
#pragma unroll
        for (int k = 0; k < 7; ++k) t7[k] = grp_sum<G>(o7[k]);
#pragma unroll
        for (int k = 0; k < 9; ++k) tR[k] = grp_sum<G>(dR[k]);
        if (lead) {
            float drot[4];
            quat_backward(g, tR, drot);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                d_xyz[3 * (size_t)i + k] = acc_out ? d_xyz[3 * (size_t)i + k] + t7[k] : t7[k];
                d_ls[3 * (size_t)i + k] = acc_out ? d_ls[3 * (size_t)i + k] + t7[3 + k] : t7[3 + k];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) d_rot[4 * (size_t)i + k] = acc_out ? d_rot[4 * (size_t)i + k] + drot[k] : drot[k];
            d_op[i] = acc_out ? d_op[i] + t7[6] : t7[6];
        }
    }
}

// Pose gradient of the map backward (mgr_views_maps_backward_pose): dL/dT[v][b] = sum_n w[n][b] * dtf[n][v], the other contraction
// of the dtf that k_views_feat_gather contracts with the bone transforms for d_skin_w.  A kernel of its own BEHIND the plain
// gather, which keeps its argument list and its code and writes the leaf rows: restating the gather's lane work inside a second
// kernel gave leaf rows that differ from k_views_feat_gather's in the last bit (the compiler contracts other multiply-adds
// there), and the leaf outputs of the two entries must be the same bits.  So this kernel repeats only what dtf needs -- the
// records of the lane's (view, Gaussian) in slot order, blend_tf / lbs_apply, project_backward, the depth's z row,
// lbs_backward_view -- for the ARTICULATED Gaussians, and writes no leaf row.  The lane layout of k_pose_part_views
// (raster_bwd.hip): lane = Gaussian_local * G + view_local; workgroup x stages the group's cameras and transforms once and takes
// the chunks x, x + gridDim.x, ... of 256 / G Gaussians (gridDim.x <= MGR_POSE_MAX_WG); a lane that held records parks dtf and
// its Gaussian index in LDS (MGR_POSE_REC words), pose_wg_lists / pose_wg_accumulate reduce the chunk per (view, bone) in lane
// order, and the workgroup stores ONE partial of G x B x 12 floats (part + x * G * B * 12), which k_pose_fold adds in slot order.
template <int G>
__global__ __launch_bounds__(VM_THREADS) void k_views_feat_gather_pose(
    int v_first, int v_count, int B, int n_art, int W, int H, const float* __restrict__ cams, const float* __restrict__ xyz,
    const float* __restrict__ log_scale, const float* __restrict__ rot, const float* __restrict__ skin_w,
    const float* __restrict__ transforms, const ushort4* __restrict__ rect, const uint32_t* __restrict__ pair_off,
    const uint32_t* __restrict__ tag, const float* __restrict__ rec, uint32_t cap, int N, int with_z, int n_chunks,
    float* __restrict__ part) {
    constexpr int IPB = VM_THREADS / G;
    extern __shared__ __align__(16) float s_vm[];        // G x (camera 40 | transforms VM_TSTRIDE(B))
    __shared__ float s_rec[VM_THREADS * MGR_POSE_REC];
    __shared__ unsigned char s_lst[G * VM_THREADS];
    __shared__ int s_cnt[8], s_wc[8 * (VM_THREADS / 64)];
    const int tid = threadIdx.x, vl = tid & (G - 1), il = tid / G;
    const int vstride = MGR_CAM_FLOATS + VM_TSTRIDE(B);
    for (int k = tid; k < G * MGR_CAM_FLOATS; k += VM_THREADS) {
        const int g = k / MGR_CAM_FLOATS, e = k % MGR_CAM_FLOATS;
        s_vm[g * vstride + e] = g < v_count ? cams[(size_t)(v_first + g) * MGR_CAM_FLOATS + e] : 0.f;
    }
    for (int k = tid; k < G * B * 16; k += VM_THREADS) {
        const int g = k / (B * 16), e = k % (B * 16);
        s_vm[g * vstride + MGR_CAM_FLOATS + e] = g < v_count ? transforms[(size_t)(v_first + g) * B * 16 + e] : 0.f;
    }
    __syncthreads();
    const float* const Tp = s_vm + vl * vstride + MGR_CAM_FLOATS;
    float pacc[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) pacc[k] = 0.f;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {      // (workgroup-uniform trip count: barriers inside)
        const int i = c * IPB + il;
        // the records of this (view, Gaussian), in slot order (k_views_feat_gather's loop)
        float acc[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float gz = 0.f;
        bool any = false;
        if (i < n_art && vl < v_count) {
            const size_t vi = (size_t)(v_first + vl) * N + i;
            const ushort4 rc = rect[vi];
            uint32_t cnt = (uint32_t)((rc.z - rc.x) * (rc.w - rc.y));
            const uint32_t off = pair_off[vi];
            if (cnt > 0 && off < cap) {
                cnt = min(cnt, cap - off);
                for (uint32_t s = 0; s < cnt; ++s) {
                    if (tag[off + s] != 1u) continue;
                    const float4* r = (const float4*)(rec + (size_t)(off + s) * FEAT_REC);
                    const float4 r0 = r[0], r1 = r[1];
                    acc[0] += r0.x; acc[1] += r0.y; acc[2] += r0.z; acc[3] += r0.w; acc[4] += r1.x; acc[5] += r1.y;
                    gz += r1.z;
                    any = true;
                }
            }
        }
        if (!with_z) gz = 0.f;
        if (any) {
            MgrCam cam;
            {
                const float* p = s_vm + vl * vstride;
                cam.tanfovx = p[0];
                cam.tanfovy = p[1];
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    cam.view[k] = p[2 + k];
                    cam.proj[k] = p[18 + k];
                }
                cam.campos[0] = p[34]; cam.campos[1] = p[35]; cam.campos[2] = p[36];
            }
            GaussCano g;
            cano_load(xyz, log_scale, rot, i, g);
            float dxyz[3] = {0.f, 0.f, 0.f}, ds[3] = {0.f, 0.f, 0.f};
            float dR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            float tf[12], p3[3], c6[6], dm[3], dc6[6], dtf[12];
            blend_tf(skin_w + (size_t)i * B, Tp, B, tf);
            lbs_apply(tf, g, p3, c6);
            project_backward(cam, W, H, p3, c6, acc, dm, dc6);
            dm[0] += cam.view[2] * gz; dm[1] += cam.view[6] * gz; dm[2] += cam.view[10] * gz;
            lbs_backward_view<false>(tf, g, dm, dc6, nullptr, dxyz, ds, dR, dtf);      // (dxyz / ds / dR: by-products, not used)
            float* r = s_rec + tid * MGR_POSE_REC;
#pragma unroll
            for (int k = 0; k < 12; ++k) r[k] = dtf[k];
            r[12] = __int_as_float(i);
        }
        pose_wg_lists<VM_THREADS>(tid, G, any ? vl : -1, s_lst, s_cnt, s_wc);
        pose_wg_accumulate<VM_THREADS>(tid, G, B, s_rec, s_lst, s_cnt, skin_w, pacc);
        __syncthreads();   // the next chunk's records
    }
    pose_wg_store<VM_THREADS>(tid, G, B, s_rec, pacc, part + (size_t)blockIdx.x * G * B * 12);
}

extern "C" size_t mgr_views_maps_backward_workspace_bytes(int V, int N, int W, int H, int64_t cap) {
    (void)W; (void)H;                 // (one record per (tile, Gaussian) pair; nothing is kept per pixel or per Gaussian)
    if (V <= 0 || N < 0 || cap < 0) return 0;
    return feat_scratch_layout(V, N, cap).geo;        // tags | records
}

// Partial slots of the pose kernel: one per workgroup, at most MGR_POSE_MAX_WG (the workspace is sized for n_articulated = N)
static int vm_pose_slots(int N, int Gv) {
    const int ipb = VM_THREADS / Gv, chunks = N / ipb + (N % ipb != 0 ? 1 : 0);      // (no N + ipb - 1: N may be INT_MAX)
    return chunks < MGR_POSE_MAX_WG ? chunks : MGR_POSE_MAX_WG;
}
extern "C" size_t mgr_views_maps_pose_workspace_bytes(int V, int N, int B) {
    if (V <= 0 || N <= 0 || B <= 0) return 0;
    const int Gv = V <= 1 ? 1 : V <= 2 ? 2 : V <= 4 ? 4 : 8;
    return ((size_t)vm_pose_slots(N, Gv) * Gv * B * 12 * sizeof(float) + 255) & ~(size_t)255;
}

struct VmPose {      // mgr_views_maps_backward_pose: what it adds to mgr_views_maps_backward
    int accumulate;
    float* d_T;
    void* ws;
    size_t ws_bytes;
};

static int views_maps_backward_impl(const char* who, const VmPose* pose, int V, int N, int B, int n_articulated, int W, int H,
                                    const float* cams, const float* xyz, const float* log_scale, const float* rot,
                                    const float* opacity_logit, const float* skin_w, const float* transforms, const float* out_alpha,
                                    const float* out_depth, const float* dL_dalpha, const float* dL_ddepth, int accumulate,
                                    float* d_xyz, float* d_log_scale, float* d_rot, float* d_opacity_logit, float* d_skin_w,
                                    const void* workspace, size_t workspace_bytes, int64_t cap, void* scratch,
                                    size_t scratch_bytes, int flags, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (V <= 0 || N < 0 || W <= 0 || H <= 0 || cap < 0 || cap > 0xFFFFFFF0ll) return mgr_fail(MGR_EINVAL, "%s: bad sizes", who);
    if (!dL_dalpha && !dL_ddepth) return mgr_fail(MGR_EINVAL, "%s: no upstream gradient (dL_dalpha and dL_ddepth are both NULL)", who);
    if ((dL_dalpha && !out_alpha) || (dL_ddepth && !out_depth) || !workspace || !scratch || !cams)
        return mgr_fail(MGR_EINVAL, "%s: null pointer", who);
    if (N > 0 && (!xyz || !log_scale || !rot || !opacity_logit || !d_xyz || !d_log_scale || !d_rot || !d_opacity_logit ||
                  (skin_w && (!transforms || !d_skin_w))))
        return mgr_fail(MGR_EINVAL, "%s: null pointer", who);
    if (skin_w && (B <= 0 || B > MGR_MAX_BONES)) return mgr_fail(MGR_EINVAL, "%s: bad B", who);
    if (skin_w && (n_articulated < 0 || n_articulated > N)) return mgr_fail(MGR_EINVAL, "%s: bad n_articulated", who);
    if (pose) {
        if (!skin_w || n_articulated <= 0)
            return mgr_fail(MGR_EINVAL, "%s: no articulated Gaussians (skin_w NULL or n_articulated <= 0): nothing to differentiate", who);
        if (!pose->d_T || !pose->ws) return mgr_fail(MGR_EINVAL, "%s: null pointer (d_transforms, pose_workspace)", who);
        if (pose->ws_bytes < mgr_views_maps_pose_workspace_bytes(V, N, B))
            return mgr_fail(MGR_ENOMEM, "%s: pose workspace smaller than mgr_views_maps_pose_workspace_bytes", who);
    }
    const int gx = (W + 15) / 16, gy = (H + 15) / 16;
    if (gx > 65535 || gy > 65535) return mgr_fail(MGR_EINVAL, "%s: image too large", who);
    const MgrLayout L = mgr_layout(V, N, W, H, cap);
    if (workspace_bytes < L.total) return mgr_fail(MGR_ENOMEM, "%s: workspace too small for these sizes", who);
    const FeatScratch S = feat_scratch_layout(V, N, cap);
    if (scratch_bytes < S.geo) return mgr_fail(MGR_ENOMEM, "%s: scratch smaller than mgr_views_maps_backward_workspace_bytes", who);
    const char* ws = (const char*)workspace;
    MgrHeader h;
    const int VT = V * gx * gy;
    {
        const int rc = feat_read_state(who, ws, L, V, N, W, H, cap, VT, stream, h);
        if (rc != MGR_OK) return rc;
    }
    if (N == 0) return MGR_OK;
    char* sc = (char*)scratch;
    // a slot nobody writes must count as zero: the tags are cleared per call, the one launch tags with 1
    MGR_HIP(hipMemsetAsync(sc + S.tag, 0, (size_t)(cap > 0 ? cap : 1) * 4, stream));

    FeatBwdArgs a;
    a.N = N; a.W = W; a.H = H; a.gx = gx; a.gy = gy; a.VT = VT;
    a.n_queue = h.queue_len_i; a.cap = (uint32_t)cap;
    a.tile_qrec = (const uint4*)(ws + L.tile_qrec);
    a.sorted_gid = (const uint32_t*)(ws + L.sorted_gid);
    a.grec = (const MgrGRec*)(ws + L.grec);
    a.depth = (const float*)(ws + L.depth);
    a.feat = nullptr; a.s_feat = 0; a.C = 0; a.c0 = 0; a.nc = 0;
    a.with_z = dL_ddepth ? 1 : 0;                     // the depth is the launch's only channel: slot 0 of the records
    a.out = out_depth; a.g_out = dL_ddepth; a.Cout = a.with_z;
    a.out_alpha = dL_dalpha ? out_alpha : nullptr;
    a.g_alpha = dL_dalpha;
    a.rec = (float*)(sc + S.rec); a.tag = (uint32_t*)(sc + S.tag);
    a.tagval = 1u;
    {
        MGR_PROF("k_blend_feat_bwd", stream);
        hipLaunchKernelGGL(k_blend_feat_bwd<2>, dim3(FEAT_GRID), dim3(256), 0, stream, a);
    }
    MGR_LAUNCH_CHECK("k_blend_feat_bwd", stream, flags & MGR_BWD_CHECK);

    const float* sw = (skin_w && n_articulated > 0) ? skin_w : nullptr;      // (no articulated Gaussian: the identity everywhere)
    const int n_art = sw ? n_articulated : 0;
    const int Gv = V <= 1 ? 1 : V <= 2 ? 2 : V <= 4 ? 4 : 8;
    const size_t lds = (size_t)Gv * (MGR_CAM_FLOATS + (sw ? VM_TSTRIDE(B) : 0)) * sizeof(float);
    const dim3 grid((unsigned)((N + VM_THREADS / Gv - 1) / (VM_THREADS / Gv)));
    for (int v0 = 0; v0 < V; v0 += Gv) {
        const int vc = V - v0 < Gv ? V - v0 : Gv;
        const int accm = (accumulate || v0 > 0) ? 1 : 0;
        {
            MGR_PROF("k_views_feat_gather", stream);
#define MGR_VM_LAUNCH(GG)                                                                                                         \
    hipLaunchKernelGGL((k_views_feat_gather<GG>), grid, dim3(VM_THREADS), lds, stream, v0, vc, N, B, n_art, W, H, cams, xyz, log_scale, \
                       rot, opacity_logit, sw, transforms, (const ushort4*)(ws + L.rect), (const uint32_t*)(ws + L.pair_off),    \
                       (const uint32_t*)a.tag, (const float*)a.rec, (uint32_t)cap, a.with_z, accm, d_xyz, d_log_scale, d_rot,    \
                       d_opacity_logit, d_skin_w)
            if (Gv == 8) MGR_VM_LAUNCH(8);
            else if (Gv == 4) MGR_VM_LAUNCH(4);
            else if (Gv == 2) MGR_VM_LAUNCH(2);
            else MGR_VM_LAUNCH(1);
#undef MGR_VM_LAUNCH
        }
        MGR_LAUNCH_CHECK("k_views_feat_gather", stream, flags & MGR_BWD_CHECK);
        if (pose) {
            // the pose gradient of this group's views: partials over the articulated Gaussians, then the fold that writes (or,
            // accumulate_pose, adds to) the group's rows of d_transforms
            const int ipb = VM_THREADS / Gv, n_chunks = (n_art + ipb - 1) / ipb, slots = vm_pose_slots(n_art, Gv);
            {
                MGR_PROF("k_views_feat_gather_pose", stream);
#define MGR_VMP_LAUNCH(GG)                                                                                                        \
    hipLaunchKernelGGL((k_views_feat_gather_pose<GG>), dim3((unsigned)slots), dim3(VM_THREADS), lds, stream, v0, vc, B, n_art, W, H,  \
                       cams, xyz, log_scale, rot, sw, transforms, (const ushort4*)(ws + L.rect), (const uint32_t*)(ws + L.pair_off), \
                       (const uint32_t*)a.tag, (const float*)a.rec, (uint32_t)cap, N, a.with_z, n_chunks, (float*)pose->ws)
                if (Gv == 8) MGR_VMP_LAUNCH(8);
                else if (Gv == 4) MGR_VMP_LAUNCH(4);
                else if (Gv == 2) MGR_VMP_LAUNCH(2);
                else MGR_VMP_LAUNCH(1);
#undef MGR_VMP_LAUNCH
            }
            MGR_LAUNCH_CHECK("k_views_feat_gather_pose", stream, flags & MGR_BWD_CHECK);
            const int rc = mgr_pose_fold_acc(v0, vc, Gv, B, (const float*)pose->ws, slots, pose->accumulate, pose->d_T, stream);
            if (rc != MGR_OK) return rc;
        }
    }
    return MGR_OK;
}

extern "C" int mgr_views_maps_backward(int V, int N, int B, int n_articulated, int W, int H, const float* cams, const float* xyz,
                                       const float* log_scale, const float* rot, const float* opacity_logit, const float* skin_w,
                                       const float* transforms, const float* out_alpha, const float* out_depth,
                                       const float* dL_dalpha, const float* dL_ddepth, int accumulate, float* d_xyz,
                                       float* d_log_scale, float* d_rot, float* d_opacity_logit, float* d_skin_w,
                                       const void* workspace, size_t workspace_bytes, int64_t cap, void* scratch,
                                       size_t scratch_bytes, int flags, void* stream) {
    return views_maps_backward_impl("mgr_views_maps_backward", nullptr, V, N, B, n_articulated, W, H, cams, xyz, log_scale, rot,
                                    opacity_logit, skin_w, transforms, out_alpha, out_depth, dL_dalpha, dL_ddepth, accumulate, d_xyz,
                                    d_log_scale, d_rot, d_opacity_logit, d_skin_w, workspace, workspace_bytes, cap, scratch,
                                    scratch_bytes, flags, stream);
}

extern "C" int mgr_views_maps_backward_pose(int V, int N, int B, int n_articulated, int W, int H, const float* cams, const float* xyz,
                                            const float* log_scale, const float* rot, const float* opacity_logit,
                                            const float* skin_w, const float* transforms, const float* out_alpha,
                                            const float* out_depth, const float* dL_dalpha, const float* dL_ddepth, int accumulate,
                                            float* d_xyz, float* d_log_scale, float* d_rot, float* d_opacity_logit, float* d_skin_w,
                                            const void* workspace, size_t workspace_bytes, int64_t cap, void* scratch,
                                            size_t scratch_bytes, int flags, int accumulate_pose, float* d_transforms,
                                            void* pose_workspace, size_t pose_workspace_bytes, void* stream) {
    const VmPose pose = {accumulate_pose, d_transforms, pose_workspace, pose_workspace_bytes};
    return views_maps_backward_impl("mgr_views_maps_backward_pose", &pose, V, N, B, n_articulated, W, H, cams, xyz, log_scale, rot,
                                    opacity_logit, skin_w, transforms, out_alpha, out_depth, dL_dalpha, dL_ddepth, accumulate, d_xyz,
                                    d_log_scale, d_rot, d_opacity_logit, d_skin_w, workspace, workspace_bytes, cap, scratch,
                                    scratch_bytes, flags, stream);
}
