// Feature render: composite caller channels, expected depth and accumulated opacity over the tile lists the last forward
// left in a workspace (mgr_raster_blend_features).  Forward only, the workspace is read and never written.
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
#include "mgr_common.h"

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
    // what the last forward left: one blocking read of the header, then every refusal is the host's (nothing is launched)
    const char* ws = (const char*)workspace;
    MgrHeader h;
    const size_t head_bytes = offsetof(MgrHeader, qctr);
    MGR_HIP(hipMemcpyAsync(&h, ws + L.header, head_bytes, hipMemcpyDeviceToHost, stream));
    MGR_HIP(hipStreamSynchronize(stream));
    if (h.fwd_seq == 0u) return mgr_fail(MGR_ESTATE, "mgr_raster_blend_features: no forward has run on this workspace");
    if (h.feat_seq != h.fwd_seq)
        return mgr_fail(MGR_ESTATE, "mgr_raster_blend_features: the last forward on this workspace did not run its blend (MGR_FWD_NO_BLEND)");
    if (h.feat_dims[0] != (uint32_t)V || h.feat_dims[1] != (uint32_t)N || h.feat_dims[2] != (uint32_t)W ||
        h.feat_dims[3] != (uint32_t)H || h.feat_dims[4] != (uint32_t)cap)
        return mgr_fail(MGR_ESTATE, "mgr_raster_blend_features: the last forward on this workspace was made for another V, N, W, H or pair capacity");
    if (h.feat_flags & MGR_FEAT_CUT)
        return mgr_fail(MGR_ESTATE, "mgr_raster_blend_features: the last forward applied the depth cut (MGR_FWD_DEPTH_CUT): its lists are cut short");
    if (h.overflow != 0u)
        return mgr_fail(MGR_ESTATE, "mgr_raster_blend_features: the last forward raised an overflow bit: its lists are incomplete");
    const int VT = V * gx * gy;
    if (h.queue_len > (uint32_t)VT || h.queue_len_i > (uint32_t)VT)
        return mgr_fail(MGR_ESTATE, "mgr_raster_blend_features: the header's queue lengths do not fit these sizes");

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
