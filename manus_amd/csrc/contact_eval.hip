// Contact evaluation for gfx950: from the 'acc_gt_eval' frame (skin-weight colours | grey contact map), the ground-truth
// contact segmentation and the ground-truth RGBA photo of V evaluation cameras to the masks, the per-pixel bone labels,
// the [I, A, B] counts behind IoU / F1 (combined and per bone) and the collage rows.
//
// Replaces, for V cameras per launch chain, scripts/process/get_iou_ours.py and get_iou.py of brown-ivl/manus:
//     cv2.inRange on the segmentation / the right half of the frame, alpha > 128       get_iou_ours.py:313-322
//     get_skin_mask: 16 x (inRange, erode, dilate), argmax, nearest-labelled fill      :74-151
//     get_contact_dist (taichi, N_res x N_skin pair tests)                             :44-71
//     cal_iou / f1_score inputs of evaluate_metric and calculate_per_bone_iou          :162-232
//     blend_masks / combine_images                                                     :269-291
//
// Everything is integer: no float atomics, no floating point at all behind the optional fp32 -> byte conversion of a
// frame.  Integer atomics are used for a view's bounding box of labelled tiles, for LDS counters and to hand out slots
// of the residual list; the list's ORDER varies from run to run, what is computed per pixel does not, so two calls on
// the same inputs give the same bytes, and a view's outputs depend on that view's images only.
//
// k_ceval_labels   a workgroup owns 64 x 16 pixels.  The left half's bytes of its 68 x 20 halo region are staged in LDS
//                  with dword loads; the 16 palette tests of a pixel become ONE 16-bit word (bit i: every channel within
//                  +-10 of palette entry i), so the 3x3 MORPH_ELLIPSE (= 4-neighbour cross) erosion is an AND of five
//                  words, the dilation an OR of five eroded words and the argmax over [background, m1..m16] a
//                  find-first-set.  OpenCV's default borders: outside the image counts as set for the erosion (word
//                  0xFFFF) and as unset for the dilation (eroded word 0).  The same kernel writes what the fill needs: a
//                  bitmap of the labelled pixels per 16 x 16 tile (16 rows of 16 bits), the tile bounding box of the
//                  view's labelled pixels and the compacted list of residual pixels (inside the hand, no label).
// k_ceval_fill     one lane per residual pixel.  The nearest labelled pixel under  min (d^2, row * W + col)  -- the
//                  reference's strict '<' scan of np.argwhere order on fp32 roots, which is this integer rule whenever
//                  the winning d^2 is below 4197200: fp32 sqrt over the integers is strictly increasing up to there (the
//                  first n with sqrt32(n) == sqrt32(n + 1), just above 2^22), so for a nearest labelled pixel closer than
//                  2048 px -- is searched over tiles in rings of growing Chebyshev distance, starting at the
//                  first ring that reaches the view's bounding box and ending when the nearest possible pixel of the
//                  next ring is farther than the best d^2 (or the box is exhausted).  In a tile row the nearest set bit
//                  to the pixel's column (left one on a tie: lower index) is the only candidate that can win, so a tile
//                  costs at most 16 bit searches whatever its population.  The N_res x N_skin scan is never done.
// k_ceval_counts   LDS integer counters per workgroup -> one record of 51 words; k_ceval_fold adds a view's records.
// k_ceval_collage  every output byte is a function of (photo byte, panel kind, alpha bit, channel): the host builds that
//                  table with the reference's float64 numpy expression, the kernel looks it up.
#include "mgr_common.h"

#define CE_T 256
#define CE_TILE 16                     // edge of an occupancy tile
#define CE_LW 64                       // pixels of a k_ceval_labels workgroup: 64 x 16 = four tiles side by side, one per wave
#define CE_LH 16
#define CE_MW (CE_LW + 4)              // staged match words per row (halo 2)
#define CE_MH (CE_LH + 4)
#define CE_RAW_DW 53                   // dwords of a staged row: 68 * 3 = 204 bytes + at most 3 in front of them = 52 dwords (+1: odd stride)
#define CE_NREC 51                     // 17 classes x [I, A, B]
#define CE_CNT_PX (CE_T * 16)          // pixels per workgroup of k_ceval_counts
#define CE_FOLD_G 16                   // groups of 64 threads of k_ceval_fold
#define CE_MAXDIM 16384                // d^2 < 2^30 and row * W + col < 2^28 fit 32 bits each
#define CE_FILL_BLOCKS 1024            // grid-stride workgroups per view of k_ceval_fill

struct CeView {                        // per view, zeroed by mgr_ceval_labels
    uint32_t nx0, ny0, x1, y1;         // labelled tiles: max of (65536 - tx), of (65536 - ty), of (tx + 1), of (ty + 1); 0 = none
    uint32_t n_res;                    // residual pixels listed
    uint32_t pad[3];
};
struct CeLayout {
    size_t view, occ, list, rec, total;
};
static inline int ce_tiles(int n) { return (n + CE_TILE - 1) / CE_TILE; }
static inline int64_t ce_cnt_blocks(int H, int W) { return ((int64_t)H * W + CE_CNT_PX - 1) / CE_CNT_PX; }
static CeLayout ce_layout(int V, int H, int W) {
    CeLayout L;
    size_t o = 0;
    L.view = o; o += mgr_align((size_t)V * sizeof(CeView));
    L.occ = o;  o += mgr_align((size_t)V * ce_tiles(H) * ce_tiles(W) * 8 * 4);
    L.list = o; o += mgr_align((size_t)V * H * W * 4);
    L.rec = o;  o += mgr_align((size_t)V * (size_t)ce_cnt_blocks(H, W) * CE_NREC * 4);
    L.total = o;
    return L;
}

// uint8(clamp(x, 0, 1) * 255) with the product in fp32, truncating: test_step's conversion of a render (base.py:245-246);
// NaN gives 0 as in eval.hip.
__device__ __forceinline__ uint32_t ce_render_byte(float p) {
    return p != p ? 0u : (uint32_t)(int)(fminf(fmaxf(p, 0.f), 1.f) * 255.0f);
}

// ---------------------------------------------------------------------------------------------------------------------
// masks
// ---------------------------------------------------------------------------------------------------------------------
template <bool F32>
__global__ __launch_bounds__(CE_T) void k_ceval_masks(int H, int W, const void* __restrict__ frame, const uint8_t* __restrict__ seg,
                                                      const uint32_t* __restrict__ rgba, uint8_t* __restrict__ frame_u8,
                                                      uint8_t* __restrict__ pred, uint8_t* __restrict__ gt, uint8_t* __restrict__ hand) {
    const int v = blockIdx.y;
    const size_t plane = (size_t)H * W, p = (size_t)blockIdx.x * CE_T + threadIdx.x;
    if (p >= plane) return;
    const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
    const size_t fl = (((size_t)v * H + y) * 2 * W + x) * 3, fr = fl + (size_t)3 * W;    // the pixel in the left / right half
    uint32_t c[3];
    if constexpr (F32) {
        const float* f = (const float*)frame;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            frame_u8[fl + k] = (uint8_t)ce_render_byte(f[fl + k]);
            c[k] = ce_render_byte(f[fr + k]);
            frame_u8[fr + k] = (uint8_t)c[k];
        }
    } else {
        const uint8_t* f = (const uint8_t*)frame;
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = f[fr + k];
    }
    const size_t q = (size_t)v * plane + p;
    const uint8_t* s = seg + q * 3;
    // cv2.inRange(img, (128,128,128), (255,255,255)): every channel >= 128
    pred[q] = (c[0] >= 128u && c[1] >= 128u && c[2] >= 128u) ? 1 : 0;
    gt[q] = (s[0] >= 128u && s[1] >= 128u && s[2] >= 128u) ? 1 : 0;
    hand[q] = (rgba[q] >> 24) > 128u ? 1 : 0;                                             // gt_rgb[..., -1] > 128
}

// ---------------------------------------------------------------------------------------------------------------------
// labels
// ---------------------------------------------------------------------------------------------------------------------
// bit i: the pixel lies in palette entry i's box, every channel within +-10 inclusive (get_skin_mask :94-123; data)
__device__ __forceinline__ uint32_t ce_match(uint32_t r, uint32_t g, uint32_t b) {
    constexpr int P[16][3] = {{43, 159, 43},   {31, 119, 178},  {173, 198, 231}, {254, 186, 119}, {151, 222, 137}, {213, 38, 39},
                              {254, 151, 149}, {196, 175, 212}, {139, 85, 74},   {195, 155, 147}, {246, 181, 209}, {126, 126, 126},
                              {198, 199, 198}, {218, 218, 140}, {25, 190, 206},  {156, 217, 228}};
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const bool in = (uint32_t)((int)r - P[i][0] + 10) <= 20u && (uint32_t)((int)g - P[i][1] + 10) <= 20u &&
                        (uint32_t)((int)b - P[i][2] + 10) <= 20u;
        m |= (in ? 1u : 0u) << i;
    }
    return m;
}

// frame: (V, H, row_px, 3) bytes whose first W pixels of every row are the skin-weight render (row_px = 2W: the whole
// 'acc_gt_eval' frame; row_px = W: the left half on its own); frame_bytes = the size of that buffer.  VEC: W % 4 == 0 and
// 4-byte aligned labels / hand, so that a thread's four pixels are one dword.
template <bool VEC>
__global__ __launch_bounds__(CE_T) void k_ceval_labels(int H, int W, int row_px, const uint8_t* __restrict__ frame, size_t frame_bytes,
                                                       const uint8_t* __restrict__ hand, uint8_t* __restrict__ labels,
                                                       uint32_t* __restrict__ occ, CeView* __restrict__ views, uint32_t* __restrict__ list) {
    __shared__ uint32_t s_raw[CE_MH][CE_RAW_DW];
    __shared__ uint32_t s_m[CE_MH][CE_MW + 1];
    __shared__ uint32_t s_e[CE_LH + 2][CE_LW + 2 + 1];
    const int tid = threadIdx.x, v = blockIdx.z, x0 = blockIdx.x * CE_LW, y0 = blockIdx.y * CE_LH;
    const int xa = max(x0 - 2, 0), xb = min(x0 + CE_LW + 2, W);          // staged columns [xa, xb)

    // 1. the rows' bytes, as aligned dwords (the last dword of the buffer byte by byte when it is not whole)
    for (int t = tid; t < CE_MH * CE_RAW_DW; t += CE_T) {
        const int j = t / CE_RAW_DW, k = t - j * CE_RAW_DW, y = y0 - 2 + j;
        if (y < 0 || y >= H) continue;
        const size_t b0 = (((size_t)v * H + y) * row_px + xa) * 3, b1 = b0 + (size_t)(xb - xa) * 3;
        const size_t a = (b0 & ~(size_t)3) + 4 * (size_t)k;
        if (a >= b1) continue;
        uint32_t w = 0;
        if (a + 4 <= frame_bytes) {
            w = *(const uint32_t*)(frame + a);
        } else {
            for (int q = 0; q < 4; ++q)
                if (a + q < frame_bytes) w |= (uint32_t)frame[a + q] << (8 * q);
        }
        s_raw[j][k] = w;
    }
    __syncthreads();
    // 2. match words; outside the image: all set (the erosion's border value)
    for (int t = tid; t < CE_MH * CE_MW; t += CE_T) {
        const int j = t / CE_MW, i = t - j * CE_MW, y = y0 - 2 + j, x = x0 - 2 + i;
        uint32_t m = 0xFFFFu;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t b0 = (((size_t)v * H + y) * row_px + xa) * 3;
            const uint8_t* rb = (const uint8_t*)s_raw[j] + (b0 & 3) + (size_t)(x - xa) * 3;
            m = ce_match(rb[0], rb[1], rb[2]);
        }
        s_m[j][i] = m;
    }
    __syncthreads();
    // 3. eroded words of the 66 x 18 region; outside the image: none set (the dilation's border value)
    for (int t = tid; t < (CE_LH + 2) * (CE_LW + 2); t += CE_T) {
        const int j = t / (CE_LW + 2), i = t - j * (CE_LW + 2), y = y0 - 1 + j, x = x0 - 1 + i;
        uint32_t e = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) e = s_m[j + 1][i + 1] & s_m[j][i + 1] & s_m[j + 2][i + 1] & s_m[j + 1][i] & s_m[j + 1][i + 2];
        s_e[j][i] = e;
    }
    __syncthreads();
    // 4. dilation, first match, hand: wave w owns tile w of the four; lane -> row lane / 4, four pixels from column 4 * (lane % 4)
    const int w = tid >> 6, lane = tid & 63, r = lane >> 2, q = (lane & 3) * 4;
    const int y = y0 + r, lx0 = w * CE_TILE + q, xg = x0 + lx0;
    const size_t off = ((size_t)v * H + y) * W + xg;
    uint32_t hand4 = 0x01010101u;
    if (hand && y < H && xg < W) {
        if constexpr (VEC) {
            hand4 = *(const uint32_t*)(hand + off);
        } else {
            hand4 = 0;
            for (int k = 0; k < 4; ++k)
                if (xg + k < W) hand4 |= (uint32_t)hand[off + k] << (8 * k);
        }
    }
    uint32_t lab4 = 0, bits_lab = 0, bits_res = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int lx = lx0 + k;
        if (y < H && x0 + lx < W) {
            const uint32_t d = s_e[r + 1][lx + 1] | s_e[r][lx + 1] | s_e[r + 2][lx + 1] | s_e[r + 1][lx] | s_e[r + 1][lx + 2];
            const bool hd = ((hand4 >> (8 * k)) & 0xFFu) != 0;
            const uint32_t lab = (d != 0 && hd) ? (uint32_t)__builtin_ctz(d) + 1u : 0u;      // all_masks * gt_mask
            lab4 |= lab << (8 * k);
            bits_lab |= (lab != 0 ? 1u : 0u) << k;
            bits_res |= ((hd && lab == 0) ? 1u : 0u) << k;                                   // xor(gt_mask > 0, all_masks > 0)
        }
    }
    if (y < H && xg < W) {
        if constexpr (VEC) {
            *(uint32_t*)(labels + off) = lab4;
        } else {
            for (int k = 0; k < 4; ++k)
                if (xg + k < W) labels[off + k] = (uint8_t)(lab4 >> (8 * k));
        }
    }
    // the tile's bitmap: 16 bits per row, two rows per word
    uint32_t row = bits_lab << q;
    row |= (uint32_t)__shfl_xor((int)row, 1, 64);
    row |= (uint32_t)__shfl_xor((int)row, 2, 64);
    const uint32_t below = (uint32_t)__shfl_down((int)row, 4, 64);
    const int TX = (W + CE_TILE - 1) / CE_TILE, TY = gridDim.y, tx = blockIdx.x * 4 + w, ty = blockIdx.y;
    const bool tile_in = tx < TX;
    if (tile_in && (lane & 7) == 0) occ[(((size_t)v * TY + ty) * TX + tx) * 8 + (lane >> 3)] = row | (below << 16);
    const unsigned long long any_lab = __builtin_amdgcn_ballot_w64(bits_lab != 0);
    if (tile_in && any_lab != 0ull && lane == 0) {
        atomicMax(&views[v].nx0, 65536u - (uint32_t)tx);
        atomicMax(&views[v].ny0, 65536u - (uint32_t)ty);
        atomicMax(&views[v].x1, (uint32_t)tx + 1u);
        atomicMax(&views[v].y1, (uint32_t)ty + 1u);
    }
    // residual pixels -> the view's list, one atomic per wave
    const uint32_t mine = (uint32_t)__popc(bits_res);
    const uint32_t incl = mgr_wave_incl_scan_u32(mine);
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (total != 0) {      // wave-uniform
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&views[v].n_res, total);
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
        uint32_t slot = base + incl - mine;
        uint32_t* lv = list + (size_t)v * H * W;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((bits_res >> k) & 1u) lv[slot++] = (uint32_t)(y * W + xg + k);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// fill
// ---------------------------------------------------------------------------------------------------------------------
// One tile against the running best key = (d^2 << 32 | row * W + col).
__device__ __forceinline__ void ce_visit(const uint32_t* __restrict__ occ_v, int TX, int W, int tx, int ty, int px, int py,
                                         unsigned long long& best) {
    const int tx0 = tx * CE_TILE, ty0 = ty * CE_TILE;
    const int dxm = px < tx0 ? tx0 - px : (px > tx0 + CE_TILE - 1 ? px - (tx0 + CE_TILE - 1) : 0);
    const int dym = py < ty0 ? ty0 - py : (py > ty0 + CE_TILE - 1 ? py - (ty0 + CE_TILE - 1) : 0);
    const uint32_t best_d2 = (uint32_t)(best >> 32);
    if ((uint32_t)(dxm * dxm + dym * dym) > best_d2) return;      // (equal: a lower index may still win)
    const uint4* t4 = (const uint4*)(occ_v + ((size_t)ty * TX + tx) * 8);
    const uint4 a = t4[0], b = t4[1];
    if ((a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) == 0u) return;
    const uint32_t wd[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const int c = min(max(px - tx0, 0), CE_TILE - 1);            // the pixel's column clamped into the tile: distances to set bits keep their order
#pragma unroll
    for (int rr = 0; rr < CE_TILE; ++rr) {
        const uint32_t m = (wd[rr >> 1] >> (16 * (rr & 1))) & 0xFFFFu;
        if (m == 0u) continue;
        const int yy = ty0 + rr, dy = yy - py;
        const uint32_t right = m >> c, left = m & ((1u << c) - 1u);
        int pos;
        if (left == 0u) {
            pos = c + __builtin_ctz(right);
        } else {
            const int pl = 31 - __builtin_clz(left);
            pos = pl;
            if (right != 0u) {
                const int prr = c + __builtin_ctz(right);
                if (prr - c < c - pl) pos = prr;                 // a tie goes to the left one: the lower index
            }
        }
        const int xx = tx0 + pos, dx = xx - px;
        const unsigned long long key = ((unsigned long long)(uint32_t)(dx * dx + dy * dy) << 32) | (uint32_t)(yy * W + xx);
        best = key < best ? key : best;
    }
}

__global__ __launch_bounds__(CE_T) void k_ceval_fill(int H, int W, const CeView* __restrict__ views, const uint32_t* __restrict__ occ,
                                                     const uint32_t* __restrict__ list, uint8_t* __restrict__ labels,
                                                     int32_t* __restrict__ flags) {
    const int v = blockIdx.y;
    const CeView cv = views[v];
    if (cv.n_res == 0u) return;
    if (cv.x1 == 0u) {                 // residual pixels and nothing labelled: the reference indexes an empty array here
        if (blockIdx.x == 0 && threadIdx.x == 0) flags[v] = 1;
        return;
    }
    const int TX = (W + CE_TILE - 1) / CE_TILE, TY = (H + CE_TILE - 1) / CE_TILE;
    const int bx0 = 65536 - (int)cv.nx0, by0 = 65536 - (int)cv.ny0, bx1 = (int)cv.x1 - 1, by1 = (int)cv.y1 - 1;   // inclusive
    const uint32_t* occ_v = occ + (size_t)v * TY * TX * 8;
    const uint32_t* lv = list + (size_t)v * H * W;
    uint8_t* lab_v = labels + (size_t)v * H * W;
    for (uint32_t i = blockIdx.x * CE_T + threadIdx.x; i < cv.n_res; i += gridDim.x * CE_T) {
        const uint32_t p = lv[i];
        const int py = (int)(p / (uint32_t)W), px = (int)(p - (uint32_t)py * (uint32_t)W);
        const int tcx = px >> 4, tcy = py >> 4;
        const int edge = min(min(px & 15, 15 - (px & 15)), min(py & 15, 15 - (py & 15)));
        const int r_first = max(max(bx0 - tcx, tcx - bx1), max(max(by0 - tcy, tcy - by1), 0));
        const int r_last = max(max(tcx - bx0, bx1 - tcx), max(tcy - by0, by1 - tcy));
        unsigned long long best = ~0ull;
        for (int r = r_first; r <= r_last; ++r) {
            if (r > 0) {               // every pixel of ring r lies at least this far away along one axis
                const long long lb = (long long)CE_TILE * (r - 1) + 1 + edge;
                if ((unsigned long long)(lb * lb) > (best >> 32)) break;
            }
            const int xl = max(tcx - r, bx0), xr = min(tcx + r, bx1);
            if (tcy - r >= by0 && tcy - r <= by1)
                for (int tx = xl; tx <= xr; ++tx) ce_visit(occ_v, TX, W, tx, tcy - r, px, py, best);
            if (r > 0 && tcy + r >= by0 && tcy + r <= by1)
                for (int tx = xl; tx <= xr; ++tx) ce_visit(occ_v, TX, W, tx, tcy + r, px, py, best);
            if (r > 0) {
                const int yt = max(tcy - r + 1, by0), yb = min(tcy + r - 1, by1);
                if (tcx - r >= bx0 && tcx - r <= bx1)
                    for (int ty = yt; ty <= yb; ++ty) ce_visit(occ_v, TX, W, tcx - r, ty, px, py, best);
                if (tcx + r >= bx0 && tcx + r <= bx1)
                    for (int ty = yt; ty <= yb; ++ty) ce_visit(occ_v, TX, W, tcx + r, ty, px, py, best);
            }
        }
        // (the box is not empty, so a labelled pixel was found; labelled pixels are never written: in place is safe)
        if (best != ~0ull) lab_v[p] = lab_v[(uint32_t)best];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// counts
// ---------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(CE_T) void k_ceval_counts(size_t plane, const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt,
                                                       const uint8_t* __restrict__ labels, uint32_t* __restrict__ rec) {
    __shared__ uint32_t s_cnt[CE_NREC];
    const int tid = threadIdx.x, v = blockIdx.y;
    if (tid < CE_NREC) s_cnt[tid] = 0;
    __syncthreads();
    const size_t vb = (size_t)v * plane;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const size_t p = (size_t)blockIdx.x * CE_CNT_PX + (size_t)it * (CE_T * 4) + (size_t)tid * 4;
        if (p >= plane) continue;
        uint32_t p4 = 0, g4 = 0, l4 = 0;
        if constexpr (VEC) {           // plane % 4 == 0: the dword is whole
            p4 = *(const uint32_t*)(pred + vb + p);
            g4 = *(const uint32_t*)(gt + vb + p);
            l4 = *(const uint32_t*)(labels + vb + p);
        } else {
            for (int k = 0; k < 4; ++k)
                if (p + k < plane) {
                    p4 |= (uint32_t)pred[vb + p + k] << (8 * k);
                    g4 |= (uint32_t)gt[vb + p + k] << (8 * k);
                    l4 |= (uint32_t)labels[vb + p + k] << (8 * k);
                }
        }
        if ((p4 | g4) == 0u) continue;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t pb = ((p4 >> (8 * k)) & 0xFFu) != 0 ? 1u : 0u, gb = ((g4 >> (8 * k)) & 0xFFu) != 0 ? 1u : 0u;
            const uint32_t L = (l4 >> (8 * k)) & 0xFFu;
            if ((pb | gb) == 0u) continue;
            // classes 0..15 are `skin_mask == i` (0 = no label, 16 is never scored: calculate_per_bone_iou); 16 = combined
            for (int cls = (L < 16u ? (int)L : 16); cls <= 16; cls = (cls == 16 ? 17 : 16)) {
                if (gb & pb) atomicAdd(&s_cnt[cls * 3 + 0], 1u);
                if (gb) atomicAdd(&s_cnt[cls * 3 + 1], 1u);
                if (pb) atomicAdd(&s_cnt[cls * 3 + 2], 1u);
            }
        }
    }
    __syncthreads();
    if (tid < CE_NREC) rec[((size_t)v * gridDim.x + blockIdx.x) * CE_NREC + tid] = s_cnt[tid];
}

// One workgroup per view: 16 groups of 64 threads add every 16th record, thread t < 51 of group 0 adds the 16 partial sums.
// Integers: the order does not matter.
__global__ __launch_bounds__(CE_FOLD_G * 64) void k_ceval_fold(int per_view, const uint32_t* __restrict__ rec, int64_t* __restrict__ counts) {
    __shared__ int64_t s_part[CE_FOLD_G][64];
    const int t = threadIdx.x & 63, grp = threadIdx.x >> 6, v = blockIdx.x;
    int64_t s = 0;
    if (t < CE_NREC) {
        const uint32_t* r = rec + (size_t)v * per_view * CE_NREC + t;
        for (int k = grp; k < per_view; k += CE_FOLD_G) s += (int64_t)r[(size_t)k * CE_NREC];
    }
    s_part[grp][t] = s;
    __syncthreads();
    if (grp == 0 && t < CE_NREC) {
        int64_t a = 0;
#pragma unroll
        for (int k = 0; k < CE_FOLD_G; ++k) a += s_part[k][t];
        counts[(size_t)v * CE_NREC + t] = a;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// collage
// ---------------------------------------------------------------------------------------------------------------------
// out (V, H, (1 + M) * W, 3): the photo on white, then the photo blended with each of the M masks.
// table[((byte * 3 + kind) * 2 + alpha) * 3 + channel], kind 0: plain panel, 1 / 2: blended with a clear / set mask pixel.
__global__ __launch_bounds__(CE_T) void k_ceval_collage(int V, int H, int W, int M, const uint32_t* __restrict__ rgba,
                                                        const uint8_t* __restrict__ masks, const uint8_t* __restrict__ table,
                                                        uint8_t* __restrict__ out) {
    const int v = blockIdx.y;
    const size_t plane = (size_t)H * W, p = (size_t)blockIdx.x * CE_T + threadIdx.x;
    if (p >= plane) return;
    const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
    const uint32_t px = rgba[(size_t)v * plane + p];
    const uint32_t al = (px >> 24) > 128u ? 1u : 0u;
    uint8_t* o = out + ((((size_t)v * H + y) * (size_t)(1 + M)) * W + x) * 3;
    for (int m = -1; m < M; ++m) {
        const uint32_t kind = m < 0 ? 0u : (masks[((size_t)m * V + v) * plane + p] != 0 ? 2u : 1u);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t byte = (px >> (8 * c)) & 0xFFu;
            o[c] = table[((byte * 3u + kind) * 2u + al) * 3u + (uint32_t)c];
        }
        o += (size_t)3 * W;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// entries
// ---------------------------------------------------------------------------------------------------------------------
static int ce_check_sizes(const char* who, int V, int H, int W) {
    if (V <= 0 || H <= 0 || W <= 0) return mgr_fail(MGR_EINVAL, "%s: bad sizes", who);
    if (V > 65535 || H > CE_MAXDIM || W > CE_MAXDIM) return mgr_fail(MGR_EINVAL, "%s: V <= 65535, H and W <= 16384", who);
    return MGR_OK;
}
static inline bool ce_al4(const void* p) { return (((uintptr_t)p) & 3) == 0; }

extern "C" size_t mgr_ceval_workspace_bytes(int V, int H, int W) {
    if (V <= 0 || H <= 0 || W <= 0 || V > 65535 || H > CE_MAXDIM || W > CE_MAXDIM) return 0;
    return ce_layout(V, H, W).total;
}

extern "C" int mgr_ceval_masks(int V, int H, int W, const void* frame, int frame_is_f32, const uint8_t* gt_seg, const uint8_t* gt_rgba,
                               uint8_t* frame_u8, uint8_t* pred, uint8_t* gt, uint8_t* hand, void* stream_) {
    if (int e = ce_check_sizes("mgr_ceval_masks", V, H, W)) return e;
    if (!frame || !gt_seg || !gt_rgba || !pred || !gt || !hand) return mgr_fail(MGR_EINVAL, "mgr_ceval_masks: null pointer");
    if (frame_is_f32 && !frame_u8) return mgr_fail(MGR_EINVAL, "mgr_ceval_masks: an fp32 frame needs frame_u8");
    if (!ce_al4(gt_rgba) || (frame_is_f32 && !ce_al4(frame))) return mgr_fail(MGR_EINVAL, "mgr_ceval_masks: gt_rgba / fp32 frame not 4-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t plane = (size_t)H * W;
    const dim3 grid((unsigned)((plane + CE_T - 1) / CE_T), V);
    MGR_PROF("k_ceval_masks", stream);
    if (frame_is_f32)
        hipLaunchKernelGGL(k_ceval_masks<true>, grid, dim3(CE_T), 0, stream, H, W, frame, gt_seg, (const uint32_t*)gt_rgba, frame_u8, pred, gt, hand);
    else
        hipLaunchKernelGGL(k_ceval_masks<false>, grid, dim3(CE_T), 0, stream, H, W, frame, gt_seg, (const uint32_t*)gt_rgba, frame_u8, pred, gt, hand);
    MGR_LAUNCH_CHECK("k_ceval_masks", stream, 0);
    return MGR_OK;
}

extern "C" int mgr_ceval_labels(int V, int H, int W, const uint8_t* frame, int row_px, const uint8_t* hand, uint8_t* labels,
                                void* workspace, size_t workspace_bytes, void* stream_) {
    if (int e = ce_check_sizes("mgr_ceval_labels", V, H, W)) return e;
    if (!frame || !labels || !workspace) return mgr_fail(MGR_EINVAL, "mgr_ceval_labels: null pointer");
    if (row_px < W) return mgr_fail(MGR_EINVAL, "mgr_ceval_labels: row_px < W");
    if (!ce_al4(frame)) return mgr_fail(MGR_EINVAL, "mgr_ceval_labels: frame not 4-byte aligned");
    const CeLayout L = ce_layout(V, H, W);
    if (workspace_bytes < L.total) return mgr_fail(MGR_ENOMEM, "mgr_ceval_labels: workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    MGR_HIP(hipMemsetAsync(ws + L.view, 0, (size_t)V * sizeof(CeView), stream));
    const size_t frame_bytes = (size_t)V * H * row_px * 3;
    const dim3 grid((W + CE_LW - 1) / CE_LW, (H + CE_LH - 1) / CE_LH, V);
    const bool vec = (W & 3) == 0 && ce_al4(labels) && (!hand || ce_al4(hand));
    MGR_PROF("k_ceval_labels", stream);
    if (vec)
        hipLaunchKernelGGL(k_ceval_labels<true>, grid, dim3(CE_T), 0, stream, H, W, row_px, frame, frame_bytes, hand, labels,
                           (uint32_t*)(ws + L.occ), (CeView*)(ws + L.view), (uint32_t*)(ws + L.list));
    else
        hipLaunchKernelGGL(k_ceval_labels<false>, grid, dim3(CE_T), 0, stream, H, W, row_px, frame, frame_bytes, hand, labels,
                           (uint32_t*)(ws + L.occ), (CeView*)(ws + L.view), (uint32_t*)(ws + L.list));
    MGR_LAUNCH_CHECK("k_ceval_labels", stream, 0);
    return MGR_OK;
}

extern "C" int mgr_ceval_fill(int V, int H, int W, uint8_t* labels, int32_t* flags, void* workspace, size_t workspace_bytes, void* stream_) {
    if (int e = ce_check_sizes("mgr_ceval_fill", V, H, W)) return e;
    if (!labels || !flags || !workspace) return mgr_fail(MGR_EINVAL, "mgr_ceval_fill: null pointer");
    const CeLayout L = ce_layout(V, H, W);
    if (workspace_bytes < L.total) return mgr_fail(MGR_ENOMEM, "mgr_ceval_fill: workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    MGR_HIP(hipMemsetAsync(flags, 0, (size_t)V * sizeof(int32_t), stream));
    const size_t plane = (size_t)H * W;
    const size_t blocks = (plane + CE_T - 1) / CE_T;
    const dim3 grid((unsigned)(blocks < CE_FILL_BLOCKS ? blocks : CE_FILL_BLOCKS), V);
    MGR_PROF("k_ceval_fill", stream);
    hipLaunchKernelGGL(k_ceval_fill, grid, dim3(CE_T), 0, stream, H, W, (const CeView*)(ws + L.view), (const uint32_t*)(ws + L.occ),
                       (const uint32_t*)(ws + L.list), labels, flags);
    MGR_LAUNCH_CHECK("k_ceval_fill", stream, 0);
    return MGR_OK;
}

extern "C" int mgr_ceval_counts(int V, int H, int W, const uint8_t* pred, const uint8_t* gt, const uint8_t* labels, int64_t* counts,
                                void* workspace, size_t workspace_bytes, void* stream_) {
    if (int e = ce_check_sizes("mgr_ceval_counts", V, H, W)) return e;
    if (!pred || !gt || !labels || !counts || !workspace) return mgr_fail(MGR_EINVAL, "mgr_ceval_counts: null pointer");
    const CeLayout L = ce_layout(V, H, W);
    if (workspace_bytes < L.total) return mgr_fail(MGR_ENOMEM, "mgr_ceval_counts: workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    uint32_t* rec = (uint32_t*)((char*)workspace + L.rec);
    const size_t plane = (size_t)H * W;
    const int nblk = (int)ce_cnt_blocks(H, W);
    const bool vec = (plane & 3) == 0 && ce_al4(pred) && ce_al4(gt) && ce_al4(labels);
    MGR_PROF("k_ceval_counts", stream);      // (with the fold)
    {
        if (vec)
            hipLaunchKernelGGL(k_ceval_counts<true>, dim3(nblk, V), dim3(CE_T), 0, stream, plane, pred, gt, labels, rec);
        else
            hipLaunchKernelGGL(k_ceval_counts<false>, dim3(nblk, V), dim3(CE_T), 0, stream, plane, pred, gt, labels, rec);
    }
    MGR_LAUNCH_CHECK("k_ceval_counts", stream, 0);
    hipLaunchKernelGGL(k_ceval_fold, dim3(V), dim3(CE_FOLD_G * 64), 0, stream, nblk, (const uint32_t*)rec, counts);
    MGR_LAUNCH_CHECK("k_ceval_fold", stream, 0);
    return MGR_OK;
}

extern "C" int mgr_ceval_collage(int V, int H, int W, int M, const uint8_t* gt_rgba, const uint8_t* masks, const uint8_t* table,
                                 uint8_t* out, void* stream_) {
    if (int e = ce_check_sizes("mgr_ceval_collage", V, H, W)) return e;
    if (M < 0 || M > 16) return mgr_fail(MGR_EINVAL, "mgr_ceval_collage: 0 <= M <= 16 masks");
    if (!gt_rgba || (M > 0 && !masks) || !table || !out) return mgr_fail(MGR_EINVAL, "mgr_ceval_collage: null pointer");
    if (!ce_al4(gt_rgba)) return mgr_fail(MGR_EINVAL, "mgr_ceval_collage: gt_rgba not 4-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    const size_t plane = (size_t)H * W;
    MGR_PROF("k_ceval_collage", stream);
    hipLaunchKernelGGL(k_ceval_collage, dim3((unsigned)((plane + CE_T - 1) / CE_T), V), dim3(CE_T), 0, stream, V, H, W, M,
                       (const uint32_t*)gt_rgba, masks, table, out);
    MGR_LAUNCH_CHECK("k_ceval_collage", stream, 0);
    return MGR_OK;
}
