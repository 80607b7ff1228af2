// LPIPS (learned perceptual image patch similarity): the fourth term of the reference's hand loss (lpips.LPIPS(net="vgg"),
// src/modules/base.py:333-341) and the LPIPS-AlexNet column of its validation CSV (src/utils/loss_utils.py:111-117), value and
// gradient w.r.t. the first image in one call (mgr_lpips).
//
//   x' = x * mask (optional)        x'' = 2 x' - 1 (normalize)        in = (x'' - shift) / scale
//   f_k = tap k of the frozen backbone (VGG16: relu1_2 .. relu5_3; AlexNet: its five ReLUs)
//   fh  = f / (sqrt(sum_c f^2) + 1e-10)        s_k = mean_hw sum_c lin_k[c] (fh0 - fh1)^2        d = sum_k s_k
//
// k_lp_conv: implicit-GEMM convolution on v_mfma_f32_32x32x2_f32.  Output channels are the accumulator rows, 32 pixels along x
// the lanes' columns: A = packed weights [k][cout] (k = (ci, ky, kx)), B = the input patch.  A workgroup of four waves takes 64
// output channels x 4 rows x 32 columns; wave w owns row w and two 32x32 accumulators.  Per chunk of input channels the halo
// patch and the weight rows are staged in LDS once and reused by all KH KW taps.  The f32-input MFMA is bit for bit a k-ordered
// fmaf chain: a chunk's sum is that chain from zero, and the chunk sums are added to the bias in chunk order, so an output
// depends on the sizes alone, never on scheduling.  KH, KW, stride, pad, Cin, Cout, H, W are run-time
// arguments (tile edges masked); K3 = true fixes 3x3 stride 1 pad 1 at compile time.  `gate` (same shape as the input) zeroes
// the staged input where gate <= 0: the data gradient dX = conv(dY * [y > 0], W') runs on the same kernel with the flipped,
// transposed weights W' that mgr_lpips_net_pack prepares.  The weights are frozen: there is no weight gradient.
//
// k_lp_conv16 (operands = MGR_LPIPS_BF16): the same workgroup tile and epilogue on v_mfma_f32_32x32x16_bf16.  The two MFMA
// operands -- the staged input AFTER the gate and the halo zeroing, and the weight -- are rounded to bf16 (round to nearest
// even) and the products are summed in fp32.  k is ordered (tap, input channel): the patch is staged as bf16
// [py][px][channel], the weights are pre-packed by k_lp_pack16 as bf16 [tap][channel / 8][cout][8], so every fragment is one
// 16-byte LDS read.  Bias, ReLU, the stored fp32 activations and everything outside the convolutions are as in fp32 mode.
// The summation order inside a bf16 MFMA is the hardware's: there is no k-ordered chain, but still no atomics, and an output
// depends on the sizes alone.  The chunk sums are blocked as above.
//
// Windows (mgr_lpips_roi_op): the chain runs on the contiguous (3,h,w) copy of a per-view rectangle of the (3,H,W) frame.  Only the
// scaling kernels know about the frame: k_lp_scale_win reads the rectangle of the pitched frame (and mask), k_lp_scale_bwd_win
// adds the gradient into the rectangle, or writes the whole frame with zeros outside it; the arithmetic per element is
// k_lp_scale's, so a window is the call on .contiguous() crops bit for bit -- the crop's own zero padding and spatial means, not
// the full-frame value restricted to a region.  mgr_lpips_roi_taps_op leaves the target tower's five taps of a window in a
// caller's buffer; a call given it skips that tower (same kernels, same bits).
//
// Batches (mgr_lpips_roi_batch_op, mgr_lpips_roi_taps_batch_op): the views of a call that share a window size run as chunks of at
// most LP_MAX_BATCH views, one chain of launches per chunk, on a workspace with every region G times as long, batch-major.  The
// convolutions carry (batch, output-channel block) in blockIdx.z and offset x / gate / y by their own Cin H W and Cout Ho Wo;
// pools run on G C channels; the scaling kernels take a per-launch table of (view, x0, y0), the head per-view target pointers
// and scales, the fold one workgroup per view.  No sum changes: a batched call is the sequential call bit for bit, and every
// other call of this file is the batch of one view.
//
// Storage (the *_st entries with storage = MGR_LPIPS_STORE_BF16, bf16 operands only): every tensor of the chain -- pred's
// convolution outputs, the target's taps and non-tap outputs, the pool outputs, every gradient buffer -- is bf16 in the
// channel-blocked layout [ceil(C / 8)][h][w][8]: 16 bytes per (pixel, block of 8 channels), channel c at block c / 8, lane
// c % 8, pad lanes written as zero so that readers load unconditionally; view b of a batch-major buffer sits at b times the
// bytes of one view.  The image-side pair stays (3,h,w) fp32 planar -- the scaled image and layer 0's data gradient -- so the
// scaling kernels and the window semantics are untouched.  A convolution keeps its chunking, MFMA sequence, fp32 accumulation,
// fp32 bias and ReLU and rounds ONCE (to nearest even) at the store; a stored value is the next MFMA's operand as it is (the
// operand mode would have rounded the fp32 value to the same bits at the load), and the gate is `stored value > 0`.  A pool is
// the maximum of the stored values (exact), the winner the FIRST maximum in row-major window order among the STORED values,
// forward and backward: ties that the rounding creates go to the first position.  A head reads the taps exactly (bf16 ->
// fp32), computes as in fp32 storage, and rounds its gradient once at the store; with add = 1 it forms fp32(stored g) + t and
// rounds once.  The fold and the fp64 partials are unchanged.  No atomics; everything said of views, batches, windows and
// d(x, x) = 0 above and below holds in this mode too.
//
// Spatial means travel as fp64 partials over a fixed tree (as k_map_loss does); no float atomics anywhere: bit-reproducible.
//
// One deviation from autograd: where a pixel's tap features are all zero, autograd through sqrt yields 0 * inf = NaN; here
// that pixel contributes a zero gradient (the skip rule of a zero skin-weight sum, include/manus_hip.h).
#include "mgr_common.h"

#include <vector>

typedef float lp_f16v __attribute__((ext_vector_type(16)));
typedef __bf16 lp_bf8 __attribute__((ext_vector_type(8)));
typedef __bf16 lp_bf4 __attribute__((ext_vector_type(4)));
typedef unsigned short lp_us8 __attribute__((ext_vector_type(8)));      // the bits of one (pixel, channel block) of bf16 storage

#define LP_T 256           // threads of every kernel of this file
#define LP_TW 32           // output columns per workgroup of k_lp_conv (the MFMA's columns)
#define LP_TH 4            // output rows per workgroup (one per wave)
#define LP_TC 64           // output channels per workgroup (two MFMA row blocks)
#define LP_LDS_BUDGET (64 * 1024)
#define LP_MAX_CK 8
#define LP16_CK 32         // input channels per chunk of k_lp_conv16 (a multiple of 8)
#define LP16_XPAD 16       // bytes of padding per staged pixel of k_lp_conv16: 80- / 48-byte pixels are conflict-free for 16-byte reads
#define LP_NTAP 5
#define LP_MAX_OPS 20

// ---------------------------------------------------------------------------
// the two networks, as a host table
// ---------------------------------------------------------------------------
struct LpOp {
    int conv;                 // 1: convolution + ReLU, 0: max-pool
    int cin, cout, k, s, p;
    int tap;                  // index of the tap this convolution's output is, or -1
};

static const LpOp LP_VGG[] = {
    {1, 3, 64, 3, 1, 1, -1},    {1, 64, 64, 3, 1, 1, 0},    {0, 64, 64, 2, 2, 0, -1},   {1, 64, 128, 3, 1, 1, -1},
    {1, 128, 128, 3, 1, 1, 1},  {0, 128, 128, 2, 2, 0, -1}, {1, 128, 256, 3, 1, 1, -1}, {1, 256, 256, 3, 1, 1, -1},
    {1, 256, 256, 3, 1, 1, 2},  {0, 256, 256, 2, 2, 0, -1}, {1, 256, 512, 3, 1, 1, -1}, {1, 512, 512, 3, 1, 1, -1},
    {1, 512, 512, 3, 1, 1, 3},  {0, 512, 512, 2, 2, 0, -1}, {1, 512, 512, 3, 1, 1, -1}, {1, 512, 512, 3, 1, 1, -1},
    {1, 512, 512, 3, 1, 1, 4}};
static const LpOp LP_ALEX[] = {{1, 3, 64, 11, 4, 2, 0},   {0, 64, 64, 3, 2, 0, -1},  {1, 64, 192, 5, 1, 2, 1}, {0, 192, 192, 3, 2, 0, -1},
                               {1, 192, 384, 3, 1, 1, 2}, {1, 384, 256, 3, 1, 1, 3}, {1, 256, 256, 3, 1, 1, 4}};

struct LpNet {
    const LpOp* ops;
    int n_ops, n_conv;
    bool has_bwd;
};

static bool lp_net(int net, LpNet* n) {
    if (net == 0) {
        *n = {LP_VGG, (int)(sizeof(LP_VGG) / sizeof(LpOp)), 13, true};
        return true;
    }
    if (net == 1) {
        *n = {LP_ALEX, (int)(sizeof(LP_ALEX) / sizeof(LpOp)), 5, false};
        return true;
    }
    return false;
}

static inline size_t lp_pad64(size_t c) { return (c + 63) & ~(size_t)63; }
static inline size_t lp_pad8(size_t c) { return (c + 7) & ~(size_t)7; }
static inline bool lp_operands_ok(int operands) { return operands == MGR_LPIPS_F32 || operands == MGR_LPIPS_BF16; }
static inline bool lp_storage_ok(int storage) { return storage == MGR_LPIPS_STORE_F32 || storage == MGR_LPIPS_STORE_BF16; }
// bytes of a (C, h, w) tensor of the chain: fp32 planar, or bf16 [pad8(C) / 8][h][w][8]
static inline size_t lp_tbytes(int storage, size_t C, size_t h, size_t w) {
    return storage == MGR_LPIPS_STORE_BF16 ? lp_pad8(C) * h * w * 2 : C * h * w * 4;
}
// bytes of one packed weight set: fp32 [K][pad64(Cout)], bf16 [taps][pad8(Cin) / 8][pad64(Cout)][8]
static inline size_t lp_wbytes(int operands, size_t cin, size_t kk, size_t cout) {
    return operands == MGR_LPIPS_BF16 ? kk * lp_pad8(cin) * lp_pad64(cout) * 2 : cin * kk * lp_pad64(cout) * 4;
}

// the packed blob: per convolution [K][pad64(Cout)] forward weights, [pad64(Cout)] bias, (VGG) [Cout KH KW][pad64(Cin)] data-gradient
// weights; then the five lin vectors.  In bf16 mode the two weight sets are bf16 in k_lp_pack16's layout, the rest is fp32.
struct LpBlob {
    size_t w[13], b[13], wt[13], lin[LP_NTAP], total;
};

static LpBlob lp_blob(const LpNet& n, int operands) {
    LpBlob B;
    size_t o = 0;
    int ci = 0;
    for (int i = 0; i < n.n_ops; ++i) {
        const LpOp& op = n.ops[i];
        if (!op.conv) continue;
        const size_t kk = (size_t)op.k * op.k;
        B.w[ci] = o;  o += mgr_align(lp_wbytes(operands, op.cin, kk, op.cout));
        B.b[ci] = o;  o += mgr_align(lp_pad64(op.cout) * 4);
        B.wt[ci] = o;
        if (n.has_bwd) o += mgr_align(lp_wbytes(operands, op.cout, kk, op.cin));
        if (op.tap >= 0) { B.lin[op.tap] = o;  o += mgr_align((size_t)op.cout * 4); }
        ++ci;
    }
    B.total = o;
    return B;
}

// sizes of every op's output; false where some output has no pixel
struct LpShape {
    int h[LP_MAX_OPS], w[LP_MAX_OPS];
};

static bool lp_shapes(const LpNet& n, int H, int W, LpShape* S) {
    int h = H, w = W;
    for (int i = 0; i < n.n_ops; ++i) {
        const LpOp& op = n.ops[i];
        if (h + 2 * op.p < op.k || w + 2 * op.p < op.k) return false;
        h = (h + 2 * op.p - op.k) / op.s + 1;
        w = (w + 2 * op.p - op.k) / op.s + 1;
        if (h < 1 || w < 1) return false;
        S->h[i] = h;
        S->w[i] = w;
    }
    return true;
}

// workspace: [pred's convolution outputs, in layer order][target's five taps][scratch A][scratch B][fp64 partials]
// A chunk of G equal-size views (the batched entries) has every region G times as long, batch-major: view b of a buffer of e
// bytes sits at b e, view b's partials at b part_off[LP_NTAP].  G = 1 is the one-view layout.  Sizes are lp_tbytes of the
// storage; the scaled image and layer 0's data gradient, which the scratch holds too, are fp32 in both.
struct LpLayout {
    size_t act[13], tap[LP_NTAP], bufa, bufb, part, total;
    size_t part_off[LP_NTAP + 1];      // in doubles: the slots of tap k are [part_off[k], part_off[k + 1])
};

static bool lp_layout(const LpNet& n, int H, int W, int need_grad, LpLayout* L, size_t G = 1, int st = MGR_LPIPS_STORE_F32) {
    LpShape S;
    if (H < 1 || W < 1 || (long long)H * W > (1ll << 24) || !lp_shapes(n, H, W, &S)) return false;
    // scratch B takes the scaled image (fp32 in both storages), so it is never smaller than one; in bf16 storage without a
    // gradient scratch A holds blocked tensors only and is sized by them alone
    const size_t img = (size_t)3 * H * W * 4;
    size_t o = 0, scratch = st == MGR_LPIPS_STORE_BF16 && !need_grad ? 0 : img;
    int ci = 0;
    for (int i = 0; i < n.n_ops; ++i) {
        const LpOp& op = n.ops[i];
        const size_t e = lp_tbytes(st, op.cout, S.h[i], S.w[i]);
        // scratch holds: the scaled image, every pool output, the target's convolution outputs that are no tap, and (with a
        // gradient) the gradient w.r.t. any of them
        if (!op.conv || op.tap < 0 || need_grad) scratch = scratch > e ? scratch : e;
        if (op.conv) { L->act[ci++] = o;  o += mgr_align(G * e); }
    }
    for (int i = 0; i < n.n_ops; ++i) {
        const LpOp& op = n.ops[i];
        if (op.conv && op.tap >= 0) {
            L->tap[op.tap] = o;  o += mgr_align(G * lp_tbytes(st, op.cout, S.h[i], S.w[i]));
            L->part_off[op.tap + 1] = ((size_t)S.h[i] * S.w[i] + LP_T - 1) / LP_T;
        }
    }
    L->part_off[0] = 0;
    for (int k = 0; k < LP_NTAP; ++k) L->part_off[k + 1] += L->part_off[k];
    L->bufa = o;  o += mgr_align(G * scratch);
    L->bufb = o;  o += mgr_align(G * (scratch > img ? scratch : img));
    L->part = o;  o += mgr_align(G * L->part_off[LP_NTAP] * 8);
    L->total = o;
    return true;
}

// ---------------------------------------------------------------------------
// weight packing
// ---------------------------------------------------------------------------
// w: torch's [Cout][Cin][KH][KW].  fwd[(ci KK + t) CoP + co] = w[co][ci][t]; bwd[(co KK + (KK - 1 - t)) CiP + ci] = w[co][ci][t]
// (the 180-degree flip of a square kernel is t -> KK - 1 - t); the padding columns are zero.
__global__ __launch_bounds__(LP_T) void k_lp_pack(int Cout, int Cin, int KK, int CoP, int CiP, const float* __restrict__ w,
                                                  const float* __restrict__ bias, float* __restrict__ fwd, float* __restrict__ bp,
                                                  float* __restrict__ bwd) {
    const size_t nf = (size_t)Cin * KK * CoP, nb = bwd ? (size_t)Cout * KK * CiP : 0;
    const size_t stride = (size_t)gridDim.x * LP_T;
    for (size_t e = (size_t)blockIdx.x * LP_T + threadIdx.x; e < nf; e += stride) {
        const int co = (int)(e % CoP);
        const size_t r = e / CoP;      // ci KK + t
        fwd[e] = co < Cout ? w[(size_t)co * Cin * KK + r] : 0.f;
    }
    for (size_t e = (size_t)blockIdx.x * LP_T + threadIdx.x; e < nb; e += stride) {
        const int ci = (int)(e % CiP);
        const size_t r = e / CiP;
        const int co = (int)(r / KK), t = KK - 1 - (int)(r % KK);
        bwd[e] = ci < Cin ? w[((size_t)co * Cin + ci) * KK + t] : 0.f;
    }
    for (size_t e = (size_t)blockIdx.x * LP_T + threadIdx.x; e < (size_t)CoP; e += stride) bp[e] = e < (size_t)Cout ? bias[e] : 0.f;
}

__global__ __launch_bounds__(LP_T) void k_lp_copy(int n, const float* __restrict__ src, float* __restrict__ dst) {
    const int e = blockIdx.x * LP_T + threadIdx.x;
    if (e < n) dst[e] = src[e];
}

// ---------------------------------------------------------------------------
// convolution
// ---------------------------------------------------------------------------
// blockIdx.z = batch NZ + (block of 64 output channels); view b's x / gate sit at b Cin H W, its y at b Cout Ho Wo
struct LpConvArgs {
    int Cin, Cout, CoP, H, W, Ho, Wo, KH, KW, stride, pad, CK, relu, NZ;
    const float *x, *gate, *wp, *bias;
    float* y;
};

template <bool K3>
__global__ __launch_bounds__(LP_T) void k_lp_conv(const LpConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lp_smem[];
    const int KH = K3 ? 3 : a.KH, KW = K3 ? 3 : a.KW, st = K3 ? 1 : a.stride, pad = K3 ? 1 : a.pad;
    const int KK = KH * KW;
    const int PH = (LP_TH - 1) * st + KH, PW = (LP_TW - 1) * st + KW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    const int zb = blockIdx.z / a.NZ;
    const int ox0 = blockIdx.x * LP_TW, oy0 = blockIdx.y * LP_TH, co0 = (blockIdx.z - zb * a.NZ) * LP_TC;
    const int ix0 = ox0 * st - pad, iy0 = oy0 * st - pad;
    const bool two = a.Cout - co0 > 32;           // the second block of 32 output channels holds any (workgroup-uniform)
    const size_t xoff = (size_t)zb * a.Cin * a.H * a.W;
    const float* ax = a.x + xoff;
    const float* agate = a.gate ? a.gate + xoff : nullptr;
    float* ay = a.y + (size_t)zb * a.Cout * a.Ho * a.Wo;
    float* sW = lp_smem;                                     // [2 ceil(CK KK / 2)][64]
    float* sX = lp_smem + (size_t)((a.CK * KK + 1) & ~1) * LP_TC;      // [CK][PH][PW]

    lp_f16v acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
        acc0[r] = a.bias ? a.bias[co0 + row] : 0.f;
        acc1[r] = a.bias ? a.bias[co0 + 32 + row] : 0.f;       // (the bias is padded to CoP, a multiple of 64)
    }

    for (int ci0 = 0; ci0 < a.Cin; ci0 += a.CK) {
        const int ckn = min(a.CK, a.Cin - ci0), Kc = ckn * KK, Kce = (Kc + 1) & ~1;
        // the weight rows of this chunk, [k][64 output channels]; an odd tail row is zero
        for (int e = tid; e < Kce * LP_TC; e += LP_T) {
            const int kk = e >> 6, c = e & 63;
            sW[e] = kk < Kc ? a.wp[((size_t)ci0 * KK + kk) * a.CoP + co0 + c] : 0.f;
        }
        // the halo patch, zero outside the image and where the gate is not positive
        const int pn = ckn * PH * PW;
        for (int e = tid; e < pn; e += LP_T) {
            const int px = e % PW, q = e / PW, py = q % PH, ci = q / PH;
            const int ix = ix0 + px, iy = iy0 + py;
            float v = 0.f;
            if (ix >= 0 && ix < a.W && iy >= 0 && iy < a.H) {
                const size_t g = ((size_t)(ci0 + ci) * a.H + iy) * a.W + ix;
                v = ax[g];
                if (agate && !(agate[g] > 0.f)) v = 0.f;
            }
            sX[e] = v;
        }
        __syncthreads();
        // lanes 0-31 take k = 2 j, lanes 32-63 k = 2 j + 1; (ci, ky, kx) advance by two taps per step
        int kx = half, ky = 0, ci = 0;
        while (kx >= KW) { kx -= KW; ++ky; }
        while (ky >= KH) { ky -= KH; ++ci; }
        const float* xrow = sX + (wave * st) * PW + col * st;
        // the chunk's own sum starts at zero and is added to the total once: a blocked sum, whose rounding error grows with
        // the chunk length plus the number of chunks instead of with Cin KH KW (4608 terms in VGG's deepest layers)
        lp_f16v c0, c1;
#pragma unroll
        for (int r = 0; r < 16; ++r) c0[r] = c1[r] = 0.f;
        for (int kk = half; kk < Kce; kk += 2) {
            const float b = ci < ckn ? xrow[(ci * PH + ky) * PW + kx] : 0.f;
            const float w0 = sW[kk * LP_TC + col];
            c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(w0, b, c0, 0, 0, 0);
            if (two) {
                const float w1 = sW[kk * LP_TC + 32 + col];
                c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w1, b, c1, 0, 0, 0);
            }
            kx += 2;
            while (kx >= KW) { kx -= KW; ++ky; }
            while (ky >= KH) { ky -= KH; ++ci; }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc0[r] += c0[r];
            acc1[r] += c1[r];
        }
        __syncthreads();
    }

    const int ox = ox0 + col, oy = oy0 + wave;
    if (ox < a.Wo && oy < a.Ho) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
            const int c0 = co0 + row, c1 = c0 + 32;
            float v0 = acc0[r], v1 = acc1[r];
            if (a.relu) {
                v0 = v0 < 0.f ? 0.f : v0;
                v1 = v1 < 0.f ? 0.f : v1;
            }
            if (c0 < a.Cout) ay[((size_t)c0 * a.Ho + oy) * a.Wo + ox] = v0;
            if (two && c1 < a.Cout) ay[((size_t)c1 * a.Ho + oy) * a.Wo + ox] = v1;
        }
    }
}

static int lp_conv_ck(int Cin, int KH, int KW, int stride, size_t* lds) {
    const size_t PH = (size_t)(LP_TH - 1) * stride + KH, PW = (size_t)(LP_TW - 1) * stride + KW, KK = (size_t)KH * KW;
    int ck = Cin < LP_MAX_CK ? Cin : LP_MAX_CK;
    for (;; --ck) {
        *lds = ((((size_t)ck * KK + 1) & ~(size_t)1) * LP_TC + (size_t)ck * PH * PW) * 4;
        if (*lds <= LP_LDS_BUDGET || ck == 1) break;
    }
    return ck;
}

// y (Cout, Ho, Wo) = [relu](conv(x * [gate > 0], w) + bias); wp: [Cin KH KW][CoP] packed, bias: [CoP] or null
static int lp_conv(hipStream_t stream, const char* name, int G, int Cin, int Cout, int H, int W, int KH, int KW, int stride, int pad,
                   const float* x, const float* gate, const float* wp, const float* bias, int relu, float* y) {
    LpConvArgs a;
    a.Cin = Cin; a.Cout = Cout; a.CoP = (int)lp_pad64(Cout); a.H = H; a.W = W;
    a.Ho = (H + 2 * pad - KH) / stride + 1; a.Wo = (W + 2 * pad - KW) / stride + 1;
    a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad; a.relu = relu;
    a.x = x; a.gate = gate; a.wp = wp; a.bias = bias; a.y = y;
    size_t lds;
    a.CK = lp_conv_ck(Cin, KH, KW, stride, &lds);
    if (lds > 150 * 1024) return mgr_fail(MGR_EINVAL, "k_lp_conv: kernel window too large for LDS");
    a.NZ = (Cout + LP_TC - 1) / LP_TC;
    const dim3 grid((a.Wo + LP_TW - 1) / LP_TW, (a.Ho + LP_TH - 1) / LP_TH, (unsigned)(G * a.NZ));
    if (grid.y > 65535u || grid.z > 65535u) return mgr_fail(MGR_EINVAL, "k_lp_conv: image too large");
    MGR_PROF(name, stream);
    if (KH == 3 && KW == 3 && stride == 1 && pad == 1) {
        hipLaunchKernelGGL(k_lp_conv<true>, grid, dim3(LP_T), lds, stream, a);
    } else {
        if (lds > 64 * 1024) {
            static bool raised = false;
            if (!raised) {
                MGR_HIP(hipFuncSetAttribute((const void*)k_lp_conv<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
                raised = true;
            }
        }
        hipLaunchKernelGGL(k_lp_conv<false>, grid, dim3(LP_T), lds, stream, a);
    }
    MGR_LAUNCH_CHECK(name, stream, 0);
    return MGR_OK;
}

// ---------------------------------------------------------------------------
// convolution with bf16 operands
// ---------------------------------------------------------------------------
// w: torch's [Cout][Cin][KH][KW].  With NBi = pad8(Cin) / 8, NBo = pad8(Cout) / 8:
//   fwd[((t NBi + ci / 8) CoP + co) 8 + ci % 8] = bf16(w[co][ci][t])
//   bwd[((t NBo + co / 8) CiP + ci) 8 + co % 8] = bf16(w[co][ci][KK - 1 - t])        (the layer used backwards: k runs over co)
// zero wherever ci >= Cin or co >= Cout; the bias stays fp32.
__global__ __launch_bounds__(LP_T) void k_lp_pack16(int Cout, int Cin, int KK, int CoP, int CiP, const float* __restrict__ w,
                                                    const float* __restrict__ bias, __bf16* __restrict__ fwd, float* __restrict__ bp,
                                                    __bf16* __restrict__ bwd) {
    const int NBi = (Cin + 7) >> 3, NBo = (Cout + 7) >> 3;
    const size_t nf = (size_t)KK * NBi * CoP * 8, nb = bwd ? (size_t)KK * NBo * CiP * 8 : 0;
    const size_t stride = (size_t)gridDim.x * LP_T;
    for (size_t e = (size_t)blockIdx.x * LP_T + threadIdx.x; e < nf; e += stride) {
        const int j = (int)(e & 7), co = (int)((e >> 3) % CoP);
        const size_t r = (e >> 3) / CoP;      // t NBi + ci / 8
        const int ci = (int)(r % NBi) * 8 + j, t = (int)(r / NBi);
        fwd[e] = (__bf16)(co < Cout && ci < Cin ? w[((size_t)co * Cin + ci) * KK + t] : 0.f);
    }
    for (size_t e = (size_t)blockIdx.x * LP_T + threadIdx.x; e < nb; e += stride) {
        const int j = (int)(e & 7), ci = (int)((e >> 3) % CiP);
        const size_t r = (e >> 3) / CiP;
        const int co = (int)(r % NBo) * 8 + j, t = KK - 1 - (int)(r / NBo);
        bwd[e] = (__bf16)(co < Cout && ci < Cin ? w[((size_t)co * Cin + ci) * KK + t] : 0.f);
    }
    for (size_t e = (size_t)blockIdx.x * LP_T + threadIdx.x; e < (size_t)CoP; e += stride) bp[e] = e < (size_t)Cout ? bias[e] : 0.f;
}

// x / gate and y are fp32 planar or bf16 blocked, by the kernel's template arguments
struct LpConv16Args {
    int Cin, Cout, CoP, NB, H, W, Ho, Wo, KH, KW, stride, pad, CK, KYN, relu, NZ;       // NB = pad8(Cin) / 8; NZ as in LpConvArgs
    const void *x, *gate;
    const float* bias;
    const lp_bf8* wp;
    void* y;
};

// one (pixel, channel block) of bf16 storage, zeroed where the gate's stored value is not positive
__device__ __forceinline__ lp_us8 lp_gate8(lp_us8 v, lp_us8 g) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (!(__uint_as_float((unsigned)g[j] << 16) > 0.f)) v[j] = 0;
    return v;
}

// A chunk is CK input channels (a multiple of 8) times KYN kernel rows (all of them for 3x3).  Its k runs over q = (tap, block
// of 8 channels); one MFMA takes q = 2 m (lanes 0-31) and q = 2 m + 1 (lanes 32-63), an odd tail is zero.
// XB: x and gate are bf16 blocked -- a staged (pixel, channel block) is one 16-byte global load, the gate block a second, the
// select is done in registers and nothing is converted.  YB: y is bf16 blocked -- the ONE rounding of the storage mode; a
// lane's four consecutive rows of an accumulator are half a (pixel, block), the two halves of a wave interleave to full pixels.
template <bool K3, bool XB, bool YB>
__global__ __launch_bounds__(LP_T) void k_lp_conv16(const LpConv16Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lp_smem16[];
    const int KH = K3 ? 3 : a.KH, KW = K3 ? 3 : a.KW, st = K3 ? 1 : a.stride, pad = K3 ? 1 : a.pad, KYN = K3 ? 3 : a.KYN;
    const int PW = (LP_TW - 1) * st + KW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 31, half = lane >> 5;
    const int zb = blockIdx.z / a.NZ;
    const int ox0 = blockIdx.x * LP_TW, oy0 = blockIdx.y * LP_TH, co0 = (blockIdx.z - zb * a.NZ) * LP_TC;
    const int ix0 = ox0 * st - pad, iy0 = oy0 * st - pad;
    const bool two = a.Cout - co0 > 32;
    const size_t xoff = (size_t)zb * a.Cin * a.H * a.W;
    const float* ax = (const float*)a.x + xoff;
    const float* agate = a.gate ? (const float*)a.gate + xoff : nullptr;
    float* ay = (float*)a.y + (size_t)zb * a.Cout * a.Ho * a.Wo;
    // the blocked views of the same buffers: [NB][H][W] and [pad8(Cout) / 8][Ho][Wo] of 16 bytes
    const size_t xboff = (size_t)zb * a.NB * a.H * a.W;
    const lp_us8* bx = (const lp_us8*)a.x + xboff;
    const lp_us8* bgate = a.gate ? (const lp_us8*)a.gate + xboff : nullptr;
    const int NBo = (a.Cout + 7) >> 3;
    lp_bf4* by = (lp_bf4*)a.y + (size_t)zb * NBo * a.Ho * a.Wo * 2;
    const int XS = a.CK * 2 + LP16_XPAD;                      // bytes per staged pixel
    lp_bf8* sW = (lp_bf8*)lp_smem16;                          // [q][64 output channels] of 8 bf16
    unsigned char* sX = lp_smem16 + (size_t)KYN * KW * (a.CK >> 3) * LP_TC * 16;       // [py][px] of XS bytes: CK bf16, padding

    lp_f16v acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
        acc0[r] = a.bias ? a.bias[co0 + row] : 0.f;
        acc1[r] = a.bias ? a.bias[co0 + 32 + row] : 0.f;
    }
    lp_bf8 zero;
#pragma unroll
    for (int j = 0; j < 8; ++j) zero[j] = (__bf16)0.f;

    for (int ci0 = 0; ci0 < 8 * a.NB; ci0 += a.CK) {
        const int nb = min(a.CK, 8 * a.NB - ci0) >> 3;
        for (int ky0 = 0; ky0 < KH; ky0 += KYN) {
            const int kyn = min(KYN, KH - ky0), Q = kyn * KW * nb, PH = (LP_TH - 1) * st + kyn;
            if (K3 && nb == 4) {
                // the hot shape: fixed trip counts and unconditional loads from clamped addresses, so that all loads of a
                // chunk are in flight together instead of one latency per iteration
#pragma unroll
                for (int it = 0; it < 9; ++it) {
                    const int e = tid + it * LP_T, c = e & 63, q = e >> 6;        // q = 4 t + cb
                    sW[e] = a.wp[((size_t)(q >> 2) * a.NB + (ci0 >> 3) + (q & 3)) * a.CoP + co0 + c];
                }
                constexpr int NP = (LP_TH + 2) * (LP_TW + 2);
#pragma unroll
                for (int it = 0; it < (4 * NP + LP_T - 1) / LP_T; ++it) {
                    const int e = tid + it * LP_T, cb = e / NP, p = e - cb * NP, py = p / (LP_TW + 2), px = p - py * (LP_TW + 2);
                    const int ix = ix0 + px, iy = iy0 + py;
                    const bool in = ix >= 0 && ix < a.W && iy >= 0 && iy < a.H;
                    const size_t gp = (size_t)min(max(iy, 0), a.H - 1) * a.W + min(max(ix, 0), a.W - 1);
                    if (XB) {
                        // (the tail iteration's cb runs past the chunk: its address is clamped, its value dropped)
                        const size_t g = (size_t)min((ci0 >> 3) + cb, a.NB - 1) * a.H * a.W + gp;
                        lp_us8 v = bx[g];
                        if (bgate) v = lp_gate8(v, bgate[g]);
                        if (!in) v = (lp_us8)(0);
                        if (e < 4 * NP) *(lp_us8*)(sX + p * (LP16_CK * 2 + LP16_XPAD) + cb * 16) = v;
                    } else {
                        float f[8], gt[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const size_t g = (size_t)min(ci0 + cb * 8 + j, a.Cin - 1) * a.H * a.W + gp;
                            f[j] = ax[g];
                            gt[j] = agate ? agate[g] : 1.f;
                        }
                        lp_bf8 v;
#pragma unroll
                        for (int j = 0; j < 8; ++j) v[j] = (__bf16)(in && ci0 + cb * 8 + j < a.Cin && gt[j] > 0.f ? f[j] : 0.f);
                        if (e < 4 * NP) *(lp_bf8*)(sX + p * (LP16_CK * 2 + LP16_XPAD) + cb * 16) = v;
                    }
                }
            } else {
                for (int e = tid; e < Q * LP_TC; e += LP_T) {
                    const int c = e & 63, q = e >> 6, t = q / nb, cb = q - t * nb;
                    sW[e] = a.wp[((size_t)(ky0 * KW + t) * a.NB + (ci0 >> 3) + cb) * a.CoP + co0 + c];
                }
                // the halo patch of kernel rows [ky0, ky0 + kyn): gated, zero outside the image and past Cin, THEN rounded
                const int np = PH * PW;
                for (int e = tid; e < nb * np; e += LP_T) {
                    const int cb = e / np, p = e - cb * np, py = p / PW, px = p - py * PW;
                    const int ix = ix0 + px, iy = iy0 + ky0 + py;
                    const bool in = ix >= 0 && ix < a.W && iy >= 0 && iy < a.H;
                    if (XB) {
                        // (ci0 / 8 + cb < NB: the chunk's blocks exist, their pad lanes are stored zeros)
                        lp_us8 v = (lp_us8)(0);
                        if (in) {
                            const size_t g = ((size_t)((ci0 >> 3) + cb) * a.H + iy) * a.W + ix;
                            v = bx[g];
                            if (bgate) v = lp_gate8(v, bgate[g]);
                        }
                        *(lp_us8*)(sX + p * XS + cb * 16) = v;
                        continue;
                    }
                    lp_bf8 v;
    #pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int c = ci0 + cb * 8 + j;
                        float f = 0.f;
                        if (in && c < a.Cin) {
                            const size_t g = ((size_t)c * a.H + iy) * a.W + ix;
                            f = ax[g];
                            if (agate && !(agate[g] > 0.f)) f = 0.f;
                        }
                        v[j] = (__bf16)f;
                    }
                    *(lp_bf8*)(sX + p * XS + cb * 16) = v;
                }
            }
            __syncthreads();
            const unsigned char* xl = sX + ((wave * st) * PW + col * st) * XS;
            lp_f16v c0, c1;
#pragma unroll
            for (int r = 0; r < 16; ++r) c0[r] = c1[r] = 0.f;
            if (K3 && nb == 4) {
                // the hot shape: 32 channels, 9 taps, every offset a constant
#pragma unroll
                for (int t = 0; t < 9; ++t) {
#pragma unroll
                    for (int pp = 0; pp < 2; ++pp) {
                        const int cb = 2 * pp + half;
                        const lp_bf8 b = *(const lp_bf8*)(xl + ((t / 3) * (LP_TW + 2) + t % 3) * (LP16_CK * 2 + LP16_XPAD) + cb * 16);
                        c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sW[(t * 4 + cb) * LP_TC + col], b, c0, 0, 0, 0);
                        if (two) c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(sW[(t * 4 + cb) * LP_TC + 32 + col], b, c1, 0, 0, 0);
                    }
                }
            } else {
                int cb = half, kx = 0, ky = 0;
                while (cb >= nb) { cb -= nb;  if (++kx == KW) { kx = 0; ++ky; } }
                for (int q = half; q < Q + half; q += 2) {
                    lp_bf8 b = zero, w0 = zero, w1 = zero;
                    if (q < Q) {
                        b = *(const lp_bf8*)(xl + (ky * PW + kx) * XS + cb * 16);
                        w0 = sW[q * LP_TC + col];
                        if (two) w1 = sW[q * LP_TC + 32 + col];
                    }
                    c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w0, b, c0, 0, 0, 0);
                    if (two) c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, b, c1, 0, 0, 0);
                    cb += 2;
                    while (cb >= nb) { cb -= nb;  if (++kx == KW) { kx = 0; ++ky; } }
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc0[r] += c0[r];
                acc1[r] += c1[r];
            }
            __syncthreads();
        }
    }

    const int ox = ox0 + col, oy = oy0 + wave;
    if (YB) {
        if (ox < a.Wo && oy < a.Ho) {
            // rows (r & 3) + 8 q + 4 half, r = 4 q .. 4 q + 3: lanes 4 half .. 4 half + 3 of block co0 / 8 + q (+ 4 for acc1);
            // a block that exists is written whole, its channels past Cout as zero
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                lp_bf4 v0, v1;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c0 = co0 + 8 * q + 4 * half + j;
                    float f0 = acc0[4 * q + j], f1 = acc1[4 * q + j];
                    if (a.relu) {
                        f0 = f0 < 0.f ? 0.f : f0;
                        f1 = f1 < 0.f ? 0.f : f1;
                    }
                    v0[j] = (__bf16)(c0 < a.Cout ? f0 : 0.f);
                    v1[j] = (__bf16)(c0 + 32 < a.Cout ? f1 : 0.f);
                }
                const int b0 = (co0 >> 3) + q, b1 = b0 + 4;
                if (b0 < NBo) by[(((size_t)b0 * a.Ho + oy) * a.Wo + ox) * 2 + half] = v0;
                if (two && b1 < NBo) by[(((size_t)b1 * a.Ho + oy) * a.Wo + ox) * 2 + half] = v1;
            }
        }
        return;
    }
    if (ox < a.Wo && oy < a.Ho) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
            const int c0 = co0 + row, c1 = c0 + 32;
            float v0 = acc0[r], v1 = acc1[r];
            if (a.relu) {
                v0 = v0 < 0.f ? 0.f : v0;
                v1 = v1 < 0.f ? 0.f : v1;
            }
            if (c0 < a.Cout) ay[((size_t)c0 * a.Ho + oy) * a.Wo + ox] = v0;
            if (two && c1 < a.Cout) ay[((size_t)c1 * a.Ho + oy) * a.Wo + ox] = v1;
        }
    }
}

static size_t lp_conv16_lds(int ck, int kyn, int KW, int stride) {
    const size_t PH = (size_t)(LP_TH - 1) * stride + kyn, PW = (size_t)(LP_TW - 1) * stride + KW;
    return (size_t)kyn * KW * (ck >> 3) * LP_TC * 16 + PH * PW * (ck * 2 + LP16_XPAD);
}

// the chunk: the most channels (32, 16, 8) and then the most kernel rows that fit the LDS budget; 8 channels of one row if none does
static void lp_conv16_chunk(int Cin, int KH, int KW, int stride, int* ck, int* kyn, size_t* lds) {
    const int cmax = (int)lp_pad8(Cin) < LP16_CK ? (int)lp_pad8(Cin) : LP16_CK;
    for (int c = cmax; c >= 8; c = c > 16 ? 16 : c - 8)
        for (int r = KH; r >= 1; --r)
            if (lp_conv16_lds(c, r, KW, stride) <= LP_LDS_BUDGET) {
                *ck = c;  *kyn = r;  *lds = lp_conv16_lds(c, r, KW, stride);
                return;
            }
    *ck = 8;  *kyn = 1;  *lds = lp_conv16_lds(8, 1, KW, stride);
}

template <bool XB, bool YB>
static int lp_conv16_launch(hipStream_t stream, bool k3, dim3 grid, size_t lds, const LpConv16Args& a) {
    if (k3) {
        hipLaunchKernelGGL((k_lp_conv16<true, XB, YB>), grid, dim3(LP_T), lds, stream, a);
    } else {
        if (lds > 64 * 1024) {
            static bool raised = false;       // (one per instantiation, as the attribute is)
            if (!raised) {
                MGR_HIP(hipFuncSetAttribute((const void*)k_lp_conv16<false, XB, YB>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
                raised = true;
            }
        }
        hipLaunchKernelGGL((k_lp_conv16<false, XB, YB>), grid, dim3(LP_T), lds, stream, a);
    }
    return MGR_OK;
}

// as lp_conv, on bf16 operands; wp: k_lp_pack16's layout.  xs / ys: the storage of x (and gate) and of y
static int lp_conv16(hipStream_t stream, const char* name, int G, int Cin, int Cout, int H, int W, int KH, int KW, int stride, int pad,
                     const void* x, const void* gate, const void* wp, const float* bias, int relu, void* y,
                     int xs = MGR_LPIPS_STORE_F32, int ys = MGR_LPIPS_STORE_F32) {
    LpConv16Args a;
    a.Cin = Cin; a.Cout = Cout; a.CoP = (int)lp_pad64(Cout); a.NB = (int)(lp_pad8(Cin) >> 3); a.H = H; a.W = W;
    a.Ho = (H + 2 * pad - KH) / stride + 1; a.Wo = (W + 2 * pad - KW) / stride + 1;
    a.KH = KH; a.KW = KW; a.stride = stride; a.pad = pad; a.relu = relu;
    a.x = x; a.gate = gate; a.wp = (const lp_bf8*)wp; a.bias = bias; a.y = y;
    size_t lds;
    lp_conv16_chunk(Cin, KH, KW, stride, &a.CK, &a.KYN, &lds);
    if (lds > 150 * 1024) return mgr_fail(MGR_EINVAL, "k_lp_conv16: kernel window too large for LDS");
    a.NZ = (Cout + LP_TC - 1) / LP_TC;
    const dim3 grid((a.Wo + LP_TW - 1) / LP_TW, (a.Ho + LP_TH - 1) / LP_TH, (unsigned)(G * a.NZ));
    if (grid.y > 65535u || grid.z > 65535u) return mgr_fail(MGR_EINVAL, "k_lp_conv16: image too large");
    MGR_PROF(name, stream);
    const bool k3 = KH == 3 && KW == 3 && stride == 1 && pad == 1, xb = xs == MGR_LPIPS_STORE_BF16, yb = ys == MGR_LPIPS_STORE_BF16;
    const int rc = xb ? (yb ? lp_conv16_launch<true, true>(stream, k3, grid, lds, a) : lp_conv16_launch<true, false>(stream, k3, grid, lds, a))
                      : (yb ? lp_conv16_launch<false, true>(stream, k3, grid, lds, a) : lp_conv16_launch<false, false>(stream, k3, grid, lds, a));
    if (rc != MGR_OK) return rc;
    MGR_LAUNCH_CHECK(name, stream, 0);
    return MGR_OK;
}

// one convolution, of G views that sit batch-major in x / gate / y, in the call's operand mode; bf16 storage (xs, ys) goes
// with bf16 operands only (the entries refuse the rest)
static int lp_conv_op(int operands, hipStream_t stream, const char* name, const char* name16, int G, int Cin, int Cout, int H, int W,
                      int KH, int KW, int stride, int pad, const void* x, const void* gate, const void* wp, const float* bias, int relu,
                      void* y, int xs = MGR_LPIPS_STORE_F32, int ys = MGR_LPIPS_STORE_F32) {
    if (operands == MGR_LPIPS_BF16)
        return lp_conv16(stream, name16, G, Cin, Cout, H, W, KH, KW, stride, pad, x, gate, wp, bias, relu, y, xs, ys);
    return lp_conv(stream, name, G, Cin, Cout, H, W, KH, KW, stride, pad, (const float*)x, (const float*)gate, (const float*)wp, bias,
                   relu, (float*)y);
}

// ---------------------------------------------------------------------------
// scaling layer, pools
// ---------------------------------------------------------------------------
__constant__ float LP_SHIFT[3] = {-0.030f, -0.088f, -0.188f};
__constant__ float LP_SCALE[3] = {0.458f, 0.448f, 0.450f};

// out (3, H, W) = ((x * mask) [* 2 - 1] - shift) / scale
__global__ __launch_bounds__(LP_T) void k_lp_scale(int HW, const float* __restrict__ x, const float* __restrict__ mask, int normalize,
                                                   float* __restrict__ out) {
    const int p = blockIdx.x * LP_T + threadIdx.x;
    if (p >= HW) return;
    const float m = mask ? mask[p] : 1.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = x[(size_t)c * HW + p];
        if (mask) v *= m;
        if (normalize) v = 2.f * v - 1.f;
        out[(size_t)c * HW + p] = (v - LP_SHIFT[c]) / LP_SCALE[c];
    }
}

// dL/dx = g / scale [* 2] [* mask], written or added
__global__ __launch_bounds__(LP_T) void k_lp_scale_bwd(int HW, const float* __restrict__ g, const float* __restrict__ mask, int normalize,
                                                       int accumulate, float* __restrict__ dx) {
    const int p = blockIdx.x * LP_T + threadIdx.x;
    if (p >= HW) return;
    const float m = mask ? mask[p] : 1.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = g[(size_t)c * HW + p] / LP_SCALE[c];
        if (normalize) v *= 2.f;
        if (mask) v *= m;
        const size_t e = (size_t)c * HW + p;
        dx[e] = accumulate ? dx[e] + v : v;
    }
}

// The window of a frame.  A windowed view runs the chain on the contiguous (3, h, w) copy of the rectangle (x0, y0, w, h) of its
// (3, FH, FW) frame: these two kernels are k_lp_scale / k_lp_scale_bwd with a pitch and an origin, the arithmetic per element
// unchanged, so a window equals the call on .contiguous() crops bit for bit.  Lanes run along x (coalesced rows), no atomics.
// The table of a launch: entry j (blockIdx.z) is the window (x0[j], y0[j], w, h) of frame view[j] of x / mask / dx, which are
// the (V, 3, FH, FW) / (V, FH, FW) frames; its contiguous copy is slot j of out / g.  w and h are shared by the launch.
struct LpWin {
    int FH, FW;
    int view[LP_MAX_BATCH], x0[LP_MAX_BATCH], y0[LP_MAX_BATCH];
};

// grid (ceil(w / LP_T), h, entries).  out[j] (3, h, w) = k_lp_scale of x[view, :, y0 : y0 + h, x0 : x0 + w] (and of that rectangle
// of the mask)
__global__ __launch_bounds__(LP_T) void k_lp_scale_win(int w, int h, const LpWin f, const float* __restrict__ x,
                                                       const float* __restrict__ mask, int normalize, float* __restrict__ out) {
    const int cx = blockIdx.x * LP_T + threadIdx.x, cy = blockIdx.y, j = blockIdx.z;
    if (cx >= w || cy >= h) return;
    const size_t FP = (size_t)f.FH * f.FW, HW = (size_t)h * w;
    const size_t sp = (size_t)(f.y0[j] + cy) * f.FW + f.x0[j] + cx, p = (size_t)cy * w + cx;
    x += (size_t)f.view[j] * 3 * FP;
    out += (size_t)j * 3 * HW;
    const float m = mask ? mask[(size_t)f.view[j] * FP + sp] : 1.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = x[c * FP + sp];
        if (mask) v *= m;
        if (normalize) v = 2.f * v - 1.f;
        out[c * HW + p] = (v - LP_SHIFT[c]) / LP_SCALE[c];
    }
}

// accumulate = 1: grid (ceil(w / LP_T), h), the rectangle's value is added (one fp32 add) to the rectangle of dx (3, FH, FW) and
// the rest of the frame is not touched.  accumulate = 0: grid (ceil(FW / LP_T), FH), ONE launch writes the whole frame, the
// value inside the rectangle and 0 outside (w = 0 or h = 0: a zero fill; g is not read).  grid.z: the table's entries, every
// one its own frame of dx.
__global__ __launch_bounds__(LP_T) void k_lp_scale_bwd_win(int w, int h, const LpWin f, const float* __restrict__ g,
                                                           const float* __restrict__ mask, int normalize, int accumulate,
                                                           float* __restrict__ dx) {
    const int t = blockIdx.x * LP_T + threadIdx.x, j = blockIdx.z;
    const int x0 = f.x0[j], y0 = f.y0[j];
    const int gx = accumulate ? x0 + t : t, gy = accumulate ? y0 + (int)blockIdx.y : (int)blockIdx.y;
    if (gx >= f.FW || gy >= f.FH) return;
    const int cx = gx - x0, cy = gy - y0;
    const bool in = cx >= 0 && cx < w && cy >= 0 && cy < h;
    if (accumulate && !in) return;
    const size_t FP = (size_t)f.FH * f.FW, HW = (size_t)h * w;
    const size_t sp = (size_t)gy * f.FW + gx, p = in ? (size_t)cy * w + cx : 0;
    g += (size_t)j * 3 * HW;
    dx += (size_t)f.view[j] * 3 * FP;
    const float m = (mask && in) ? mask[(size_t)f.view[j] * FP + sp] : 1.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = 0.f;
        if (in) {
            v = g[c * HW + p] / LP_SCALE[c];
            if (normalize) v *= 2.f;
            if (mask) v *= m;
        }
        const size_t e = c * FP + sp;
        dx[e] = accumulate ? __fadd_rn(dx[e], v) : v;
    }
}

// max-pool k x k stride 2 (floor): the FIRST maximum in row-major window order, as torch
__global__ __launch_bounds__(LP_T) void k_lp_pool(int C, int H, int W, int Ho, int Wo, int k, const float* __restrict__ x,
                                                  float* __restrict__ y) {
    const size_t e = (size_t)blockIdx.x * LP_T + threadIdx.x;
    if (e >= (size_t)C * Ho * Wo) return;
    const int ox = (int)(e % Wo), oy = (int)((e / Wo) % Ho);
    const size_t c = e / ((size_t)Wo * Ho);
    const float* src = x + (c * H + 2 * oy) * W + 2 * ox;
    float m = src[0];
    for (int dy = 0; dy < k; ++dy)
        for (int dx = 0; dx < k; ++dx) {
            const float v = src[dy * W + dx];
            if (v > m) m = v;
        }
    y[e] = m;
}

// 2 x 2 stride 2 backward: one thread per INPUT element; the winner is recomputed from the stored input
__global__ __launch_bounds__(LP_T) void k_lp_pool2_bwd(int C, int H, int W, int Ho, int Wo, const float* __restrict__ x,
                                                       const float* __restrict__ gy, float* __restrict__ gx) {
    const size_t e = (size_t)blockIdx.x * LP_T + threadIdx.x;
    if (e >= (size_t)C * H * W) return;
    const int ix = (int)(e % W), iy = (int)((e / W) % H);
    const size_t c = e / ((size_t)W * H);
    const int ox = ix >> 1, oy = iy >> 1;
    float g = 0.f;
    if (ox < Wo && oy < Ho) {
        const float* src = x + (c * H + 2 * oy) * W + 2 * ox;
        float m = src[0];
        int win = 0;
        if (src[1] > m) { m = src[1]; win = 1; }
        if (src[W] > m) { m = src[W]; win = 2; }
        if (src[W + 1] > m) { m = src[W + 1]; win = 3; }
        if (win == ((iy & 1) << 1 | (ix & 1))) g = gy[(c * Ho + oy) * Wo + ox];
    }
    gx[e] = g;
}

// bf16 storage: one thread per (channel block, output pixel), 16-byte accesses; NBC = (views) x (blocks of 8 channels).  The
// maximum of the stored values is exact, the first maximum in row-major window order wins (its bits are copied).
__device__ __forceinline__ float lp_bf(unsigned short u) { return __uint_as_float((unsigned)u << 16); }

__global__ __launch_bounds__(LP_T) void k_lp_pool_b(int NBC, int H, int W, int Ho, int Wo, int k, const lp_us8* __restrict__ x,
                                                    lp_us8* __restrict__ y) {
    const size_t e = (size_t)blockIdx.x * LP_T + threadIdx.x;
    if (e >= (size_t)NBC * Ho * Wo) return;
    const int ox = (int)(e % Wo), oy = (int)((e / Wo) % Ho);
    const size_t c = e / ((size_t)Wo * Ho);
    const lp_us8* src = x + (c * H + 2 * oy) * W + 2 * ox;
    lp_us8 m = src[0];
    for (int dy = 0; dy < k; ++dy)
        for (int dx = 0; dx < k; ++dx) {
            const lp_us8 v = src[dy * W + dx];
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (lp_bf(v[j]) > lp_bf(m[j])) m[j] = v[j];
        }
    y[e] = m;
}

// 2 x 2 stride 2 backward, bf16 storage: one thread per (channel block, INPUT pixel); the winner is recomputed from the stored
// input, per lane.  Pad lanes hold zeros in x and gy, so they come out zero.
__global__ __launch_bounds__(LP_T) void k_lp_pool2_bwd_b(int NBC, int H, int W, int Ho, int Wo, const lp_us8* __restrict__ x,
                                                         const lp_us8* __restrict__ gy, lp_us8* __restrict__ gx) {
    const size_t e = (size_t)blockIdx.x * LP_T + threadIdx.x;
    if (e >= (size_t)NBC * H * W) return;
    const int ix = (int)(e % W), iy = (int)((e / W) % H);
    const size_t c = e / ((size_t)W * H);
    const int ox = ix >> 1, oy = iy >> 1;
    lp_us8 g = (lp_us8)(0);
    if (ox < Wo && oy < Ho) {
        const lp_us8* src = x + (c * H + 2 * oy) * W + 2 * ox;
        const lp_us8 s0 = src[0], s1 = src[1], s2 = src[W], s3 = src[W + 1], go = gy[(c * Ho + oy) * Wo + ox];
        const int me = (iy & 1) << 1 | (ix & 1);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float m = lp_bf(s0[j]);
            int win = 0;
            if (lp_bf(s1[j]) > m) { m = lp_bf(s1[j]); win = 1; }
            if (lp_bf(s2[j]) > m) { m = lp_bf(s2[j]); win = 2; }
            if (lp_bf(s3[j]) > m) { m = lp_bf(s3[j]); win = 3; }
            if (win == me) g[j] = go[j];
        }
    }
    gx[e] = g;
}

// ---------------------------------------------------------------------------
// head
// ---------------------------------------------------------------------------
__device__ __forceinline__ double lp_block_sum(double a, double* s_red, int tid) {
    s_red[tid] = a;
    __syncthreads();
#pragma unroll
    for (int h = LP_T / 2; h > 0; h >>= 1) {
        if (tid < h) s_red[tid] += s_red[tid + h];
        __syncthreads();
    }
    return s_red[0];
}

// one thread per pixel of a tap: sum_c lin[c] (f0 / n0 - f1 / n1)^2 into the workgroup's fp64 partial; with g: the gradient of
// gs * (that sum) w.r.t. f0, written (add = 0) or added (add = 1).  A pixel whose f0 is all zero contributes no gradient.
// blockIdx.y is the view of the chunk: f0 and g are batch-major, f1 (cached taps live in a buffer per view) and gs (the view's
// grad_scale / (H_k W_k)) come per view, and view b's partials start at b part_stride.
struct LpHeadArgs {
    const float* f1[LP_MAX_BATCH];
    float gs[LP_MAX_BATCH];
};

__global__ __launch_bounds__(LP_T) void k_lp_head(int C, int HW, const float* __restrict__ f0, const LpHeadArgs t,
                                                  const float* __restrict__ lin, float* __restrict__ g, int add,
                                                  double* __restrict__ part, int part_stride) {
    __shared__ double s_red[LP_T];
    const int tid = threadIdx.x, p = blockIdx.x * LP_T + tid, vb = blockIdx.y;
    const float* __restrict__ f1 = t.f1[vb];
    const float gs = t.gs[vb];
    f0 += (size_t)vb * C * HW;
    if (g) g += (size_t)vb * C * HW;
    part += (size_t)vb * part_stride;
    double val = 0.0;
    if (p < HW) {
        float s0 = 0.f, s1 = 0.f;
        for (int c = 0; c < C; ++c) {
            const float a = f0[(size_t)c * HW + p], b = f1[(size_t)c * HW + p];
            s0 = fmaf(a, a, s0);
            s1 = fmaf(b, b, s1);
        }
        const float r0 = sqrtf(s0), n0 = r0 + 1e-10f, n1 = sqrtf(s1) + 1e-10f;
        float v = 0.f, dot = 0.f;
        for (int c = 0; c < C; ++c) {
            const float a = f0[(size_t)c * HW + p], b = f1[(size_t)c * HW + p];
            const float d = a / n0 - b / n1, l = lin[c];
            v = fmaf(l, d * d, v);
            dot = fmaf(2.f * l * d, a, dot);
        }
        val = (double)v;
        if (g) {
            // u = f0 / n0, n0 = r0 + eps: dL/df0[c] = gu[c] / n0 - (sum_c' gu[c'] f0[c']) f0[c] / (n0^2 r0), gu = 2 gs lin (u - v)
            const float k2 = r0 > 0.f ? dot / (n0 * n0 * r0) : 0.f;
            for (int c = 0; c < C; ++c) {
                const size_t e = (size_t)c * HW + p;
                const float a = f0[e], b = f1[e];
                const float d = a / n0 - b / n1;
                const float t = r0 > 0.f ? gs * (2.f * lin[c] * d / n0 - k2 * a) : 0.f;
                g[e] = add ? g[e] + t : t;
            }
        }
    }
    const double tot = lp_block_sum(val, s_red, tid);
    if (tid == 0) part[blockIdx.x] = tot;
}

// k_lp_head on bf16 storage: f0, f1 and g are [ceil(C / 8)][HW][8] bf16 (t.f1 holds the per-view addresses of such buffers).
// The taps are read exactly, the arithmetic and its channel order are k_lp_head's; the gradient is rounded once at the store --
// with add = 1, fp32(stored g) + t rounded once -- and the pad lanes of g are written as zero.
__global__ __launch_bounds__(LP_T) void k_lp_head_b(int C, int HW, const lp_us8* __restrict__ f0, const LpHeadArgs t,
                                                    const float* __restrict__ lin, lp_us8* __restrict__ g, int add,
                                                    double* __restrict__ part, int part_stride) {
    __shared__ double s_red[LP_T];
    const int tid = threadIdx.x, p = blockIdx.x * LP_T + tid, vb = blockIdx.y, NB = (C + 7) >> 3;
    const lp_us8* __restrict__ f1 = (const lp_us8*)t.f1[vb];
    const float gs = t.gs[vb];
    f0 += (size_t)vb * NB * HW;
    if (g) g += (size_t)vb * NB * HW;
    part += (size_t)vb * part_stride;
    double val = 0.0;
    if (p < HW) {
        float s0 = 0.f, s1 = 0.f;
        for (int cb = 0; cb < NB; ++cb) {
            const lp_us8 va = f0[(size_t)cb * HW + p], vbb = f1[(size_t)cb * HW + p];
#pragma unroll
            for (int j = 0; j < 8; ++j) {       // (a pad lane adds +0)
                const float a = lp_bf(va[j]), b = lp_bf(vbb[j]);
                s0 = fmaf(a, a, s0);
                s1 = fmaf(b, b, s1);
            }
        }
        const float r0 = sqrtf(s0), n0 = r0 + 1e-10f, n1 = sqrtf(s1) + 1e-10f;
        float v = 0.f, dot = 0.f;
        for (int cb = 0; cb < NB; ++cb) {
            const lp_us8 va = f0[(size_t)cb * HW + p], vbb = f1[(size_t)cb * HW + p];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (cb * 8 + j >= C) break;
                const float a = lp_bf(va[j]), b = lp_bf(vbb[j]);
                const float d = a / n0 - b / n1, l = lin[cb * 8 + j];
                v = fmaf(l, d * d, v);
                dot = fmaf(2.f * l * d, a, dot);
            }
        }
        val = (double)v;
        if (g) {
            const float k2 = r0 > 0.f ? dot / (n0 * n0 * r0) : 0.f;
            for (int cb = 0; cb < NB; ++cb) {
                const size_t e = (size_t)cb * HW + p;
                const lp_us8 va = f0[e], vbb = f1[e];
                lp_us8 old = (lp_us8)(0);
                if (add) old = g[e];
                lp_bf8 out;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float w = 0.f;
                    if (cb * 8 + j < C) {
                        const float a = lp_bf(va[j]), b = lp_bf(vbb[j]);
                        const float d = a / n0 - b / n1;
                        const float tt = r0 > 0.f ? gs * (2.f * lin[cb * 8 + j] * d / n0 - k2 * a) : 0.f;
                        w = add ? lp_bf(old[j]) + tt : tt;
                    }
                    out[j] = (__bf16)w;
                }
                *(lp_bf8*)(g + e) = out;
            }
        }
    }
    const double tot = lp_block_sum(val, s_red, tid);
    if (tid == 0) part[blockIdx.x] = tot;
}

struct LpFoldArgs {
    int off[LP_NTAP + 1];
    double inv[LP_NTAP];
    int view[LP_MAX_BATCH];       // workgroup b folds the partials at b off[LP_NTAP] into value[view[b]]
};

// values[v] = sum_k (sum of tap k's partials) / (H_k W_k): thread t adds slots t, t + 256, ... in ascending order, fixed tree
__global__ __launch_bounds__(LP_T) void k_lp_fold(const LpFoldArgs a, const double* __restrict__ part, float* __restrict__ value) {
    __shared__ double s_red[LP_T];
    const int tid = threadIdx.x;
    part += (size_t)blockIdx.x * a.off[LP_NTAP];
    value += a.view[blockIdx.x];
    double d = 0.0;
    for (int k = 0; k < LP_NTAP; ++k) {
        double s = 0.0;
        for (int i = a.off[k] + tid; i < a.off[k + 1]; i += LP_T) s += part[i];
        const double tot = lp_block_sum(s, s_red, tid);
        __syncthreads();
        d += tot * a.inv[k];
    }
    if (tid == 0) *value = (float)d;
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" size_t mgr_lpips_net_bytes_op(int net, int operands) {
    LpNet n;
    if (!lp_net(net, &n) || !lp_operands_ok(operands)) return 0;
    return lp_blob(n, operands).total;
}

extern "C" size_t mgr_lpips_net_bytes(int net) { return mgr_lpips_net_bytes_op(net, MGR_LPIPS_F32); }

extern "C" int mgr_lpips_net_pack_op(int net, const float* const* conv_w, const float* const* conv_b, const float* const* lin_w,
                                     void* blob, size_t blob_bytes, void* stream_, int operands) {
    hipStream_t stream = (hipStream_t)stream_;
    LpNet n;
    if (!lp_net(net, &n)) return mgr_fail(MGR_EINVAL, "mgr_lpips_net_pack: net must be 0 (vgg) or 1 (alex)");
    if (!lp_operands_ok(operands)) return mgr_fail(MGR_EINVAL, "mgr_lpips_net_pack: operands must be 0 (fp32) or 1 (bf16)");
    if (!conv_w || !conv_b || !lin_w || !blob) return mgr_fail(MGR_EINVAL, "mgr_lpips_net_pack: null pointer");
    const LpBlob B = lp_blob(n, operands);
    if (blob_bytes != B.total)
        return mgr_fail(MGR_EINVAL, "mgr_lpips_net_pack: blob_bytes is not mgr_lpips_net_bytes(net) of this operand mode");
    for (int i = 0; i < n.n_conv; ++i)
        if (!conv_w[i] || !conv_b[i]) return mgr_fail(MGR_EINVAL, "mgr_lpips_net_pack: null weight or bias pointer");
    for (int k = 0; k < LP_NTAP; ++k)
        if (!lin_w[k]) return mgr_fail(MGR_EINVAL, "mgr_lpips_net_pack: null lin pointer");
    char* base = (char*)blob;
    int ci = 0;
    for (int i = 0; i < n.n_ops; ++i) {
        const LpOp& op = n.ops[i];
        if (!op.conv) continue;
        const int KK = op.k * op.k, CoP = (int)lp_pad64(op.cout), CiP = (int)lp_pad64(op.cin);
        const size_t nf = (size_t)op.cin * KK * CoP;
        const unsigned nb = (unsigned)((nf + LP_T - 1) / LP_T < 4096 ? (nf + LP_T - 1) / LP_T : 4096);
        if (operands == MGR_LPIPS_BF16) {
            hipLaunchKernelGGL(k_lp_pack16, dim3(nb), dim3(LP_T), 0, stream, op.cout, op.cin, KK, CoP, CiP, conv_w[ci], conv_b[ci],
                               (__bf16*)(base + B.w[ci]), (float*)(base + B.b[ci]),
                               n.has_bwd ? (__bf16*)(base + B.wt[ci]) : (__bf16*)nullptr);
            MGR_LAUNCH_CHECK("k_lp_pack16", stream, 0);
        } else {
            hipLaunchKernelGGL(k_lp_pack, dim3(nb), dim3(LP_T), 0, stream, op.cout, op.cin, KK, CoP, CiP, conv_w[ci], conv_b[ci],
                               (float*)(base + B.w[ci]), (float*)(base + B.b[ci]),
                               n.has_bwd ? (float*)(base + B.wt[ci]) : (float*)nullptr);
            MGR_LAUNCH_CHECK("k_lp_pack", stream, 0);
        }
        if (op.tap >= 0) {
            hipLaunchKernelGGL(k_lp_copy, dim3((op.cout + LP_T - 1) / LP_T), dim3(LP_T), 0, stream, op.cout, lin_w[op.tap],
                               (float*)(base + B.lin[op.tap]));
            MGR_LAUNCH_CHECK("k_lp_copy", stream, 0);
        }
        ++ci;
    }
    return MGR_OK;
}

extern "C" int mgr_lpips_net_pack(int net, const float* const* conv_w, const float* const* conv_b, const float* const* lin_w, void* blob,
                                  size_t blob_bytes, void* stream) {
    return mgr_lpips_net_pack_op(net, conv_w, conv_b, lin_w, blob, blob_bytes, stream, MGR_LPIPS_F32);
}

extern "C" size_t mgr_lpips_workspace_bytes_st(int net, int H, int W, int need_grad, int storage) {
    LpNet n;
    LpLayout L;
    if (!lp_net(net, &n) || !lp_storage_ok(storage) || !lp_layout(n, H, W, need_grad, &L, 1, storage)) return 0;
    return L.total;
}

extern "C" size_t mgr_lpips_workspace_bytes(int net, int H, int W, int need_grad) {
    return mgr_lpips_workspace_bytes_st(net, H, W, need_grad, MGR_LPIPS_STORE_F32);
}

extern "C" int mgr_lpips_layout_st(int net, int H, int W, int need_grad, size_t* offsets, int n_off, int storage) {
    LpNet n;
    LpLayout L;
    if (!lp_net(net, &n)) return mgr_fail(MGR_EINVAL, "mgr_lpips_layout: net must be 0 (vgg) or 1 (alex)");
    if (!lp_storage_ok(storage)) return mgr_fail(MGR_EINVAL, "mgr_lpips_layout: storage must be 0 (fp32) or 1 (bf16)");
    if (!lp_layout(n, H, W, need_grad, &L, 1, storage))
        return mgr_fail(MGR_EINVAL, "mgr_lpips_layout: image too small for the deepest tap (or too large)");
    const int need = n.n_conv + LP_NTAP + 4;
    if (!offsets || n_off < need) return mgr_fail(MGR_EINVAL, "mgr_lpips_layout: offsets holds fewer than n_conv + 9 entries");
    int j = 0;
    for (int i = 0; i < n.n_conv; ++i) offsets[j++] = L.act[i];
    for (int k = 0; k < LP_NTAP; ++k) offsets[j++] = L.tap[k];
    offsets[j++] = L.bufa;
    offsets[j++] = L.bufb;
    offsets[j++] = L.part;
    offsets[j++] = L.total;
    return need;
}

extern "C" int mgr_lpips_layout(int net, int H, int W, int need_grad, size_t* offsets, int n_off) {
    return mgr_lpips_layout_st(net, H, W, need_grad, offsets, n_off, MGR_LPIPS_STORE_F32);
}

// the refusal shared by the *_st entries: null where (operands, storage) is a mode of this file
static const char* lp_storage_refusal(int operands, int storage) {
    if (!lp_storage_ok(storage)) return "storage must be 0 (fp32) or 1 (bf16)";
    if (storage == MGR_LPIPS_STORE_BF16 && operands == MGR_LPIPS_F32) return "bf16 storage needs bf16 operands (fp32 operands are refused)";
    return nullptr;
}

extern "C" int mgr_lpips_conv_st(int Cin, int Cout, int H, int W, int KH, int KW, int stride, int pad, const float* x, const float* gate,
                                 const float* w, const float* bias, int relu, int transposed, float* y, void* scratch,
                                 size_t scratch_bytes, void* stream_, int operands, int x_storage, int y_storage) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!lp_operands_ok(operands)) return mgr_fail(MGR_EINVAL, "mgr_lpips_conv: operands must be 0 (fp32) or 1 (bf16)");
    for (int s : {x_storage, y_storage})
        if (const char* why = lp_storage_refusal(operands, s)) return mgr_fail(MGR_EINVAL, "mgr_lpips_conv: %s", why);
    if (Cin < 1 || Cout < 1 || H < 1 || W < 1 || KH < 1 || KW < 1 || KH != KW || stride < 1 || pad < 0 || H + 2 * pad < KH || W + 2 * pad < KW)
        return mgr_fail(MGR_EINVAL, "mgr_lpips_conv: bad sizes");
    if (!x || !w || !y || !scratch) return mgr_fail(MGR_EINVAL, "mgr_lpips_conv: null pointer");
    if (transposed && (stride != 1 || 2 * pad != KH - 1)) return mgr_fail(MGR_EINVAL, "mgr_lpips_conv: the data gradient needs stride 1 and a same-size pad");
    if (transposed && bias) return mgr_fail(MGR_EINVAL, "mgr_lpips_conv: the data gradient takes no bias");
    const int KK = KH * KW, CoP = (int)lp_pad64(Cout), CiP = (int)lp_pad64(Cin);
    // scratch: [forward pack][bias pack][data-gradient pack]
    const size_t o_f = 0, o_b = mgr_align(lp_wbytes(operands, Cin, KK, Cout)), o_t = o_b + mgr_align((size_t)CoP * 4),
                 tot = o_t + mgr_align(lp_wbytes(operands, Cout, KK, Cin));
    if (scratch_bytes < tot) return mgr_fail(MGR_ENOMEM, "mgr_lpips_conv: scratch too small");
    char* base = (char*)scratch;
    // w is [Cout][Cin][KH][KW]; transposed: the layer is used backwards, x has Cout channels and y gets Cin
    const float* bsrc = bias ? bias : w;        // (k_lp_pack reads Cout values; unused where bias is null)
    if (operands == MGR_LPIPS_BF16) {
        hipLaunchKernelGGL(k_lp_pack16, dim3(256), dim3(LP_T), 0, stream, Cout, Cin, KK, CoP, CiP, w, bsrc, (__bf16*)(base + o_f),
                           (float*)(base + o_b), (__bf16*)(base + o_t));
        MGR_LAUNCH_CHECK("k_lp_pack16", stream, 0);
    } else {
        hipLaunchKernelGGL(k_lp_pack, dim3(256), dim3(LP_T), 0, stream, Cout, Cin, KK, CoP, CiP, w, bsrc, (float*)(base + o_f),
                           (float*)(base + o_b), (float*)(base + o_t));
        MGR_LAUNCH_CHECK("k_lp_pack", stream, 0);
    }
    if (transposed)
        return lp_conv_op(operands, stream, "k_lp_conv_bwd", "k_lp_conv16_bwd", 1, Cout, Cin, H, W, KH, KW, 1, pad, x, gate, base + o_t,
                          nullptr, relu, y, x_storage, y_storage);
    return lp_conv_op(operands, stream, "k_lp_conv", "k_lp_conv16", 1, Cin, Cout, H, W, KH, KW, stride, pad, x, gate, base + o_f,
                      bias ? (const float*)(base + o_b) : nullptr, relu, y, x_storage, y_storage);
}

extern "C" int mgr_lpips_conv_op(int Cin, int Cout, int H, int W, int KH, int KW, int stride, int pad, const float* x, const float* gate,
                                 const float* w, const float* bias, int relu, int transposed, float* y, void* scratch,
                                 size_t scratch_bytes, void* stream, int operands) {
    return mgr_lpips_conv_st(Cin, Cout, H, W, KH, KW, stride, pad, x, gate, w, bias, relu, transposed, y, scratch, scratch_bytes, stream,
                             operands, MGR_LPIPS_STORE_F32, MGR_LPIPS_STORE_F32);
}

extern "C" int mgr_lpips_conv(int Cin, int Cout, int H, int W, int KH, int KW, int stride, int pad, const float* x, const float* gate,
                              const float* w, const float* bias, int relu, int transposed, float* y, void* scratch, size_t scratch_bytes,
                              void* stream) {
    return mgr_lpips_conv_op(Cin, Cout, H, W, KH, KW, stride, pad, x, gate, w, bias, relu, transposed, y, scratch, scratch_bytes, stream,
                             MGR_LPIPS_F32);
}

extern "C" size_t mgr_lpips_conv_scratch_bytes_op(int Cin, int Cout, int KH, int KW, int operands) {
    if (Cin < 1 || Cout < 1 || KH < 1 || KW < 1 || !lp_operands_ok(operands)) return 0;
    const size_t KK = (size_t)KH * KW;
    return mgr_align(lp_wbytes(operands, Cin, KK, Cout)) + mgr_align(lp_pad64(Cout) * 4) + mgr_align(lp_wbytes(operands, Cout, KK, Cin));
}

extern "C" size_t mgr_lpips_conv_scratch_bytes(int Cin, int Cout, int KH, int KW) {
    return mgr_lpips_conv_scratch_bytes_op(Cin, Cout, KH, KW, MGR_LPIPS_F32);
}

// forward of G images: scaled images -> sb, then the ops; a convolution writes to its slot of `store` (by convolution index)
// where that is not null, else to the scratch buffer its input is not in.  Every buffer is batch-major.  win = null: G = 1 and
// img / mask are one contiguous (3,H,W) / (H,W) image; else they are the frames and (H, W) is the size of win's G rectangles.
// st: the storage of every tensor but the scaled image, which is fp32 (the first convolution reads it so).
static int lp_forward(int operands, hipStream_t stream, const LpNet& n, const LpBlob& B, const char* blob, const LpShape& S, int H, int W,
                      int G, const float* img, const float* mask, int normalize, void* const* store, void* sa, void* sb,
                      const LpWin* win = nullptr, int st = MGR_LPIPS_STORE_F32) {
    const int HW = H * W;
    if (win) {
        hipLaunchKernelGGL(k_lp_scale_win, dim3((W + LP_T - 1) / LP_T, H, G), dim3(LP_T), 0, stream, W, H, *win, img, mask, normalize,
                           (float*)sb);
        MGR_LAUNCH_CHECK("k_lp_scale_win", stream, 0);
    } else {
        hipLaunchKernelGGL(k_lp_scale, dim3((HW + LP_T - 1) / LP_T), dim3(LP_T), 0, stream, HW, img, mask, normalize, (float*)sb);
        MGR_LAUNCH_CHECK("k_lp_scale", stream, 0);
    }
    const void* cur = sb;
    int h = H, w = W, ci = 0;
    for (int i = 0; i < n.n_ops; ++i) {
        const LpOp& op = n.ops[i];
        void* out;
        if (op.conv) {
            out = store[ci] ? store[ci] : (cur == sa ? sb : sa);
            const int rc = lp_conv_op(operands, stream, "k_lp_conv", "k_lp_conv16", G, op.cin, op.cout, h, w, op.k, op.k, op.s, op.p, cur,
                                      nullptr, blob + B.w[ci], (const float*)(blob + B.b[ci]), 1, out, i ? st : MGR_LPIPS_STORE_F32, st);
            if (rc != MGR_OK) return rc;
            ++ci;
        } else if (st == MGR_LPIPS_STORE_BF16) {
            // a per-block kernel: the G views are G pad8(cout) / 8 blocks
            out = cur == sa ? sb : sa;
            const int nbc = G * (int)(lp_pad8(op.cout) >> 3);
            const size_t ne = (size_t)nbc * S.h[i] * S.w[i];
            hipLaunchKernelGGL(k_lp_pool_b, dim3((unsigned)((ne + LP_T - 1) / LP_T)), dim3(LP_T), 0, stream, nbc, h, w, S.h[i], S.w[i],
                               op.k, (const lp_us8*)cur, (lp_us8*)out);
            MGR_LAUNCH_CHECK("k_lp_pool_b", stream, 0);
        } else {
            // a per-channel kernel: the G views are G cout channels
            out = cur == sa ? sb : sa;
            const size_t ne = (size_t)G * op.cout * S.h[i] * S.w[i];
            hipLaunchKernelGGL(k_lp_pool, dim3((unsigned)((ne + LP_T - 1) / LP_T)), dim3(LP_T), 0, stream, G * op.cout, h, w, S.h[i],
                               S.w[i], op.k, (const float*)cur, (float*)out);
            MGR_LAUNCH_CHECK("k_lp_pool", stream, 0);
        }
        cur = out;
        h = S.h[i];
        w = S.w[i];
    }
    return MGR_OK;
}

// G equal-size views of a call (one chunk; G = 1 in the plain and the sequential windowed call), validated by the caller: the
// two forwards (the target's only for the views whose `taps` entry is null, batched among themselves), the heads, the gradient
// chain and the folds into values[view].  The workspace is lp_layout's of G.  win = null: G = 1 and pred / target / mk / dL /
// values are that view's contiguous images and value; else they are the call's frames and (H, W) is the size of win's
// rectangles.  taps[b]: view b's five target taps as mgr_lpips_roi_taps_op left them (in the one-view layout), or null.
static int lp_views(int operands, hipStream_t stream, const LpNet& n, const LpBlob& B, const char* blob, int H, int W, int G,
                    const LpWin* win, const float* pred, const float* target, const float* mk, const float* const* taps, int normalize,
                    const float* grad_scale, float* values, float* dL, int accumulate, char* ws, int st = MGR_LPIPS_STORE_F32) {
    const int need_grad = dL != nullptr;
    const bool blocked = st == MGR_LPIPS_STORE_BF16;
    LpLayout L, L1;
    LpShape S;
    if (!lp_layout(n, H, W, need_grad, &L, (size_t)G, st) || !lp_layout(n, H, W, need_grad, &L1, 1, st) || !lp_shapes(n, H, W, &S))
        return mgr_fail(MGR_EINVAL, "mgr_lpips: image too small");
    void *sa = ws + L.bufa, *sb = ws + L.bufb;
    double* part = (double*)(ws + L.part);
    const int part_stride = (int)L.part_off[LP_NTAP];
    // the views whose target tower runs: slot j of the workspace's tap regions is view tw.view[j]
    LpWin tw = {};
    int slot[LP_MAX_BATCH], GT = 0;
    if (win) {
        tw.FH = win->FH;
        tw.FW = win->FW;
    }
    for (int b = 0; b < G; ++b) {
        slot[b] = -1;
        if (taps && taps[b]) continue;
        slot[b] = GT;
        if (win) { tw.view[GT] = win->view[b];  tw.x0[GT] = win->x0[b];  tw.y0[GT] = win->y0[b]; }
        ++GT;
    }
    void *act[13], *tgt[13];
    LpHeadArgs ha[LP_NTAP];
    int tap_conv[LP_NTAP], tap_op[LP_NTAP];
    {
        int ci = 0;
        for (int i = 0; i < n.n_ops; ++i) {
            const LpOp& op = n.ops[i];
            if (!op.conv) continue;
            act[ci] = ws + L.act[ci];
            tgt[ci] = nullptr;
            if (op.tap >= 0) {
                tgt[ci] = ws + L.tap[op.tap];
                const size_t e = lp_tbytes(st, op.cout, S.h[i], S.w[i]);       // bytes of one view
                for (int b = 0; b < LP_MAX_BATCH; ++b) {
                    ha[op.tap].f1[b] = nullptr;
                    ha[op.tap].gs[b] = 0.f;
                    if (b >= G) continue;
                    ha[op.tap].f1[b] = slot[b] < 0 ? (const float*)((const char*)taps[b] + (L1.tap[op.tap] - L1.tap[0]))
                                                   : (const float*)((const char*)tgt[ci] + (size_t)slot[b] * e);
                }
                tap_conv[op.tap] = ci;
                tap_op[op.tap] = i;
            }
            ++ci;
        }
    }
    LpFoldArgs fa = {};
    for (int k = 0; k <= LP_NTAP; ++k) fa.off[k] = (int)L.part_off[k];
    for (int k = 0; k < LP_NTAP; ++k) fa.inv[k] = 1.0 / ((double)S.h[tap_op[k]] * S.w[tap_op[k]]);
    for (int b = 0; b < G; ++b) fa.view[b] = win ? win->view[b] : 0;
    if (need_grad)
        for (int k = 0; k < LP_NTAP; ++k)
            for (int b = 0; b < G; ++b) ha[k].gs[b] = (float)((double)grad_scale[b] * fa.inv[k]);

    int rc;
    if (GT) {
        rc = lp_forward(operands, stream, n, B, blob, S, H, W, GT, target, mk, normalize, tgt, sa, sb, win ? &tw : nullptr, st);
        if (rc != MGR_OK) return rc;
    }
    rc = lp_forward(operands, stream, n, B, blob, S, H, W, G, pred, mk, normalize, act, sa, sb, win, st);
    if (rc != MGR_OK) return rc;
    if (!need_grad) {
        MGR_PROF("k_lp_head", stream);
        for (int k = 0; k < LP_NTAP; ++k) {
            const int i = tap_op[k], hw = S.h[i] * S.w[i];
            if (blocked)
                hipLaunchKernelGGL(k_lp_head_b, dim3((hw + LP_T - 1) / LP_T, G), dim3(LP_T), 0, stream, n.ops[i].cout, hw,
                                   (const lp_us8*)act[tap_conv[k]], ha[k], (const float*)(blob + B.lin[k]), (lp_us8*)nullptr, 0,
                                   part + L.part_off[k], part_stride);
            else
                hipLaunchKernelGGL(k_lp_head, dim3((hw + LP_T - 1) / LP_T, G), dim3(LP_T), 0, stream, n.ops[i].cout, hw,
                                   (const float*)act[tap_conv[k]], ha[k], (const float*)(blob + B.lin[k]), (float*)nullptr, 0,
                                   part + L.part_off[k], part_stride);
            MGR_LAUNCH_CHECK("k_lp_head", stream, 0);
        }
    } else {
        // from the deepest tap down: g holds dL/d(post-ReLU output) of the current op
        void *g = sa, *o = sb;
        bool have = false;       // g holds a gradient from deeper layers
        int h_in, w_in;
        for (int i = n.n_ops - 1; i >= 0; --i) {
            const LpOp& op = n.ops[i];
            h_in = i ? S.h[i - 1] : H;
            w_in = i ? S.w[i - 1] : W;
            if (op.conv) {
                int ci = 0;
                for (int j = 0; j < i; ++j) ci += n.ops[j].conv;
                if (op.tap >= 0) {
                    const int hw = S.h[i] * S.w[i], k = op.tap;
                    MGR_PROF("k_lp_head", stream);
                    if (blocked)
                        hipLaunchKernelGGL(k_lp_head_b, dim3((hw + LP_T - 1) / LP_T, G), dim3(LP_T), 0, stream, op.cout, hw,
                                           (const lp_us8*)act[ci], ha[k], (const float*)(blob + B.lin[k]), (lp_us8*)g, have ? 1 : 0,
                                           part + L.part_off[k], part_stride);
                    else
                        hipLaunchKernelGGL(k_lp_head, dim3((hw + LP_T - 1) / LP_T, G), dim3(LP_T), 0, stream, op.cout, hw,
                                           (const float*)act[ci], ha[k], (const float*)(blob + B.lin[k]), (float*)g, have ? 1 : 0,
                                           part + L.part_off[k], part_stride);
                    MGR_LAUNCH_CHECK("k_lp_head", stream, 0);
                    have = true;
                }
                // dL/d(input) = conv(g * [y > 0], W'); layer 0's is dL/d(scaled image), fp32 in both storages
                rc = lp_conv_op(operands, stream, "k_lp_conv_bwd", "k_lp_conv16_bwd", G, op.cout, op.cin, S.h[i], S.w[i], op.k, op.k, 1,
                                op.p, g, act[ci], blob + B.wt[ci], nullptr, 0, o, st, i ? st : MGR_LPIPS_STORE_F32);
                if (rc != MGR_OK) return rc;
            } else {
                // the pool's input is the previous convolution's stored output
                int ci = -1;
                for (int j = 0; j < i; ++j) ci += n.ops[j].conv;
                MGR_PROF("k_lp_pool2_bwd", stream);
                if (blocked) {
                    const int nbc = G * (int)(lp_pad8(op.cin) >> 3);
                    const size_t ne = (size_t)nbc * h_in * w_in;
                    hipLaunchKernelGGL(k_lp_pool2_bwd_b, dim3((unsigned)((ne + LP_T - 1) / LP_T)), dim3(LP_T), 0, stream, nbc, h_in, w_in,
                                       S.h[i], S.w[i], (const lp_us8*)act[ci], (const lp_us8*)g, (lp_us8*)o);
                } else {
                    const size_t ne = (size_t)G * op.cin * h_in * w_in;
                    hipLaunchKernelGGL(k_lp_pool2_bwd, dim3((unsigned)((ne + LP_T - 1) / LP_T)), dim3(LP_T), 0, stream, G * op.cin, h_in,
                                       w_in, S.h[i], S.w[i], (const float*)act[ci], (const float*)g, (float*)o);
                }
                MGR_LAUNCH_CHECK("k_lp_pool2_bwd", stream, 0);
            }
            void* t = g;  g = o;  o = t;
        }
        if (win) {
            const dim3 grid = accumulate ? dim3((W + LP_T - 1) / LP_T, H, G) : dim3((win->FW + LP_T - 1) / LP_T, win->FH, G);
            hipLaunchKernelGGL(k_lp_scale_bwd_win, grid, dim3(LP_T), 0, stream, W, H, *win, (const float*)g, mk, normalize, accumulate, dL);
            MGR_LAUNCH_CHECK("k_lp_scale_bwd_win", stream, 0);
        } else {
            const int HW = H * W;
            hipLaunchKernelGGL(k_lp_scale_bwd, dim3((HW + LP_T - 1) / LP_T), dim3(LP_T), 0, stream, HW, (const float*)g, mk, normalize,
                               accumulate, dL);
            MGR_LAUNCH_CHECK("k_lp_scale_bwd", stream, 0);
        }
    }
    hipLaunchKernelGGL(k_lp_fold, dim3(G), dim3(LP_T), 0, stream, fa, (const double*)part, values);
    MGR_LAUNCH_CHECK("k_lp_fold", stream, 0);
    return MGR_OK;
}

extern "C" int mgr_lpips_st(int net, int V, int H, int W, const float* pred, const float* target, const float* mask, const void* blob_,
                            size_t blob_bytes, int normalize, float grad_scale, float* values, float* dL_dpred, int accumulate,
                            void* workspace, size_t workspace_bytes, void* stream_, int operands, int storage) {
    hipStream_t stream = (hipStream_t)stream_;
    LpNet n;
    if (!lp_net(net, &n)) return mgr_fail(MGR_EINVAL, "mgr_lpips: net must be 0 (vgg) or 1 (alex)");
    if (!lp_operands_ok(operands)) return mgr_fail(MGR_EINVAL, "mgr_lpips: operands must be 0 (fp32) or 1 (bf16)");
    if (const char* why = lp_storage_refusal(operands, storage)) return mgr_fail(MGR_EINVAL, "mgr_lpips: %s", why);
    if (V <= 0 || H <= 0 || W <= 0) return mgr_fail(MGR_EINVAL, "mgr_lpips: bad sizes");
    if (!pred || !target || !blob_ || !values || !workspace) return mgr_fail(MGR_EINVAL, "mgr_lpips: null pointer");
    if (dL_dpred && !n.has_bwd) return mgr_fail(MGR_EINVAL, "mgr_lpips: the AlexNet network is forward only (dL_dpred must be null)");
    const int need_grad = dL_dpred != nullptr;
    LpLayout L;
    if (!lp_layout(n, H, W, need_grad, &L, 1, storage))
        return mgr_fail(MGR_EINVAL, "mgr_lpips: image too small for the deepest tap to have one pixel (or above 2^24 pixels)");
    const LpBlob B = lp_blob(n, operands);
    if (blob_bytes != B.total) return mgr_fail(MGR_EINVAL, "mgr_lpips: blob_bytes is not mgr_lpips_net_bytes(net) of this operand mode");
    if (workspace_bytes < L.total) return mgr_fail(MGR_ENOMEM, "mgr_lpips: workspace smaller than mgr_lpips_workspace_bytes");
    const size_t img = (size_t)3 * H * W, px = (size_t)H * W;
    for (int v = 0; v < V; ++v) {
        const int rc = lp_views(operands, stream, n, B, (const char*)blob_, H, W, 1, nullptr, pred + v * img, target + v * img,
                                mask ? mask + v * px : nullptr, nullptr, normalize, &grad_scale, values + v,
                                dL_dpred ? dL_dpred + v * img : nullptr, accumulate, (char*)workspace, storage);
        if (rc != MGR_OK) return rc;
    }
    return MGR_OK;
}

extern "C" int mgr_lpips_op(int net, int V, int H, int W, const float* pred, const float* target, const float* mask, const void* blob,
                            size_t blob_bytes, int normalize, float grad_scale, float* values, float* dL_dpred, int accumulate,
                            void* workspace, size_t workspace_bytes, void* stream, int operands) {
    return mgr_lpips_st(net, V, H, W, pred, target, mask, blob, blob_bytes, normalize, grad_scale, values, dL_dpred, accumulate, workspace,
                        workspace_bytes, stream, operands, MGR_LPIPS_STORE_F32);
}

extern "C" int mgr_lpips(int net, int V, int H, int W, const float* pred, const float* target, const float* mask, const void* blob,
                         size_t blob_bytes, int normalize, float grad_scale, float* values, float* dL_dpred, int accumulate,
                         void* workspace, size_t workspace_bytes, void* stream) {
    return mgr_lpips_op(net, V, H, W, pred, target, mask, blob, blob_bytes, normalize, grad_scale, values, dL_dpred, accumulate, workspace,
                        workspace_bytes, stream, MGR_LPIPS_F32);
}

// ---------------------------------------------------------------------------
// the windowed call
// ---------------------------------------------------------------------------
// 0: empty, 1: fine, < 0: refused (-1 negative size, -2 outside the frame, -3 too small for the deepest tap or too large)
static int lp_rect_check(const LpNet& n, int H, int W, const int* r, int need_grad, LpLayout* L, int st = MGR_LPIPS_STORE_F32) {
    const long long x0 = r[0], y0 = r[1], w = r[2], h = r[3];
    if (w < 0 || h < 0) return -1;
    if (w == 0 || h == 0) return 0;
    if (x0 < 0 || y0 < 0 || x0 + w > W || y0 + h > H) return -2;
    return lp_layout(n, (int)h, (int)w, need_grad, L, 1, st) ? 1 : -3;
}

static int lp_rect_fail(const char* who, int rc) {
    return mgr_fail(MGR_EINVAL, "%s: %s", who,
                    rc == -1 ? "a rectangle has a negative size"
                             : rc == -2 ? "a rectangle is not inside the frame"
                                        : "a rectangle is too small for the deepest tap to have one pixel (or above 2^24 pixels)");
}

// The chunks of a windowed call: the non-empty views grouped by (w, h) in ascending view order, every group cut into runs of at
// most `cap` views; the chunks stand in the order of their first view.  cap = 1: one chunk per non-empty view.
struct LpChunk {
    int w, h, n;
    int view[LP_MAX_BATCH];
};

static void lp_chunks(int V, const int* rects, int cap, std::vector<LpChunk>* out) {
    out->clear();
    for (int v = 0; v < V; ++v) {
        const int w = rects[4 * v + 2], h = rects[4 * v + 3];
        if (w <= 0 || h <= 0) continue;
        LpChunk* c = nullptr;
        if (cap > 1)
            for (size_t j = out->size(); j-- > 0;)
                if ((*out)[j].w == w && (*out)[j].h == h) {        // the group's last chunk: the only one that may have room
                    if ((*out)[j].n < cap) c = &(*out)[j];
                    break;
                }
        if (!c) {
            out->push_back(LpChunk{w, h, 0, {}});
            c = &out->back();
        }
        c->view[c->n++] = v;
    }
}

static inline int lp_batch_cap(int max_batch) { return max_batch < LP_MAX_BATCH ? max_batch : LP_MAX_BATCH; }

// the largest chunk's workspace; 0 where a rectangle is refused
static size_t lp_chunks_bytes(const LpNet& n, const std::vector<LpChunk>& chunks, int need_grad, int st = MGR_LPIPS_STORE_F32) {
    size_t need = 0;
    for (const LpChunk& c : chunks) {
        LpLayout L;
        if (!lp_layout(n, c.h, c.w, need_grad, &L, (size_t)c.n, st)) return 0;
        need = need > L.total ? need : L.total;
    }
    return need;
}

static size_t lp_roi_bytes(const LpNet& n, int V, const int* rects, int need_grad, int cap, int st = MGR_LPIPS_STORE_F32) {
    for (int v = 0; v < V; ++v) {
        const int* r = rects + 4 * v;
        if (r[2] == 0 || r[3] == 0) continue;
        if (r[2] < 0 || r[3] < 0) return 0;
    }
    std::vector<LpChunk> chunks;
    lp_chunks(V, rects, cap, &chunks);
    return lp_chunks_bytes(n, chunks, need_grad, st);
}

extern "C" size_t mgr_lpips_roi_workspace_bytes(int net, int V, const int* rects, int need_grad) {
    LpNet n;
    if (!lp_net(net, &n) || V <= 0 || !rects) return 0;
    return lp_roi_bytes(n, V, rects, need_grad, 1);
}

extern "C" size_t mgr_lpips_roi_batch_workspace_bytes_st(int net, int V, const int* rects, int need_grad, int max_batch, int storage) {
    LpNet n;
    if (!lp_net(net, &n) || !lp_storage_ok(storage) || V <= 0 || !rects || max_batch < 1) return 0;
    return lp_roi_bytes(n, V, rects, need_grad, lp_batch_cap(max_batch), storage);
}

extern "C" size_t mgr_lpips_roi_batch_workspace_bytes(int net, int V, const int* rects, int need_grad, int max_batch) {
    return mgr_lpips_roi_batch_workspace_bytes_st(net, V, rects, need_grad, max_batch, MGR_LPIPS_STORE_F32);
}

extern "C" size_t mgr_lpips_taps_bytes_st(int net, int h, int w, int storage) {
    LpNet n;
    LpLayout L;
    if (!lp_net(net, &n) || !lp_storage_ok(storage) || !lp_layout(n, h, w, 0, &L, 1, storage)) return 0;
    return L.bufa - L.tap[0];
}

extern "C" size_t mgr_lpips_taps_bytes(int net, int h, int w) { return mgr_lpips_taps_bytes_st(net, h, w, MGR_LPIPS_STORE_F32); }

// view b's n floats at src + b n -> dst[b] + off (the taps of a chunk leave the batch-major workspace for the views' buffers)
struct LpTapOut {
    float* dst[LP_MAX_BATCH];
};

__global__ __launch_bounds__(LP_T) void k_lp_taps_out(size_t n, const float* __restrict__ src, const LpTapOut t, size_t off) {
    const size_t e = (size_t)blockIdx.x * LP_T + threadIdx.x;
    if (e < n) t.dst[blockIdx.y][off + e] = src[(size_t)blockIdx.y * n + e];
}

// the target tower of one chunk into its views' tap buffers; one view writes them directly (the one-view entry), more go through
// the workspace's batch-major tap regions
static int lp_taps_chunk(int operands, hipStream_t stream, const LpNet& n, const LpBlob& B, const char* blob, int H, int W, const int* rects,
                         const LpChunk& c, const float* target, const float* mask, int normalize, float* const* taps_out, char* ws,
                         int st = MGR_LPIPS_STORE_F32) {
    LpLayout L, L1;
    LpShape S;
    lp_layout(n, c.h, c.w, 0, &L, (size_t)c.n, st);
    lp_layout(n, c.h, c.w, 0, &L1, 1, st);
    lp_shapes(n, c.h, c.w, &S);
    LpWin win = {};
    win.FH = H;
    win.FW = W;
    for (int b = 0; b < c.n; ++b) {
        win.view[b] = c.view[b];
        win.x0[b] = rects[4 * c.view[b]];
        win.y0[b] = rects[4 * c.view[b] + 1];
    }
    void* tgt[13];
    int ci = 0;
    for (int i = 0; i < n.n_ops; ++i) {
        const LpOp& op = n.ops[i];
        if (!op.conv) continue;
        tgt[ci] = nullptr;
        if (op.tap >= 0)
            tgt[ci] = c.n == 1 ? (void*)((char*)taps_out[c.view[0]] + (L1.tap[op.tap] - L1.tap[0])) : (void*)(ws + L.tap[op.tap]);
        ++ci;
    }
    const int rc = lp_forward(operands, stream, n, B, blob, S, c.h, c.w, c.n, target, mask, normalize, tgt, ws + L.bufa, ws + L.bufb, &win,
                              st);
    if (rc != MGR_OK || c.n == 1) return rc;
    LpTapOut to = {};
    for (int b = 0; b < c.n; ++b) to.dst[b] = taps_out[c.view[b]];
    for (int i = 0; i < n.n_ops; ++i) {
        const LpOp& op = n.ops[i];
        if (!op.conv || op.tap < 0) continue;
        const size_t e = lp_tbytes(st, op.cout, S.h[i], S.w[i]) / 4;       // a view's tap in 4-byte words: the copy is by bytes
        hipLaunchKernelGGL(k_lp_taps_out, dim3((unsigned)((e + LP_T - 1) / LP_T), c.n), dim3(LP_T), 0, stream, e,
                           (const float*)(ws + L.tap[op.tap]), to, (L1.tap[op.tap] - L1.tap[0]) / 4);
        MGR_LAUNCH_CHECK("k_lp_taps_out", stream, 0);
    }
    return MGR_OK;
}

extern "C" int mgr_lpips_roi_taps_op(int net, int H, int W, const int* rect, const float* target_v, const float* mask_v, const void* blob_,
                                     size_t blob_bytes, int normalize, float* taps_out, void* workspace, size_t workspace_bytes,
                                     void* stream_, int operands) {
    hipStream_t stream = (hipStream_t)stream_;
    LpNet n;
    if (!lp_net(net, &n)) return mgr_fail(MGR_EINVAL, "mgr_lpips_roi_taps: net must be 0 (vgg) or 1 (alex)");
    if (!lp_operands_ok(operands)) return mgr_fail(MGR_EINVAL, "mgr_lpips_roi_taps: operands must be 0 (fp32) or 1 (bf16)");
    if (H <= 0 || W <= 0 || H > 65535) return mgr_fail(MGR_EINVAL, "mgr_lpips_roi_taps: bad sizes");
    if (!rect || !target_v || !blob_ || !taps_out || !workspace) return mgr_fail(MGR_EINVAL, "mgr_lpips_roi_taps: null pointer");
    LpLayout L;
    const int ok = lp_rect_check(n, H, W, rect, 0, &L);
    if (ok < 0) return lp_rect_fail("mgr_lpips_roi_taps", ok);
    if (ok == 0) return mgr_fail(MGR_EINVAL, "mgr_lpips_roi_taps: an empty rectangle has no taps");
    const LpBlob B = lp_blob(n, operands);
    if (blob_bytes != B.total) return mgr_fail(MGR_EINVAL, "mgr_lpips_roi_taps: blob_bytes is not mgr_lpips_net_bytes(net) of this operand mode");
    if (workspace_bytes < L.total) return mgr_fail(MGR_ENOMEM, "mgr_lpips_roi_taps: workspace smaller than mgr_lpips_workspace_bytes(net, h, w, 0)");
    const LpChunk c = {rect[2], rect[3], 1, {}};
    return lp_taps_chunk(operands, stream, n, B, (const char*)blob_, H, W, rect, c, target_v, mask_v, normalize, &taps_out, (char*)workspace);
}

extern "C" int mgr_lpips_roi_taps_batch_st(int net, int V, int H, int W, const int* rects, const float* target, const float* mask,
                                           const void* blob_, size_t blob_bytes, int normalize, float* const* taps_out, int max_batch,
                                           void* workspace, size_t workspace_bytes, void* stream_, int operands, int storage) {
    hipStream_t stream = (hipStream_t)stream_;
    LpNet n;
    if (!lp_net(net, &n)) return mgr_fail(MGR_EINVAL, "mgr_lpips_roi_taps_batch: net must be 0 (vgg) or 1 (alex)");
    if (!lp_operands_ok(operands)) return mgr_fail(MGR_EINVAL, "mgr_lpips_roi_taps_batch: operands must be 0 (fp32) or 1 (bf16)");
    if (const char* why = lp_storage_refusal(operands, storage)) return mgr_fail(MGR_EINVAL, "mgr_lpips_roi_taps_batch: %s", why);
    if (V <= 0 || H <= 0 || W <= 0 || H > 65535) return mgr_fail(MGR_EINVAL, "mgr_lpips_roi_taps_batch: bad sizes");
    if (max_batch < 1) return mgr_fail(MGR_EINVAL, "mgr_lpips_roi_taps_batch: max_batch must be at least 1");
    if (!rects || !target || !blob_ || !taps_out) return mgr_fail(MGR_EINVAL, "mgr_lpips_roi_taps_batch: null pointer");
    for (int v = 0; v < V; ++v) {
        LpLayout L;
        const int ok = lp_rect_check(n, H, W, rects + 4 * v, 0, &L, storage);
        if (ok < 0) return lp_rect_fail("mgr_lpips_roi_taps_batch", ok);
        if (ok && !taps_out[v]) return mgr_fail(MGR_EINVAL, "mgr_lpips_roi_taps_batch: null pointer (a non-empty view has no tap buffer)");
    }
    const LpBlob B = lp_blob(n, operands);
    if (blob_bytes != B.total)
        return mgr_fail(MGR_EINVAL, "mgr_lpips_roi_taps_batch: blob_bytes is not mgr_lpips_net_bytes(net) of this operand mode");
    std::vector<LpChunk> chunks;
    lp_chunks(V, rects, lp_batch_cap(max_batch), &chunks);
    const size_t need = lp_chunks_bytes(n, chunks, 0, storage);
    if (need && !workspace) return mgr_fail(MGR_EINVAL, "mgr_lpips_roi_taps_batch: null pointer");
    if (workspace_bytes < need)
        return mgr_fail(MGR_ENOMEM, "mgr_lpips_roi_taps_batch: workspace smaller than mgr_lpips_roi_batch_workspace_bytes(.., 0, max_batch)");
    for (const LpChunk& c : chunks) {
        // the one-view entry takes the view's own frame: chunk views index the call's frames here
        const int rc = lp_taps_chunk(operands, stream, n, B, (const char*)blob_, H, W, rects, c, target, mask, normalize, taps_out,
                                     (char*)workspace, storage);
        if (rc != MGR_OK) return rc;
    }
    return MGR_OK;
}

extern "C" int mgr_lpips_roi_taps_batch_op(int net, int V, int H, int W, const int* rects, const float* target, const float* mask,
                                           const void* blob, size_t blob_bytes, int normalize, float* const* taps_out, int max_batch,
                                           void* workspace, size_t workspace_bytes, void* stream, int operands) {
    return mgr_lpips_roi_taps_batch_st(net, V, H, W, rects, target, mask, blob, blob_bytes, normalize, taps_out, max_batch, workspace,
                                       workspace_bytes, stream, operands, MGR_LPIPS_STORE_F32);
}

// the windowed call, sequential (cap = 1) or batched
static int lp_roi_run(const char* who, int net, int V, int H, int W, const int* rects, const float* pred, const float* target,
                      const float* mask, const void* blob_, size_t blob_bytes, int normalize, const float* grad_scales, float* values,
                      float* dL_dpred, int accumulate, const float* const* target_taps, int max_batch, void* workspace,
                      size_t workspace_bytes, hipStream_t stream, int operands, int storage = MGR_LPIPS_STORE_F32) {
    LpNet n;
    if (!lp_net(net, &n)) return mgr_fail(MGR_EINVAL, "%s: net must be 0 (vgg) or 1 (alex)", who);
    if (!lp_operands_ok(operands)) return mgr_fail(MGR_EINVAL, "%s: operands must be 0 (fp32) or 1 (bf16)", who);
    if (const char* why = lp_storage_refusal(operands, storage)) return mgr_fail(MGR_EINVAL, "%s: %s", who, why);
    if (V <= 0 || H <= 0 || W <= 0 || H > 65535) return mgr_fail(MGR_EINVAL, "%s: bad sizes", who);
    if (max_batch < 1) return mgr_fail(MGR_EINVAL, "%s: max_batch must be at least 1", who);
    if (!rects || !pred || !blob_ || !values || (dL_dpred && !grad_scales)) return mgr_fail(MGR_EINVAL, "%s: null pointer", who);
    if (dL_dpred && !n.has_bwd) return mgr_fail(MGR_EINVAL, "%s: the AlexNet network is forward only (dL_dpred must be null)", who);
    const int need_grad = dL_dpred != nullptr;
    // every view is judged before the first launch
    for (int v = 0; v < V; ++v) {
        LpLayout L;
        const int ok = lp_rect_check(n, H, W, rects + 4 * v, need_grad, &L, storage);
        if (ok < 0) return lp_rect_fail(who, ok);
        if (ok == 0) continue;
        if (!target && !(target_taps && target_taps[v]))
            return mgr_fail(MGR_EINVAL, "%s: null pointer (a view has neither a target nor cached taps)", who);
    }
    const LpBlob B = lp_blob(n, operands);
    if (blob_bytes != B.total) return mgr_fail(MGR_EINVAL, "%s: blob_bytes is not mgr_lpips_net_bytes(net) of this operand mode", who);
    std::vector<LpChunk> chunks;
    lp_chunks(V, rects, lp_batch_cap(max_batch), &chunks);
    const size_t need = lp_chunks_bytes(n, chunks, need_grad, storage);
    if (need && !workspace) return mgr_fail(MGR_EINVAL, "%s: null pointer", who);
    if (workspace_bytes < need) return mgr_fail(MGR_ENOMEM, "%s: workspace smaller than %s_workspace_bytes", who, who);
    const size_t img = (size_t)3 * H * W;
    size_t next = 0;
    for (int v = 0; v < V; ++v) {
        const int* r = rects + 4 * v;
        if (r[2] == 0 || r[3] == 0) {
            // an empty view: the value is 0 (a fold over no partials); no gradient, and a written frame is zero
            float* dL = dL_dpred ? dL_dpred + v * img : nullptr;
            LpFoldArgs fa = {};
            hipLaunchKernelGGL(k_lp_fold, dim3(1), dim3(LP_T), 0, stream, fa, (const double*)nullptr, values + v);
            MGR_LAUNCH_CHECK("k_lp_fold", stream, 0);
            if (dL && !accumulate) {
                LpWin win = {};
                win.FH = H;
                win.FW = W;
                hipLaunchKernelGGL(k_lp_scale_bwd_win, dim3((W + LP_T - 1) / LP_T, H), dim3(LP_T), 0, stream, 0, 0, win,
                                   (const float*)nullptr, (const float*)nullptr, 0, 0, dL);
                MGR_LAUNCH_CHECK("k_lp_scale_bwd_win", stream, 0);
            }
            continue;
        }
        if (next >= chunks.size() || chunks[next].view[0] != v) continue;       // a later view of a chunk that has run
        const LpChunk& c = chunks[next++];
        LpWin win = {};
        win.FH = H;
        win.FW = W;
        const float* taps[LP_MAX_BATCH];
        float gs[LP_MAX_BATCH];
        for (int b = 0; b < c.n; ++b) {
            win.view[b] = c.view[b];
            win.x0[b] = rects[4 * c.view[b]];
            win.y0[b] = rects[4 * c.view[b] + 1];
            taps[b] = target_taps ? target_taps[c.view[b]] : nullptr;
            gs[b] = need_grad ? grad_scales[c.view[b]] : 0.f;
        }
        const int rc = lp_views(operands, stream, n, B, (const char*)blob_, c.h, c.w, c.n, &win, pred, target, mask, taps, normalize, gs,
                                values, dL_dpred, accumulate, (char*)workspace, storage);
        if (rc != MGR_OK) return rc;
    }
    return MGR_OK;
}

extern "C" int mgr_lpips_roi_op(int net, int V, int H, int W, const int* rects, const float* pred, const float* target, const float* mask,
                                const void* blob, size_t blob_bytes, int normalize, const float* grad_scales, float* values,
                                float* dL_dpred, int accumulate, const float* const* target_taps, void* workspace, size_t workspace_bytes,
                                void* stream, int operands) {
    return lp_roi_run("mgr_lpips_roi", net, V, H, W, rects, pred, target, mask, blob, blob_bytes, normalize, grad_scales, values, dL_dpred,
                      accumulate, target_taps, 1, workspace, workspace_bytes, (hipStream_t)stream, operands);
}

extern "C" int mgr_lpips_roi(int net, int V, int H, int W, const int* rects, const float* pred, const float* target, const float* mask,
                             const void* blob, size_t blob_bytes, int normalize, const float* grad_scales, float* values, float* dL_dpred,
                             int accumulate, const float* const* target_taps, void* workspace, size_t workspace_bytes, void* stream) {
    return mgr_lpips_roi_op(net, V, H, W, rects, pred, target, mask, blob, blob_bytes, normalize, grad_scales, values, dL_dpred, accumulate,
                            target_taps, workspace, workspace_bytes, stream, MGR_LPIPS_F32);
}

extern "C" int mgr_lpips_roi_batch_op(int net, int V, int H, int W, const int* rects, const float* pred, const float* target,
                                      const float* mask, const void* blob, size_t blob_bytes, int normalize, const float* grad_scales,
                                      float* values, float* dL_dpred, int accumulate, const float* const* target_taps, void* workspace,
                                      size_t workspace_bytes, void* stream, int operands, int max_batch) {
    return lp_roi_run("mgr_lpips_roi_batch", net, V, H, W, rects, pred, target, mask, blob, blob_bytes, normalize, grad_scales, values,
                      dL_dpred, accumulate, target_taps, max_batch, workspace, workspace_bytes, (hipStream_t)stream, operands);
}

extern "C" int mgr_lpips_roi_batch_st(int net, int V, int H, int W, const int* rects, const float* pred, const float* target,
                                      const float* mask, const void* blob, size_t blob_bytes, int normalize, const float* grad_scales,
                                      float* values, float* dL_dpred, int accumulate, const float* const* target_taps, void* workspace,
                                      size_t workspace_bytes, void* stream, int operands, int max_batch, int storage) {
    return lp_roi_run("mgr_lpips_roi_batch", net, V, H, W, rects, pred, target, mask, blob, blob_bytes, normalize, grad_scales, values,
                      dL_dpred, accumulate, target_taps, max_batch, workspace, workspace_bytes, (hipStream_t)stream, operands, storage);
}

extern "C" int mgr_lpips_roi_batch(int net, int V, int H, int W, const int* rects, const float* pred, const float* target,
                                   const float* mask, const void* blob, size_t blob_bytes, int normalize, const float* grad_scales,
                                   float* values, float* dL_dpred, int accumulate, const float* const* target_taps, void* workspace,
                                   size_t workspace_bytes, void* stream, int max_batch) {
    return mgr_lpips_roi_batch_op(net, V, H, W, rects, pred, target, mask, blob, blob_bytes, normalize, grad_scales, values, dL_dpred,
                                  accumulate, target_taps, workspace, workspace_bytes, stream, MGR_LPIPS_F32, max_batch);
}
