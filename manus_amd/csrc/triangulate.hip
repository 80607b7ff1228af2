// Robust multi-view triangulation of keypoints on the device (manus_amd/pose.py: triangulate_keypoints,
// KinematicPoseRefiner.triangulate): 2-D detections of C cameras and their projection matrices in, 3-D keypoints out, with a
// confidence and a per-detection inlier flag.  Deterministic consensus over camera PAIRS, no random sampling: what the reference
// does offline per frame and keypoint (preprocess/scripts/keypoints_3d.py through EasyMocap's iterative triangulation with
// dist_max = 25, min_conf = 0.1, min_view = 3) as one launch over the independent (frame, keypoint) problems.
//
// mgr_triangulate -- the whole algorithm, per problem (f, k), independent of every other problem.
//   Inputs: proj (C,3,4) with rows P0, P1, P2 of P_c; targets t (F,C,K,2); weights s (F,C,K); C <= MGR_TRI_MAX_CAMERAS = 64: camera c
//   is lane c of the problem's wave and a set of cameras is one 64-bit ballot.  Scalars are converted once: tau, min_conf, z_min
//   and det_min to float for the fp32 parts, det_min stays double for the fp64 solves.  All fp32 arithmetic below is
//   uncontracted (no fma), every sum written a + b + c is taken left to right.
//
//   ACTIVE.  Camera c is active iff  s > (float)min_conf  (a NaN weight is not; min_conf >= 0, so a weight not > 0 never is),
//   both target coordinates are finite, and both plane norms below are finite and > 0.  What an inactive camera holds never
//   enters a result.
//
//   PLANES (fp32, lane c).  a_u = t_x P2 - P0 and a_v = t_y P2 - P1 (4-vectors); |a|_3 = sqrt(a0^2 + a1^2 + a2^2);
//   (n_u, d_u) = a_u / |a_u|_3 and (n_v, d_v) = a_v / |a_v|_3, four divisions each: the two planes through the camera centre
//   that hold the detection's ray, with residuals n.X + d in world units -- the 3x3 normal matrix below is conditioned by the
//   rig's geometry alone (pixel-unit DLT rows would square a condition number of about 10^3).
//   Per camera  M_c = n_u n_u^T + n_v n_v^T  (six entries, each nu_i nu_j + nv_i nv_j)  and  m_c = -(d_u n_u + d_v n_v).
//
//   solve(N, b, det_min) for a symmetric N: the cofactors c00 = N11 N22 - N12 N12, c01 = N02 N12 - N01 N22, c02 = N01 N12 - N02 N11,
//   c11 = N00 N22 - N02 N02, c12 = N01 N02 - N00 N12, c22 = N00 N11 - N01 N01; det = N00 c00 + N01 c01 + N02 c02;
//   m = (N00 + N11 + N22) / 3; ACCEPTED iff det > det_min (m m) m (a NaN is rejected); X_i = (c_i0 b0 + c_i1 b1 + c_i2 b2) / det.
//
//   CLASSIFICATION of camera c at X (fp32, lane c).  q_i = P_i0 X0 + P_i1 X1 + P_i2 X2 + P_i3; u = (q0 / q2, q1 / q2);
//   r = u - t_c; d_c(X) = sqrt(r0 r0 + r1 r1); front_c = active and q2 > (float)z_min; inlier_c(X) = front_c and d_c < (float)tau.
//   inliers(X) is the ballot of inlier_c, its size a popcount.
//
//   SEED (fp32).  The pairs a < b of active cameras are walked in lexicographic order.  X_ab = solve(M_a + M_b, m_a + m_b,
//   (float)det_min), every lane forming the same X_ab from the plane table in LDS; the pair is accepted iff the solve is and
//   front_a(X_ab) and front_b(X_ab) hold.  count_ab = |inliers(X_ab)|.  The seed is the FIRST accepted pair with the maximal
//   count.  No accepted pair: the problem is invalid.
//
//   REFIT, refit_rounds (>= 1) times.  S = inliers(X); |S| < 2: invalid.  N = sum_{c in S} s_c M_c and b = sum_{c in S} s_c m_c
//   with every product formed in fp64 from the fp32 planes -- (double)s ((double)nu_i (double)nu_j + (double)nv_i (double)nv_j),
//   -(double)s ((double)d_u (double)nu_i + (double)d_v (double)nv_i) -- and the nine sums taken in fp64 over c = 0, 1, .., C - 1 in
//   ascending order (a camera outside S adds an exact 0): an order that depends on C alone.  solve(N, b, det_min) in fp64;
//   rejected: invalid; otherwise X = the solution rounded to fp32.  After the rounds S = inliers(X) is the FINAL SET;
//   |S| < min_views: invalid.
//
//   POLISH, gn_iters (>= 0) Gauss-Newton steps on sum_{c in S} s_c |u_c(X) - t_c|^2 over the fixed final set.  Lane c, fp32:
//   q, u, r as in the classification; J0 = (P0[:3] - u0 P2[:3]) / q2, J1 = (P1[:3] - u1 P2[:3]) / q2.  H = sum s (J0_i J0_j + J1_i J1_j)
//   and g = sum s (J0_i r0 + J1_i r1), products and sums in fp64 in the refit's order.  solve(H, g, det_min) in fp64 gives the
//   step e; rejected (a NaN included): the polish ends and X stays; otherwise X = (float)((double)X - e).
//
//   OUTPUTS.  xyz[f,k] = X after the polish; n_inliers[f,k] = |S|; inliers[f,c,k] = S as 0 / 1 bytes -- the set the fit used,
//   classified BEFORE the polish; conf[f,k] = (float)(sum_{c in S} (double)s_c / |S|), the sum in the refit's order (the
//   reference's conf3d); dist[f,c,k] = d_c at the FINAL X, after the polish, where front_c holds there, NaN otherwise.  A camera
//   of S can so carry a dist >= tau, or NaN, if the polish moved X across its threshold.
//   An INVALID problem gives xyz = NaN, conf = 0, n_inliers = 0, inliers = 0 and dist = NaN, and nothing else is written for it.
//
// Layout (the plain one): one wave per problem, four problems per workgroup.  P_c, t_c, s_c and the two planes stay in lane c's
// registers -- no lane ever needs another camera's projection --; the seed's table (M_c, m_c: nine floats in a 48-byte slot per
// camera) sits in LDS and the wave reads camera b's slot at a wave-uniform address.  The active set, the front set and the inlier
// set are ballots; the pair loops walk the set bits of the active ballot in scalar registers.  The refit's and polish's nine
// fp64 sums go through LDS: every lane stores its terms, then every lane adds the C columns in ascending order and so holds
// the totals itself.  No atomics, no workspace, no scratch.  The workgroup barriers around the LDS exchanges are reached by all
// four waves the same number of times, whatever their problems do: an invalid problem (or a wave past the last problem) keeps
// walking with an empty set and writes at the end.
#include <cmath>

#include "mgr_common.h"

#define TRI_WAVES 4
#define TRI_BLOCK (TRI_WAVES * MGR_WAVE)
#define TRI_SLOT 12           // floats per camera of the seed's table: M00 M01 M02 M11 M12 M22 m0 m1 m2 and three of padding
#define TRI_SUMS 9            // fp64 sums of one reduction: six of the symmetric matrix, three of the right side

struct TriParams {
    float tau, min_conf, z_min, det_min;
    double det_min_d;
    int min_views, refit_rounds, gn_iters;
};

// solve(N, b, det_min) of the header: N = (N00, N01, N02, N11, N12, N22)
template <typename T>
__device__ __forceinline__ bool tri_solve(const T (&N)[6], const T (&b)[3], T det_min, T (&X)[3]) {
#pragma clang fp contract(off)
    const T c00 = N[3] * N[5] - N[4] * N[4], c01 = N[2] * N[4] - N[1] * N[5], c02 = N[1] * N[4] - N[2] * N[3];
    const T c11 = N[0] * N[5] - N[2] * N[2], c12 = N[1] * N[2] - N[0] * N[4], c22 = N[0] * N[3] - N[1] * N[1];
    const T det = (N[0] * c00 + N[1] * c01) + N[2] * c02;
    const T m = ((N[0] + N[3]) + N[5]) / (T)3;
    if (!(det > det_min * ((m * m) * m))) return false;
    X[0] = ((c00 * b[0] + c01 * b[1]) + c02 * b[2]) / det;
    X[1] = ((c01 * b[0] + c11 * b[1]) + c12 * b[2]) / det;
    X[2] = ((c02 * b[0] + c12 * b[1]) + c22 * b[2]) / det;
    return true;
}

struct TriView {              // camera c at X: q2, the pixel u, the residual r = u - t and its length
    float q2, u0, u1, r0, r1, d;
};

__device__ __forceinline__ TriView tri_view(const float (&P)[12], float tx, float ty, const float (&X)[3]) {
#pragma clang fp contract(off)
    TriView v;
    const float q0 = ((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[3];
    const float q1 = ((P[4] * X[0] + P[5] * X[1]) + P[6] * X[2]) + P[7];
    v.q2 = ((P[8] * X[0] + P[9] * X[1]) + P[10] * X[2]) + P[11];
    v.u0 = q0 / v.q2;
    v.u1 = q1 / v.q2;
    v.r0 = v.u0 - tx;
    v.r1 = v.u1 - ty;
    v.d = sqrtf(v.r0 * v.r0 + v.r1 * v.r1);
    return v;
}

// Every lane's nine terms -> every lane the nine sums over the columns c = 0 .. C - 1 in ascending order.  Both barriers are
// reached by the whole workgroup: callers are in wave-uniform, workgroup-uniform control flow.
__device__ __forceinline__ void tri_sums(double (&v)[TRI_SUMS], double* __restrict__ red, int lane, int C) {
#pragma unroll
    for (int i = 0; i < TRI_SUMS; ++i) red[i * MGR_WAVE + lane] = v[i];
    __syncthreads();
    double acc[TRI_SUMS];
#pragma unroll
    for (int i = 0; i < TRI_SUMS; ++i) acc[i] = 0.0;
    for (int c = 0; c < C; ++c) {
#pragma unroll
        for (int i = 0; i < TRI_SUMS; ++i) acc[i] += red[i * MGR_WAVE + c];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TRI_SUMS; ++i) v[i] = acc[i];
}

__global__ __launch_bounds__(TRI_BLOCK) void k_triangulate(int F, int C, int K, const float* __restrict__ proj,
                                                           const float* __restrict__ targets, const float* __restrict__ weights,
                                                           TriParams pr, float* __restrict__ xyz, float* __restrict__ conf,
                                                           int32_t* __restrict__ n_inliers, uint8_t* __restrict__ inliers,
                                                           float* __restrict__ dist) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float s_tab[TRI_WAVES][MGR_WAVE * TRI_SLOT];
    __shared__ double s_red[TRI_WAVES][TRI_SUMS * MGR_WAVE];
    const int lane = threadIdx.x & (MGR_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / MGR_WAVE));
    const long long problem = (long long)blockIdx.x * TRI_WAVES + wave;
    const bool exists = problem < (long long)F * K;               // wave-uniform
    const int f = exists ? (int)(problem / K) : 0, k = exists ? (int)(problem % K) : 0;
    const bool cam = exists && lane < C;
    const size_t det_idx = ((size_t)f * C + (cam ? lane : 0)) * K + k;      // of (f, lane, k) in the (F,C,K) tables
    float* tab = s_tab[wave];
    double* red = s_red[wave];
    const float nanf_ = __int_as_float(0x7fc00000);

    // ---- this lane's camera: projection, detection, planes ----
    float P[12], tx = 0.0f, ty = 0.0f, s = 0.0f;
#pragma unroll
    for (int i = 0; i < 12; ++i) P[i] = cam ? proj[(size_t)lane * 12 + i] : 0.0f;
    if (cam) {
        s = weights[det_idx];
        tx = targets[det_idx * 2 + 0];
        ty = targets[det_idx * 2 + 1];
    }
    bool active = cam && s > pr.min_conf && isfinite(tx) && isfinite(ty);
    float nu[3], nv[3], du, dv;
    {
        float au[4], av[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            au[i] = tx * P[8 + i] - P[i];
            av[i] = ty * P[8 + i] - P[4 + i];
        }
        const float lu = sqrtf((au[0] * au[0] + au[1] * au[1]) + au[2] * au[2]);
        const float lv = sqrtf((av[0] * av[0] + av[1] * av[1]) + av[2] * av[2]);
        active = active && isfinite(lu) && lu > 0.0f && isfinite(lv) && lv > 0.0f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            nu[i] = active ? au[i] / lu : 0.0f;
            nv[i] = active ? av[i] / lv : 0.0f;
        }
        du = active ? au[3] / lu : 0.0f;
        dv = active ? av[3] / lv : 0.0f;
    }
    if (!active) {             // nothing an inactive camera holds is read into a result
        s = 0.0f;
        tx = 0.0f;
        ty = 0.0f;
    }
    {
        float4* slot = reinterpret_cast<float4*>(tab + lane * TRI_SLOT);
        slot[0] = make_float4(nu[0] * nu[0] + nv[0] * nv[0], nu[0] * nu[1] + nv[0] * nv[1], nu[0] * nu[2] + nv[0] * nv[2],
                              nu[1] * nu[1] + nv[1] * nv[1]);
        slot[1] = make_float4(nu[1] * nu[2] + nv[1] * nv[2], nu[2] * nu[2] + nv[2] * nv[2], -(du * nu[0] + dv * nv[0]),
                              -(du * nu[1] + dv * nv[1]));
        slot[2] = make_float4(-(du * nu[2] + dv * nv[2]), 0.0f, 0.0f, 0.0f);
    }
    __syncthreads();
    const unsigned long long act = __builtin_amdgcn_ballot_w64(active);
    const unsigned long long me = 1ull << lane;

    // ---- seed: the first accepted pair with the most inliers ----
    bool valid = false;
    int best = -1;
    float X[3] = {0.0f, 0.0f, 0.0f};
    for (unsigned long long ra = act; ra != 0ull; ra &= ra - 1ull) {
        const int a = __builtin_ctzll(ra);
        const float4* sa = reinterpret_cast<const float4*>(tab + a * TRI_SLOT);
        const float4 a0 = sa[0], a1 = sa[1], a2 = sa[2];
        for (unsigned long long rb = ra & (ra - 1ull); rb != 0ull; rb &= rb - 1ull) {
            const int b = __builtin_ctzll(rb);
            const float4* sb = reinterpret_cast<const float4*>(tab + b * TRI_SLOT);
            const float4 b0 = sb[0], b1 = sb[1], b2 = sb[2];
            const float N[6] = {a0.x + b0.x, a0.y + b0.y, a0.z + b0.z, a0.w + b0.w, a1.x + b1.x, a1.y + b1.y};
            const float rhs[3] = {a1.z + b1.z, a1.w + b1.w, a2.x + b2.x};
            float Y[3];
            if (!tri_solve<float>(N, rhs, pr.det_min, Y)) continue;
            const TriView v = tri_view(P, tx, ty, Y);
            const bool front = active && v.q2 > pr.z_min;
            const unsigned long long fm = __builtin_amdgcn_ballot_w64(front);
            if (((fm >> a) & (fm >> b) & 1ull) == 0ull) continue;
            const int count = __builtin_popcountll(__builtin_amdgcn_ballot_w64(front && v.d < pr.tau));
            if (count > best) {
                best = count;
                valid = true;
                X[0] = Y[0];
                X[1] = Y[1];
                X[2] = Y[2];
            }
        }
    }

    // ---- refit on the inliers of X, weighted by the confidences ----
    const double sd = (double)s;
    const double nud[3] = {(double)nu[0], (double)nu[1], (double)nu[2]}, nvd[3] = {(double)nv[0], (double)nv[1], (double)nv[2]};
    const double dud = (double)du, dvd = (double)dv;
    unsigned long long S = 0ull;
    for (int round = 0; round <= pr.refit_rounds; ++round) {
        const TriView v = tri_view(P, tx, ty, X);
        S = valid ? __builtin_amdgcn_ballot_w64(active && v.q2 > pr.z_min && v.d < pr.tau) : 0ull;
        if (round == pr.refit_rounds) break;                      // the final set
        if (__builtin_popcountll(S) < 2) valid = false;
        const double w = (valid && (S & me)) ? sd : 0.0;
        double t[TRI_SUMS] = {w * (nud[0] * nud[0] + nvd[0] * nvd[0]), w * (nud[0] * nud[1] + nvd[0] * nvd[1]),
                              w * (nud[0] * nud[2] + nvd[0] * nvd[2]), w * (nud[1] * nud[1] + nvd[1] * nvd[1]),
                              w * (nud[1] * nud[2] + nvd[1] * nvd[2]), w * (nud[2] * nud[2] + nvd[2] * nvd[2]),
                              -(w * (dud * nud[0] + dvd * nvd[0])), -(w * (dud * nud[1] + dvd * nvd[1])),
                              -(w * (dud * nud[2] + dvd * nvd[2]))};
        tri_sums(t, red, lane, C);
        const double N[6] = {t[0], t[1], t[2], t[3], t[4], t[5]}, rhs[3] = {t[6], t[7], t[8]};
        double Y[3];
        if (valid && tri_solve<double>(N, rhs, pr.det_min_d, Y)) {
            X[0] = (float)Y[0];
            X[1] = (float)Y[1];
            X[2] = (float)Y[2];
        } else {
            valid = false;
        }
    }
    const int n = __builtin_popcountll(S);
    if (n < pr.min_views) valid = false;
    if (!valid) S = 0ull;
    const bool mine = (S & me) != 0ull;

    // ---- polish: Gauss-Newton on the weighted reprojection error over the fixed set ----
    bool polishing = valid;
    for (int it = 0; it < pr.gn_iters; ++it) {
        const TriView v = tri_view(P, tx, ty, X);
        float J0[3], J1[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            J0[i] = (P[i] - v.u0 * P[8 + i]) / v.q2;
            J1[i] = (P[4 + i] - v.u1 * P[8 + i]) / v.q2;
        }
        const bool on = polishing && mine;
        const double w = on ? sd : 0.0;
        const double a[3] = {on ? (double)J0[0] : 0.0, on ? (double)J0[1] : 0.0, on ? (double)J0[2] : 0.0};
        const double b[3] = {on ? (double)J1[0] : 0.0, on ? (double)J1[1] : 0.0, on ? (double)J1[2] : 0.0};
        const double r0 = on ? (double)v.r0 : 0.0, r1 = on ? (double)v.r1 : 0.0;
        double t[TRI_SUMS] = {w * (a[0] * a[0] + b[0] * b[0]), w * (a[0] * a[1] + b[0] * b[1]), w * (a[0] * a[2] + b[0] * b[2]),
                              w * (a[1] * a[1] + b[1] * b[1]), w * (a[1] * a[2] + b[1] * b[2]), w * (a[2] * a[2] + b[2] * b[2]),
                              w * (a[0] * r0 + b[0] * r1), w * (a[1] * r0 + b[1] * r1), w * (a[2] * r0 + b[2] * r1)};
        tri_sums(t, red, lane, C);
        const double H[6] = {t[0], t[1], t[2], t[3], t[4], t[5]}, g[3] = {t[6], t[7], t[8]};
        double e[3];
        if (polishing && tri_solve<double>(H, g, pr.det_min_d, e)) {
            X[0] = (float)((double)X[0] - e[0]);
            X[1] = (float)((double)X[1] - e[1]);
            X[2] = (float)((double)X[2] - e[2]);
        } else {
            polishing = false;
        }
    }

    // ---- the confidence: the mean weight of the set, summed in the refit's order ----
    double t[TRI_SUMS] = {mine ? sd : 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    tri_sums(t, red, lane, C);
    if (!exists) return;
    const size_t row = (size_t)problem;
    if (lane == 0) {
        xyz[row * 3 + 0] = valid ? X[0] : nanf_;
        xyz[row * 3 + 1] = valid ? X[1] : nanf_;
        xyz[row * 3 + 2] = valid ? X[2] : nanf_;
        conf[row] = valid ? (float)(t[0] / (double)n) : 0.0f;
        n_inliers[row] = valid ? n : 0;
    }
    if (cam) {
        if (inliers) inliers[det_idx] = mine ? 1 : 0;
        if (dist) {
            const TriView v = tri_view(P, tx, ty, X);
            dist[det_idx] = (valid && active && v.q2 > pr.z_min) ? v.d : nanf_;
        }
    }
}

// ---------------------------------------------------------------------------
// host entry: every refusal is decided on the arguments, before any launch
// ---------------------------------------------------------------------------
extern "C" int mgr_triangulate(int F, int C, int K, const float* proj, const float* targets, const float* weights, double tau,
                               double min_conf, int min_views, double z_min, double det_min, int refit_rounds, int gn_iters, float* xyz,
                               float* conf, int32_t* n_inliers, uint8_t* inliers, float* dist, void* stream_) {
    if (F < 1 || C < 1 || K < 1) return mgr_fail(MGR_EINVAL, "mgr_triangulate: F, C and K must be at least 1");
    if (C > MGR_TRI_MAX_CAMERAS) return mgr_fail(MGR_EINVAL, "mgr_triangulate: C above MGR_TRI_MAX_CAMERAS (a camera is a lane of one wave)");
    if (!proj || !targets || !weights || !xyz || !conf || !n_inliers) return mgr_fail(MGR_EINVAL, "mgr_triangulate: null pointer");
    if (!(tau > 0.0) || !std::isfinite(tau)) return mgr_fail(MGR_EINVAL, "mgr_triangulate: tau must be finite and > 0");
    if (!(z_min > 0.0) || !std::isfinite(z_min)) return mgr_fail(MGR_EINVAL, "mgr_triangulate: z_min must be finite and > 0");
    if (!(det_min > 0.0) || !std::isfinite(det_min)) return mgr_fail(MGR_EINVAL, "mgr_triangulate: det_min must be finite and > 0");
    if (!(min_conf >= 0.0) || !std::isfinite(min_conf)) return mgr_fail(MGR_EINVAL, "mgr_triangulate: min_conf must be finite and >= 0");
    if (min_views < 2) return mgr_fail(MGR_EINVAL, "mgr_triangulate: min_views must be at least 2");
    if (refit_rounds < 1) return mgr_fail(MGR_EINVAL, "mgr_triangulate: refit_rounds must be at least 1");
    if (gn_iters < 0) return mgr_fail(MGR_EINVAL, "mgr_triangulate: gn_iters must be at least 0");
    if ((long long)F * K > (1ll << 30)) return mgr_fail(MGR_EINVAL, "mgr_triangulate: F * K above 2^30");
    hipStream_t stream = (hipStream_t)stream_;
    const TriParams pr = {(float)tau, (float)min_conf, (float)z_min, (float)det_min, det_min, min_views, refit_rounds, gn_iters};
    const long long problems = (long long)F * K;
    {
        MGR_PROF("k_triangulate", stream);
        hipLaunchKernelGGL(k_triangulate, dim3((unsigned)((problems + TRI_WAVES - 1) / TRI_WAVES)), dim3(TRI_BLOCK), 0, stream, F, C, K, proj,
                           targets, weights, pr, xyz, conf, n_inliers, inliers, dist);
    }
    MGR_LAUNCH_CHECK("k_triangulate", stream, 0);
    return MGR_OK;
}
