// The trilinear set-up shared by the skin-weight kernels (lbs_sh.hip) and the skin-grid gradient (skin_grid.hip):
// align_corners=True, u = (x,y,z) indexing (W,H,D), the base corner and the fractional parts of one Gaussian.
#pragma once
#include "mgr_common.h"

struct TriSetup {
    int x0, y0, z0;
    float fx, fy, fz;  // fractional parts
};

__device__ __forceinline__ TriSetup tri_setup(const float* __restrict__ xyz, int i,
                                              const float* __restrict__ center,
                                              const float* __restrict__ scale, int D, int H, int W) {
    TriSetup s;
    const float ux = (xyz[3 * i + 0] - center[0]) / scale[0];
    const float uy = (xyz[3 * i + 1] - center[1]) / scale[1];
    const float uz = (xyz[3 * i + 2] - center[2]) / scale[2];
    const float ix = ((ux + 1.0f) * 0.5f) * (float)(W - 1);
    const float iy = ((uy + 1.0f) * 0.5f) * (float)(H - 1);
    const float iz = ((uz + 1.0f) * 0.5f) * (float)(D - 1);
    const float flx = floorf(ix), fly = floorf(iy), flz = floorf(iz);
    // clamp far-away points so the int conversion is defined; they are out of
    // bounds either way and contribute zero
    s.x0 = (int)fminf(fmaxf(flx, -2.0f), (float)W + 1.0f);
    s.y0 = (int)fminf(fmaxf(fly, -2.0f), (float)H + 1.0f);
    s.z0 = (int)fminf(fmaxf(flz, -2.0f), (float)D + 1.0f);
    s.fx = ix - flx;
    s.fy = iy - fly;
    s.fz = iz - flz;
    return s;
}

#define SKIN_BP 24

__device__ __forceinline__ void tri_weights(const TriSetup& s, float Wk[8]) {
    const float wx[2] = {1.0f - s.fx, s.fx}, wy[2] = {1.0f - s.fy, s.fy}, wz[2] = {1.0f - s.fz, s.fz};
#pragma unroll
    for (int k = 0; k < 8; ++k) Wk[k] = wx[k & 1] * wy[(k >> 1) & 1] * wz[k >> 2];
}
