// The row Adam update shared by the pose chain (pose.hip: k_pose_adam) and the kinematic chain (fk.hip: k_fk_adam): one element,
// the arithmetic of k_sg_adam (torch.optim.SparseAdam), no clamp.  step_size = lr * sqrt(1 - beta2^step) / (1 - beta1^step),
// omb1 = 1 - beta1, omb2 = 1 - beta2, all rounded to fp32 by the host entry.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void pose_adam_one(float g, float* __restrict__ x, float* __restrict__ m_, float* __restrict__ v_,
                                              float step_size, float omb1, float omb2, float eps) {
    const float m0 = *m_, v0 = *v_;
    const float m = m0 + (g - m0) * omb1;
    const float v = v0 + (g * g - v0) * omb2;
    *m_ = m;
    *v_ = v;
    *x = *x - step_size * (m / (sqrtf(v) + eps));
}
