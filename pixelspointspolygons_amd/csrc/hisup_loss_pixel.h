// p3hip - per-pixel arithmetic of the five HiSup losses (models/hisup/model_hisup.py:241-245 = :302-306, sigmoid_l1_loss :27-37), shared by
// p3_hisup_val_loss (hisup_predict.hip: values) and p3_hisup_train_loss (hisup_loss.hip: values + gradients), and the layout of a workgroup's partials.
// A target never indexes anything: classes are selected by comparison, so any target value is safe (a jloc target outside {0, 1} counts as class 2 in
// the cross-entropy, a mask target is truncated to an integer and anything but 0 counts as class 1).
#pragma once
#include "p3_common.h"

namespace hisup_px {

constexpr int PIX = 1024;              // pixels per workgroup
constexpr int NPART = 6;               // partials per workgroup: CE jloc | CE mask | CE remask | L1 afm | masked |sigmoid(joff) - 0.5 - t| | junction pixels

__device__ __forceinline__ bool is_junction(int64_t tj) { return tj == 1 || tj == 2; }
__device__ __forceinline__ int mask_class(float t_mask) { return (int)(int64_t)t_mask; }        // targets['mask'].long()

// cross-entropy of one pixel = m + log(sum_c exp(l_c - m)) - l_t; e_c = exp(l_c - m) and their sum s come back for the softmax of the gradient
__device__ __forceinline__ float ce2(float l0, float l1, int t, float& e0, float& e1, float& s) {
    const float m = fmaxf(l0, l1);
    e0 = expf(l0 - m); e1 = expf(l1 - m);
    s = e0 + e1;
    return m + logf(s) - (t ? l1 : l0);
}
__device__ __forceinline__ float ce2(float l0, float l1, int t) {
    float e0, e1, s;
    return ce2(l0, l1, t, e0, e1, s);
}
__device__ __forceinline__ float ce3(float l0, float l1, float l2, int64_t t, float& e0, float& e1, float& e2, float& s) {
    const float m = fmaxf(l0, fmaxf(l1, l2));
    e0 = expf(l0 - m); e1 = expf(l1 - m); e2 = expf(l2 - m);
    s = e0 + e1 + e2;
    return m + logf(s) - (t == 0 ? l0 : (t == 1 ? l1 : l2));
}
__device__ __forceinline__ float ce3(float l0, float l1, float l2, int64_t t) {
    float e0, e1, e2, s;
    return ce3(l0, l1, l2, t, e0, e1, e2, s);
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }
// sigmoid_l1_loss's residual of one junction-pixel element: sigmoid(joff) - 0.5 - t_joff (its absolute value is the loss term)
__device__ __forceinline__ float joff_residual(float sig, float t) { return (sig - 0.5f) - t; }

}  // namespace hisup_px
