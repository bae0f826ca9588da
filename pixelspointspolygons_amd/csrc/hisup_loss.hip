// p3hip HiSup training losses with their gradients (models/hisup/model_hisup.py:302-306 `EncoderDecoder.forward_train`, sigmoid_l1_loss :27-37,
// weighted as train/trainer_hisup.py:31-39 `LossReducer`): p3_hisup_train_loss = the five losses, their weighted total and d total / d map for the
// five head maps, in three launches (two without gradients):
//   junction_count_kernel   grid (ceil(HW / 4096), B): junction pixels of each slice of t_jloc -> int32 counts.  The joff gradient of a pixel is
//                           scaled by H*W / c_b, c_b = the image's junction pixels, which is known only after a reduction; t_jloc is 8 of the 72
//                           bytes a pixel reads, and the second read behind this pass comes out of the cache.
//   train_loss_kernel       grid (ceil(HW / 1024), B): one pass over the pixels; each lane owns FOUR consecutive pixels, so that NCHW planes move as
//                           16-byte accesses; every logit and target is read once, every gradient written once, six fp32 partials per workgroup.
//   train_loss_final_kernel one workgroup: partials summed in a fixed order in float64 -> losses[6].
// Maps are addressed as base[b*sb + c*sc + pix*sp] (p3hip.h, "HiSup inference after the heads"); each map takes the widest access its strides and
// addresses allow (map_mode below), else element accesses - e.g. H*W = 37 * 41 = 1517, whose planes are not 16-byte aligned.
// No floating-point atomics, nothing data dependent in the launch sequence; every output repeats bit for bit.
#include "p3_common.h"
#include "hisup_loss_pixel.h"

namespace {

using namespace hisup_px;

constexpr int CNT_PIX = 4096;          // pixels per workgroup of the count pass
constexpr int64_t MAX_HW = 1 << 22;

typedef long long i64x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

enum { MODE_ELEM = 0, MODE_PLANE4 = 1, MODE_ROW2 = 2 };

struct Map {
    const float* p;                    // logits
    float* g;                          // gradient, same strides (unused without gradients)
    int64_t sb, sc, sp;
    int mode;
};

struct Args {
    Map jloc, joff, mask, afm, remask;
    const int64_t* t_jloc;
    const float *t_joff, *t_mask, *t_afm;
    int HW, tvec;                      // tvec: the four target arrays take 16-byte accesses
    float k_jloc, k_mask, k_remask, k_afm;      // w / N, w / N, w / N, w / 2N
    double k_joff;                     // w / 2N
    const int32_t* cnt;                // [B, ncb] junction counts of the count pass
    int ncb;
    float* parts;                      // [B, gridDim.x, NPART]
};

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- count pass: cnt[b, blockIdx.x] = junction pixels among pixels [blockIdx.x * CNT_PIX, + CNT_PIX) of image b
__global__ __launch_bounds__(256) void junction_count_kernel(const int64_t* __restrict__ t_jloc, int HW, int vec, int32_t* __restrict__ cnt) {
    __shared__ int red[4];
    const int64_t* t = t_jloc + (int64_t)blockIdx.y * HW;
    const int p0 = blockIdx.x * CNT_PIX;
    int n = 0;
#pragma unroll
    for (int i = 0; i < CNT_PIX / 512; ++i) {
        const int pix = p0 + (i * 256 + (int)threadIdx.x) * 2;
        if (vec && pix + 1 < HW) {                       // vec: HW even and the base 16-byte aligned
            const i64x2 q = *(const i64x2*)(t + pix);
            n += (int)is_junction(q.x) + (int)is_junction(q.y);
        } else {
            if (pix < HW) n += (int)is_junction(t[pix]);
            if (pix + 1 < HW) n += (int)is_junction(t[pix + 1]);
        }
    }
    n = wave_sum_i(n);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) cnt[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- the N channels of a lane's four pixels [pix0, pix0 + nv), nv in 1..4
template <int N>
__device__ __forceinline__ void load_map(const Map& m, int b, int pix0, int nv, float (&v)[N][4]) {
    const float* base = m.p + (int64_t)b * m.sb;
    if (m.mode == MODE_PLANE4) {                         // nv == 4 (HW % 4 == 0)
#pragma unroll
        for (int c = 0; c < N; ++c) {
            const f32x4 q = *(const f32x4*)(base + c * m.sc + pix0);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[c][k] = q[k];
        }
    } else if (m.mode == MODE_ROW2) {                    // channels adjacent, every pixel's first channel 8-byte aligned
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float* r = base + (int64_t)(pix0 + k) * m.sp;
            f32x2 q = {0.f, 0.f};
            float t = 0.f;
            if (k < nv) {
                q = *(const f32x2*)r;
                if (N == 3) t = r[2];
            }
            v[0][k] = q[0]; v[1][k] = q[1];
            if (N == 3) v[N - 1][k] = t;
        }
    } else {
#pragma unroll
        for (int c = 0; c < N; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k) v[c][k] = k < nv ? base[c * m.sc + (int64_t)(pix0 + k) * m.sp] : 0.f;
    }
}

// only the N valid channels of the valid pixels are written
template <int N>
__device__ __forceinline__ void store_map(const Map& m, int b, int pix0, int nv, const float (&v)[N][4]) {
    float* base = m.g + (int64_t)b * m.sb;
    if (m.mode == MODE_PLANE4) {
#pragma unroll
        for (int c = 0; c < N; ++c) {
            const f32x4 q = {v[c][0], v[c][1], v[c][2], v[c][3]};
            *(f32x4*)(base + c * m.sc + pix0) = q;
        }
    } else if (m.mode == MODE_ROW2) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < nv) {
                float* r = base + (int64_t)(pix0 + k) * m.sp;
                const f32x2 q = {v[0][k], v[1][k]};
                *(f32x2*)r = q;
                if (N == 3) r[2] = v[N - 1][k];
            }
    } else {
#pragma unroll
        for (int c = 0; c < N; ++c)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nv) base[c * m.sc + (int64_t)(pix0 + k) * m.sp] = v[c][k];
    }
}

// a contiguous fp32 target plane
__device__ __forceinline__ void load_target(const float* __restrict__ plane, int pix0, int nv, int vec, float (&v)[4]) {
    if (vec) {
        const f32x4 q = *(const f32x4*)(plane + pix0);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = q[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = k < nv ? plane[pix0 + k] : 0.f;
    }
}

__device__ __forceinline__ float signf(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }       // torch.abs's gradient: sign(0) = 0

// grid (ceil(HW / PIX), B), 256 lanes, lane owns pixels [pix0, pix0 + 4).  GRAD = false computes the same partials from the same instructions in the same
// order, so the values do not depend on whether gradients were asked for.
template <bool GRAD>
__global__ __launch_bounds__(256) void train_loss_kernel(const Args a) {
    __shared__ float red[4][NPART];
    __shared__ int cred[4];
    const int b = blockIdx.y, HW = a.HW;
    const int pix0 = blockIdx.x * PIX + (int)threadIdx.x * 4;
    const int nv = min(4, HW - pix0);                    // <= 0: nothing to do but the reductions

    float joff_scale = 0.f;                              // w_joff / 2N * HW / c_b; an image without junctions has no junction pixel to scale
    if (GRAD) {
        int c = 0;
        for (int i = threadIdx.x; i < a.ncb; i += 256) c += a.cnt[(int64_t)b * a.ncb + i];
        c = wave_sum_i(c);
        if ((threadIdx.x & 63) == 0) cred[threadIdx.x >> 6] = c;
        __syncthreads();
        const int cb = (cred[0] + cred[1]) + (cred[2] + cred[3]);
        if (cb > 0) joff_scale = (float)(a.k_joff * (double)HW / (double)cb);
    }

    float acc[NPART] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (nv > 0) {
        int64_t tj[4];
        float tm[4];
        {
            const int64_t* t = a.t_jloc + (int64_t)b * HW + pix0;
            if (a.tvec) {
                const i64x2 q0 = *(const i64x2*)t, q1 = *(const i64x2*)(t + 2);
                tj[0] = q0.x; tj[1] = q0.y; tj[2] = q1.x; tj[3] = q1.y;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) tj[k] = k < nv ? t[k] : 0;
            }
            load_target(a.t_mask + (int64_t)b * HW, pix0, nv, a.tvec, tm);
        }
        {   // ---- jloc: 3-class cross-entropy, gradient w / N * (softmax - onehot)
            float l[3][4], g[3][4];
            load_map<3>(a.jloc, b, pix0, nv, l);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nv) {
                    float e0, e1, e2, s;
                    acc[0] += ce3(l[0][k], l[1][k], l[2][k], tj[k], e0, e1, e2, s);
                    if (GRAD) {
                        const float inv = 1.f / s;
                        g[0][k] = a.k_jloc * (e0 * inv - (tj[k] == 0 ? 1.f : 0.f));
                        g[1][k] = a.k_jloc * (e1 * inv - (tj[k] == 1 ? 1.f : 0.f));
                        g[2][k] = a.k_jloc * (e2 * inv - (tj[k] == 0 || tj[k] == 1 ? 0.f : 1.f));
                    }
                }
            if (GRAD) store_map<3>(a.jloc, b, pix0, nv, g);
        }
#pragma unroll
        for (int which = 0; which < 2; ++which) {   // ---- mask, remask: 2-class cross-entropy against (int64) t_mask
            const Map& m = which == 0 ? a.mask : a.remask;
            const float kw = which == 0 ? a.k_mask : a.k_remask;
            float l[2][4], g[2][4];
            load_map<2>(m, b, pix0, nv, l);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nv) {
                    const int t = mask_class(tm[k]);
                    float e0, e1, s;
                    acc[1 + which] += ce2(l[0][k], l[1][k], t, e0, e1, s);
                    if (GRAD) {
                        const float inv = 1.f / s;
                        g[0][k] = kw * (e0 * inv - (t ? 0.f : 1.f));
                        g[1][k] = kw * (e1 * inv - (t ? 1.f : 0.f));
                    }
                }
            if (GRAD) store_map<2>(m, b, pix0, nv, g);
        }
        {   // ---- afm: L1, gradient w / 2N * sign(afm - t)
            float l[2][4], g[2][4], t[2][4];
            load_map<2>(a.afm, b, pix0, nv, l);
            load_target(a.t_afm + (int64_t)b * 2 * HW, pix0, nv, a.tvec, t[0]);
            load_target(a.t_afm + (int64_t)b * 2 * HW + HW, pix0, nv, a.tvec, t[1]);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nv) {
                    const float d0 = l[0][k] - t[0][k], d1 = l[1][k] - t[1][k];
                    acc[3] += fabsf(d0) + fabsf(d1);
                    if (GRAD) { g[0][k] = a.k_afm * signf(d0); g[1][k] = a.k_afm * signf(d1); }
                }
            if (GRAD) store_map<2>(a.afm, b, pix0, nv, g);
        }
        {   // ---- joff: |sigmoid - 0.5 - t| on junction pixels, times H*W / c_b (applied to the value by the final kernel)
            float l[2][4], g[2][4], t[2][4];
            load_map<2>(a.joff, b, pix0, nv, l);
            load_target(a.t_joff + (int64_t)b * 2 * HW, pix0, nv, a.tvec, t[0]);
            load_target(a.t_joff + (int64_t)b * 2 * HW + HW, pix0, nv, a.tvec, t[1]);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nv) {
                    g[0][k] = 0.f; g[1][k] = 0.f;
                    if (is_junction(tj[k])) {
                        const float s0 = sigmoidf(l[0][k]), s1 = sigmoidf(l[1][k]);
                        const float d0 = joff_residual(s0, t[0][k]), d1 = joff_residual(s1, t[1][k]);
                        acc[4] += fabsf(d0) + fabsf(d1);
                        acc[5] += 1.f;
                        if (GRAD) {
                            g[0][k] = joff_scale * (signf(d0) * (s0 * (1.f - s0)));
                            g[1][k] = joff_scale * (signf(d1) * (s1 * (1.f - s1)));
                        }
                    }
                }
            if (GRAD) store_map<2>(a.joff, b, pix0, nv, g);
        }
    }
#pragma unroll
    for (int i = 0; i < NPART; ++i) {
        const float v = wave_sum(acc[i]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < NPART)
        a.parts[((int64_t)b * gridDim.x + blockIdx.x) * NPART + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// one workgroup of four waves.  Wave w takes images w, w + 4, ...; its lane l sums partials l, l + 64, ... of the image in float64, the lanes are combined by
// a fixed butterfly, the images in ascending order, the four waves in order: one fixed summation tree.  out[6] = LOSS_KEYS order + weighted total.
__global__ __launch_bounds__(256) void train_loss_final_kernel(const float* __restrict__ parts, int B, int nblk, int HW, double w_jloc, double w_joff,
                                                               double w_mask, double w_afm, double w_remask, float* __restrict__ out) {
    __shared__ double tot[4][NPART];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double run[NPART] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = wave; b < B; b += 4) {
        double s[NPART] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = lane; k < nblk; k += 64) {
            const float* p = parts + ((int64_t)b * nblk + k) * NPART;
#pragma unroll
            for (int i = 0; i < NPART; ++i) s[i] += (double)p[i];
        }
#pragma unroll
        for (int i = 0; i < NPART; ++i) s[i] = wave_sum_d(s[i]);
        if (s[5] > 0.0) s[4] = s[4] * (double)HW / s[5];    // sigmoid_l1_loss: loss * t / w, w = share of junction pixels, w == 0 -> 1
#pragma unroll
        for (int i = 0; i < NPART; ++i) run[i] += s[i];
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NPART; ++i) tot[wave][i] = run[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[NPART];
#pragma unroll
        for (int i = 0; i < NPART; ++i) t[i] = (tot[0][i] + tot[1][i]) + (tot[2][i] + tot[3][i]);
        const double n1 = (double)B * HW, n2 = 2.0 * n1;
        const double l_jloc = t[0] / n1, l_joff = t[4] / n2, l_mask = t[1] / n1, l_afm = t[3] / n2, l_remask = t[2] / n1;
        out[0] = (float)l_jloc; out[1] = (float)l_joff; out[2] = (float)l_mask; out[3] = (float)l_afm; out[4] = (float)l_remask;
        out[5] = (float)(w_jloc * l_jloc + w_joff * l_joff + w_mask * l_mask + w_afm * l_afm + w_remask * l_remask);
    }
}

bool aligned(const void* p, int bytes) { return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0; }

// the widest access every (image, channel, pixel group) of a map - and of its gradient - can take
int map_mode(const float* p, const float* g, int64_t sb, int64_t sc, int64_t sp, int HW) {
    if (sp == 1 && HW % 4 == 0 && sb % 4 == 0 && sc % 4 == 0 && aligned(p, 16) && aligned(g, 16)) return MODE_PLANE4;
    if (sc == 1 && sp % 2 == 0 && sb % 2 == 0 && aligned(p, 8) && aligned(g, 8)) return MODE_ROW2;
    return MODE_ELEM;
}

int64_t parts_bytes(int B, int64_t HW) { return p3_up256((int64_t)B * p3_ceil_div(HW, PIX) * NPART * 4); }

}  // namespace

extern "C" int64_t p3_hisup_train_loss_workspace_bytes(int B, int H, int W) {
    const int64_t HW = (int64_t)H * W;
    return parts_bytes(B, HW) + p3_up256((int64_t)B * p3_ceil_div(HW, CNT_PIX) * 4);
}

extern "C" int p3_hisup_train_loss(const float* jloc, int64_t jloc_sb, int64_t jloc_sc, int64_t jloc_sp, const float* joff, int64_t joff_sb,
                                   int64_t joff_sc, int64_t joff_sp, const float* mask, int64_t mask_sb, int64_t mask_sc, int64_t mask_sp,
                                   const float* afm, int64_t afm_sb, int64_t afm_sc, int64_t afm_sp, const float* remask, int64_t remask_sb,
                                   int64_t remask_sc, int64_t remask_sp, const int64_t* t_jloc, const float* t_joff, const float* t_mask,
                                   const float* t_afm, int B, int H, int W, const float* weights, float* losses, float* d_jloc, float* d_joff,
                                   float* d_mask, float* d_afm, float* d_remask, void* workspace, void* stream) {
    P3_CHECK(jloc && joff && mask && afm && remask && t_jloc && t_joff && t_mask && t_afm && weights && losses && workspace, P3_EINVAL,
             "p3_hisup_train_loss: null pointer");
    const int ngrad = (d_jloc != nullptr) + (d_joff != nullptr) + (d_mask != nullptr) + (d_afm != nullptr) + (d_remask != nullptr);
    P3_CHECK(ngrad == 0 || ngrad == 5, P3_EINVAL, "p3_hisup_train_loss: the five gradient pointers are given together or not at all");
    P3_CHECK(B > 0 && B <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= MAX_HW, P3_ESHAPE, "p3_hisup_train_loss: bad sizes (H * W <= 2^22, B <= 65535)");
    hipStream_t s = (hipStream_t)stream;
    const int HW = H * W, nblk = p3_ceil_div(HW, PIX), ncb = p3_ceil_div(HW, CNT_PIX);
    const bool grad = ngrad == 5;
    const double n1 = (double)B * HW, n2 = 2.0 * n1;
    Args a;
    a.jloc = Map{jloc, d_jloc, jloc_sb, jloc_sc, jloc_sp, map_mode(jloc, d_jloc, jloc_sb, jloc_sc, jloc_sp, HW)};
    a.joff = Map{joff, d_joff, joff_sb, joff_sc, joff_sp, map_mode(joff, d_joff, joff_sb, joff_sc, joff_sp, HW)};
    a.mask = Map{mask, d_mask, mask_sb, mask_sc, mask_sp, map_mode(mask, d_mask, mask_sb, mask_sc, mask_sp, HW)};
    a.afm = Map{afm, d_afm, afm_sb, afm_sc, afm_sp, map_mode(afm, d_afm, afm_sb, afm_sc, afm_sp, HW)};
    a.remask = Map{remask, d_remask, remask_sb, remask_sc, remask_sp, map_mode(remask, d_remask, remask_sb, remask_sc, remask_sp, HW)};
    a.t_jloc = t_jloc; a.t_joff = t_joff; a.t_mask = t_mask; a.t_afm = t_afm;
    a.HW = HW;
    a.tvec = HW % 4 == 0 && aligned(t_jloc, 16) && aligned(t_joff, 16) && aligned(t_mask, 16) && aligned(t_afm, 16);
    a.k_jloc = (float)((double)weights[0] / n1);
    a.k_joff = (double)weights[1] / n2;
    a.k_mask = (float)((double)weights[2] / n1);
    a.k_afm = (float)((double)weights[3] / n2);
    a.k_remask = (float)((double)weights[4] / n1);
    a.parts = (float*)workspace;
    a.cnt = (const int32_t*)((char*)workspace + parts_bytes(B, HW));
    a.ncb = ncb;
    if (grad) {
        hipLaunchKernelGGL(junction_count_kernel, dim3(ncb, B), dim3(256), 0, s, t_jloc, HW, (int)(HW % 2 == 0 && aligned(t_jloc, 16)),
                           (int32_t*)((char*)workspace + parts_bytes(B, HW)));
        P3_LAUNCH_CHECK();
        hipLaunchKernelGGL(train_loss_kernel<true>, dim3(nblk, B), dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL(train_loss_kernel<false>, dim3(nblk, B), dim3(256), 0, s, a);
    }
    P3_LAUNCH_CHECK();
    hipLaunchKernelGGL(train_loss_final_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, B, nblk, HW, (double)weights[0], (double)weights[1],
                       (double)weights[2], (double)weights[3], (double)weights[4], losses);
    P3_LAUNCH_CHECK();
    return P3_OK;
}
