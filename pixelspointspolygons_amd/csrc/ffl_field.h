// p3hip - frame-field sampling of the FFL polygon optimisers (acm.hip, asm.hip): the pixel clamp, the level term, the align term of an edge with its
// gradient, and the fixed-order workgroup sum of the three loss terms.  The only place these are written down: both optimisers, fast path and fallback,
// evaluate them through the functions below, which is what keeps their results bit-compatible.
//
// Contraction: hipcc fuses a * b + c into an fma by default, and whether it does decides the low bits of every expression here.  The optimisers promise the
// same bits from both of their paths, so all of this is compiled with contraction OFF.  A file-scope pragma acts from where it stands to the end of the
// translation unit, so one in the including file alone, placed after its includes, would leave this header contracted: the header carries the pragma
// itself.  Include it only from translation units that turn contraction off themselves (ffl_loss.hip does not, and keeps its own align_err).
#pragma once
#include "p3_common.h"

#pragma clang fp contract(off)

// float coordinate -> pixel index in [0, n-1]; the clamp in float first keeps the conversion defined for any input (NaN lands on 0)
__device__ __forceinline__ int ffl_pix(float v, int n) {
    const int i = (int)fminf(fmaxf(v, -1.f), (float)n);
    return min(max(i, 0), n - 1);
}

struct FflLevel { float dv, dIdy, dIdx; };          // indicator(p) - level, and d indicator / d (row, col) at p
struct FflEdge {
    float e0, e1, norm, mask;      // e = b - a, |e|, and 0 where |e| < 0.1 (else 1)
    float ge0, ge1;                // d align / d e, NOT masked
    float align;                   // |f(z)|^2, masked
};

// level term at p = (row, col) of the indicator map `ind` [H,W]: bilinear_interpolate (torch_lydorn/torch/nn/functionnal.py:4-42), x = col, y = row;
// weights from the unclamped floor, fetches clamped.  The caller squares dv for the loss and scales 2 dv (dIdy, dIdx) by its own data coefficient.
__device__ __forceinline__ FflLevel ffl_level(const float* ind, int H, int W, float level, float2 p) {
    const float y = p.x, x = p.y;
    const float x0 = floorf(x), y0 = floorf(y), x1 = x0 + 1.f, y1 = y0 + 1.f;
    const int x0i = ffl_pix(x0, W), x1i = ffl_pix(x1, W), y0i = ffl_pix(y0, H), y1i = ffl_pix(y1, H);
    const float Ia = ind[(int64_t)y0i * W + x0i], Ib = ind[(int64_t)y1i * W + x0i], Ic = ind[(int64_t)y0i * W + x1i], Id = ind[(int64_t)y1i * W + x1i];
    const float ax = x1 - x, bx = x - x0, ay = y1 - y, by = y - y0;
    const float val = (ax * ay) * Ia + (ax * by) * Ib + (bx * ay) * Ic + (bx * by) * Id;
    FflLevel o;
    o.dv = val - level;
    o.dIdy = (ax * Ib - ax * Ia) + (bx * Id - bx * Ic);
    o.dIdx = (ay * Ic - ay * Ia) + (by * Id - by * Ib);
    return o;
}

// align term of the edge a -> b against the frame field `cf` [4,H,W] = (re c0, im c0, re c2, im c2), looked up at the edge's midpoint
// (polygonize_acm.py:98-122, polygonize_asm.py:182-201): z = e / (|e| + eps), with eps 1e-3 in the ACM and 1e-6 in the ASM.
__device__ __forceinline__ FflEdge ffl_edge(const float* cf, int H, int W, float eps, float2 a, float2 b) {
    FflEdge o;
    const float e0 = b.x - a.x, e1 = b.y - a.y;
    const int pr = ffl_pix(rintf((b.x + a.x) / 2.f), H), pc = ffl_pix(rintf((b.y + a.y) / 2.f), W);          // round half to even, like torch.round
    const int64_t hw = (int64_t)H * W;
    const float* q = cf + (int64_t)pr * W + pc;
    const float c0r = q[0], c0i = q[hw], c2r = q[2 * hw], c2i = q[3 * hw];
    const float norm = sqrtf(e0 * e0 + e1 * e1);
    const float mask = norm < 0.1f ? 0.f : 1.f;
    const float d = norm + eps;
    const float z0 = e0 / d, z1 = e1 / d;
    const float z2r = z0 * z0 - z1 * z1, z2i = z0 * z1 + z1 * z0;
    const float z4r = z2r * z2r - z2i * z2i, z4i = z2r * z2i + z2i * z2r;
    const float fr = z4r + (c2r * z2r - c2i * z2i) + c0r, fi = z4i + (c2r * z2i + c2i * z2r) + c0i;          // f(z) = z^4 + c2 z^2 + c0
    o.align = (fr * fr + fi * fi) * mask;
    // d|f|^2 / d(re z, im z) = 2 conj(f'(z)) f(z),  f'(z) = 4 z^3 + 2 c2 z
    const float z3r = z2r * z0 - z2i * z1, z3i = z2r * z1 + z2i * z0;
    const float pr_ = 4.f * z3r + 2.f * (c2r * z0 - c2i * z1), pi_ = 4.f * z3i + 2.f * (c2r * z1 + c2i * z0);
    const float gz0 = 2.f * (pr_ * fr + pi_ * fi), gz1 = 2.f * (pr_ * fi - pi_ * fr);
    // z = e / (|e| + eps):  dz_i / de_j = delta_ij / d - e_i e_j / (|e| d^2), the second term 0 at |e| = 0 (torch.norm's subgradient)
    const float dot = gz0 * e0 + gz1 * e1;
    const float k = norm > 0.f ? dot / (norm * d * d) : 0.f;
    o.ge0 = gz0 / d - k * e0;
    o.ge1 = gz1 / d - k * e1;
    o.e0 = e0; o.e1 = e1; o.norm = norm; o.mask = mask;
    return o;
}

// sums of (align, level, length) over a workgroup of THREADS threads in a fixed order: xor butterfly inside a wave, then the waves in index order.
// red: 3 * (THREADS / 64) floats of LDS
template <int THREADS>
__device__ __forceinline__ void ffl_reduce3(float a, float l, float g, float* red, float* out3) {
    static_assert(THREADS % 64 == 0, "whole waves");
    a = wave_sum(a); l = wave_sum(l); g = wave_sum(g);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[3 * w] = a; red[3 * w + 1] = l; red[3 * w + 2] = g; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        for (int i = 0; i < THREADS / 64; ++i) { s0 += red[3 * i]; s1 += red[3 * i + 1]; s2 += red[3 * i + 2]; }
        out3[0] = s0; out3[1] = s1; out3[2] = s2;
    }
}
