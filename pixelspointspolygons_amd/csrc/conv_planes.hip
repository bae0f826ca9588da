// p3hip: the passes around a 3 x 3 convolution that runs on the PLANES GEMM kernels (include/p3hip.h: p3_gemm_x3 conv_*, p3_gemm_tn_x3_conv)
//
//   p3_pad_nhwc_planes   fp32 token-major map [B*H*W, C] -> zero-bordered planes image [B, H+2, W+2, C] with guard rows, one pass: what p3_pad_nhwc followed by
//                        p3_to_planes would write, plus - `pre` given - the BatchNorm statistics term of a gradient (p3_affine_fix_ld's arithmetic) on the way
//   p3_col_stats         column sums and sums of squares of the convolution's fp32 output (the BatchNorm batch statistics; the planes epilogue has no column
//                        sums): workgroup partials, added in workgroup order in float64 by p3_det_reduce - no float atomics, the same bits on every run
#include "p3_common.h"
#include "gemm_x3_epi.h"

namespace {

// one thread = 8 channels of one row of the destination (guard rows, border pixels and tail rows included: every byte of the buffer is written here)
__global__ __launch_bounds__(256) void pad_nhwc_planes_kernel(const float* __restrict__ src, int ld_src, const float* __restrict__ pre, int ld_pre,
                                                              const float* __restrict__ a, const float* __restrict__ b, bf16_t* __restrict__ hi,
                                                              bf16_t* __restrict__ lo, int ld_dst, int B, int H, int W, int C, int c8n, int guard, int64_t rows_total) {
    const int Pw = W + 2, Pp = (H + 2) * Pw;
    const int64_t img_rows = (int64_t)B * Pp, total = (rows_total + 2 * (int64_t)guard) * c8n;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t rg = i / c8n;
        const int c = (int)(i - rg * c8n) * 8;
        const int64_t r = rg - guard;                    // row of the padded image; < 0 / >= img_rows: guard and tail rows
        uint4 h = make_uint4(0, 0, 0, 0), l = make_uint4(0, 0, 0, 0);
        if (r >= 0 && r < img_rows) {
            const int bi = (int)(r / Pp), rr = (int)(r - (int64_t)bi * Pp), py = rr / Pw, px = rr - py * Pw;
            if (py >= 1 && py <= H && px >= 1 && px <= W && c < C) {           // columns C .. Cp - 1 are zero padding
                const int64_t m = ((int64_t)bi * H + (py - 1)) * W + (px - 1);
                const float* s = src + m * ld_src + c;
                const float4 s0 = *reinterpret_cast<const float4*>(s), s1 = *reinterpret_cast<const float4*>(s + 4);
                float d[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
                if (pre) {
                    const float* p = pre + m * ld_pre + c;
                    const float4 p0 = *reinterpret_cast<const float4*>(p), p1 = *reinterpret_cast<const float4*>(p + 4);
                    const float hh[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
#pragma unroll
                    for (int k = 0; k < 8; ++k) d[k] += a[c + k] + b[c + k] * hh[k];          // affine_fix_kernel's expression, unchanged
                }
                x3_split8(d, h, l);
            }
        }
        *reinterpret_cast<uint4*>(hi + r * ld_dst + c) = h;
        *reinterpret_cast<uint4*>(lo + r * ld_dst + c) = l;
    }
}

// thread -> (row lane rl = tid / Q, column quad q = tid % Q), Q = N / 4; the workgroup owns rows [blk * rpb, (blk + 1) * rpb), a thread every RL-th of them.
// The RL row lanes fold through LDS in lane order; the workgroup's 2 N partials go to scratch[blk][2 N].
__global__ __launch_bounds__(256) void col_stats_kernel(const float* __restrict__ x, int ld, int64_t M, int N, int64_t rpb, float* __restrict__ parts) {
    __shared__ float red[256 * 8];
    const int Q = N / 4, RL = 256 / Q, tid = threadIdx.x;
    const int rl = tid / Q, q = tid - rl * Q;
    float s[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {0.f, 0.f, 0.f, 0.f};
    if (rl < RL) {
        const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = r0 + rpb < M ? r0 + rpb : M;
        for (int64_t r = r0 + rl; r < r1; r += RL) {
            const float4 v = *reinterpret_cast<const float4*>(x + r * ld + q * 4);
            s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
            ss[0] = fmaf(v.x, v.x, ss[0]); ss[1] = fmaf(v.y, v.y, ss[1]); ss[2] = fmaf(v.z, v.z, ss[2]); ss[3] = fmaf(v.w, v.w, ss[3]);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) { red[tid * 8 + k] = s[k]; red[tid * 8 + 4 + k] = ss[k]; }
    }
    __syncthreads();
    for (int t = tid; t < 2 * N; t += 256) {
        const int which = t / N, col = t - which * N, cq = col >> 2, k = col & 3;
        float acc = 0.f;
        for (int j = 0; j < RL; ++j) acc += red[(j * Q + cq) * 8 + which * 4 + k];
        parts[(int64_t)blockIdx.x * 2 * N + t] = acc;
    }
}

}  // namespace

extern "C" int p3_pad_nhwc_planes(const float* src, int ld_src, const float* pre, int ld_pre, const float* a, const float* b, void* hi, void* lo, int ld_dst, int B,
                                  int H, int W, int C, int Cp, int guard, int64_t rows_total, void* stream) {
    P3_CHECK(src && hi && lo && B > 0 && H > 0 && W > 0 && C > 0 && guard >= 0, P3_EINVAL, "p3_pad_nhwc_planes: bad arguments");
    P3_CHECK(rows_total >= (int64_t)B * (H + 2) * (W + 2), P3_ESHAPE, "p3_pad_nhwc_planes: rows_total smaller than the padded image");
    P3_CHECK(!pre || (a && b), P3_EINVAL, "p3_pad_nhwc_planes: pre needs a and b");
    P3_CHECK(C % 8 == 0 && Cp % 8 == 0 && Cp >= C && ld_src % 4 == 0 && ld_src >= C && ld_dst % 8 == 0 && ld_dst >= Cp && (!pre || (ld_pre % 4 == 0 && ld_pre >= C)) &&
                 ((uintptr_t)src | (uintptr_t)pre | (uintptr_t)hi | (uintptr_t)lo) % 16 == 0,
             P3_EALIGN, "p3_pad_nhwc_planes: C % 8, 16-byte rows");
    const int64_t total = (rows_total + 2 * (int64_t)guard) * (Cp / 8);
    const int grid = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
    if (p3_tracing()) p3_note_kernel(pre ? "pad_nhwc_planes_kernel<fix>" : "pad_nhwc_planes_kernel");
    hipLaunchKernelGGL(pad_nhwc_planes_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, src, ld_src, pre, ld_pre, a, b, (bf16_t*)hi, (bf16_t*)lo, ld_dst, B, H, W,
                       C, Cp / 8, guard, rows_total);
    P3_LAUNCH_CHECK();
    return P3_OK;
}

extern "C" int p3_col_stats(const float* x, int ld, int64_t M, int N, float* sums, float* scratch, int64_t scratch_floats, void* stream) {
    P3_CHECK(x && sums && scratch && M > 0 && N > 0, P3_EINVAL, "p3_col_stats: bad arguments");
    P3_CHECK(N % 4 == 0 && N <= 1024 && ld % 4 == 0 && ld >= N && ((uintptr_t)x % 16) == 0, P3_EALIGN, "p3_col_stats: N % 4 == 0, N <= 1024, 16-byte rows");
    P3_CHECK(scratch_floats >= 2 * (int64_t)N, P3_EINVAL, "p3_col_stats: scratch smaller than one workgroup's partials");
    int64_t nb = scratch_floats / (2 * (int64_t)N);
    if (nb > 1024) nb = 1024;
    const int64_t want = (M + 31) / 32;                 // at least 32 rows per workgroup
    if (nb > want) nb = want;
    const int64_t rpb = (M + nb - 1) / nb;
    nb = (M + rpb - 1) / rpb;
    hipStream_t s = (hipStream_t)stream;
    if (p3_tracing()) p3_note_kernel("col_stats_kernel");
    hipLaunchKernelGGL(col_stats_kernel, dim3((int)nb), dim3(256), 0, s, x, ld, M, N, rpb, scratch);
    P3_LAUNCH_CHECK();
    return p3_det_reduce(scratch, (int)nb, 2 * (int64_t)N, sums, 2 * N, 0, s);
}
