// p3hip - FFL active-contour (ACM) polygon optimiser (predict/ffl/polygonize_acm.py:77-220: PolygonAlignLoss + TensorPolyOptimizer).
//   p3_acm_optimize   `steps` SGD iterations on every contour vertex with the analytic gradient of the reference's loss, no autograd graph.
//
// Every contour is independent of every other, and a vertex's gradient needs its two neighbours only, so
//   fast path  acm_lds_kernel: ONE launch for all steps, one workgroup per polygon.  The polygon's positions ping-pong between two LDS buffers with one
//              barrier per step; the field values (indicator: 4 bilinear taps, c0c2: 4 values per edge) are gathered from global memory - one image's maps
//              are ~1 MB at 224 x 224 and stay in L2.  A vertex evaluates BOTH of its edges (each edge is computed twice, by its two ends): that is what
//              saves the second barrier an edge pass would need.
//   fallback   acm_global_kernel: polygons over ACM_LDS_CAP vertices (or all, when forced) ping-pong between `pos` and a workspace copy, one launch per step.
// Both call acm_vertex(), compiled with floating-point contraction off: the two paths give the same bits, and so do two runs, any split of the steps into
// calls (first_iter) and any order of the polygons.  No atomics, no host synchronisation.  The sampling of the two maps (pixel clamp, level term, align term
// of an edge) and the fixed-order sum of the loss terms are shared with asm.hip: ffl_field.h, which turns contraction off for itself.
#include "p3_common.h"
#include "ffl_field.h"

#pragma clang fp contract(off)

#ifndef ACM_THREADS
#define ACM_THREADS 256           // a multiple of 64; -DACM_THREADS=64 / 128 builds the variants DESIGN.md section 11 compares (tools/build_variant.sh)
#endif
#define ACM_EPS 1e-3f             // z = e / (|e| + 1e-3) (polygonize_acm.py:117)
#define ACM_LDS_CAP 4096          // vertices: 2 buffers x 8 B x 4096 = 64 KiB, the most a workgroup gets without opting in to more dynamic LDS (16 vertices per thread)
static_assert(ACM_THREADS % 64 == 0 && ACM_LDS_CAP <= 64 * ACM_THREADS, "whole waves, and a thread's endpoint flags fit one word");
#if ACM_LDS_CAP <= 32 * ACM_THREADS
typedef uint32_t acm_flags_t;          // one bit per vertex a thread owns
#else
typedef uint64_t acm_flags_t;
#endif

struct AcmFields {
    const float* indicator;       // [B,H,W]
    const float* c0c2;            // [B,4,H,W]
    int B, H, W;
    float wd, wl, wc;             // coefficient / (sum of coefficients): the weight the reference's backward gives each term
    float level;
};
struct AcmSched { double poly_lr, warmup_factor; int warmup_iters; };
struct AcmVertex { float r, c, align, level, length; };          // new position; loss terms of the vertex and of its outgoing edge, before the update

__host__ __device__ __forceinline__ float acm_lr(const AcmSched& s, int it) {          // LambdaLR of polygonize_acm.py:183-190 in double, as Python evaluates it
    double coef = 1.0;
    if (it < s.warmup_iters) coef = 1.0 + (s.warmup_factor - 1.0) * (double)(s.warmup_iters - it) / (double)s.warmup_iters;
    return (float)(s.poly_lr * coef);
}

// One SGD step of one vertex from the positions of its predecessor, itself and its successor (cyclic inside the polygon).  The only place the ACM's loss is
// put together, from the level and align terms of ffl_field.h: both kernels call it.
__device__ __forceinline__ AcmVertex acm_vertex(const AcmFields& f, int img, float2 prev, float2 cur, float2 next, bool endpoint, float lr) {
    AcmVertex o;
    const int64_t hw = (int64_t)f.H * f.W;
    const float* ind = f.indicator + (int64_t)img * hw;
    const float* cf = f.c0c2 + (int64_t)img * 4 * hw;
    const FflLevel lv = ffl_level(ind, f.H, f.W, f.level, cur);
    o.level = lv.dv * lv.dv;
    const float gI = f.wd * (2.f * lv.dv);
    // per edge: gradient of (wc * align + wl * length) with respect to e = head - tail, length = (|e| mask)^2
    const FflEdge in = ffl_edge(cf, f.H, f.W, ACM_EPS, prev, cur), out = ffl_edge(cf, f.H, f.W, ACM_EPS, cur, next);
    const float gin_r = in.mask * (f.wc * in.ge0 + f.wl * (2.f * in.e0)), gin_c = in.mask * (f.wc * in.ge1 + f.wl * (2.f * in.e1));
    const float gout_r = out.mask * (f.wc * out.ge0 + f.wl * (2.f * out.e0)), gout_c = out.mask * (f.wc * out.ge1 + f.wl * (2.f * out.e1));
    const float nm = out.norm * out.mask;
    o.align = out.align;
    o.length = nm * nm;
    // d/dp_v: the vertex's level term, + the incoming edge's gradient (p_v is its head), - the outgoing edge's (p_v is its tail): always in this order
    const float g_r = (gI * lv.dIdy + gin_r) - gout_r;
    const float g_c = (gI * lv.dIdx + gin_c) - gout_c;
    o.r = endpoint ? cur.x : fmaf(-lr, g_r, cur.x);
    o.c = endpoint ? cur.y : fmaf(-lr, g_c, cur.y);
    return o;
}

// polygon p's clamped vertex range and image: nothing a bad slice or batch entry holds can index outside pos or the maps
__device__ __forceinline__ void acm_poly(const int32_t* poly_slice, const int32_t* poly_batch, int p, int64_t N, int B, int& start, int& n, int& img) {
    const int64_t s = min(max((int64_t)poly_slice[2 * p], (int64_t)0), N), e = min(max((int64_t)poly_slice[2 * p + 1], s), N);
    start = (int)s;
    n = (int)(e - s);
    img = min(max(poly_batch[p], 0), B - 1);
}

// fast path.  Dynamic LDS: 2 * lds_len float2 (>= 64 B).  Polygons longer than lds_len are left to the fallback.
__global__ __launch_bounds__(ACM_THREADS) void acm_lds_kernel(float2* pos, int64_t N, const int32_t* poly_slice, const int32_t* poly_batch,
                                                              const uint8_t* is_endpoint, AcmFields f, AcmSched sched, int first_iter, int steps, int lds_len,
                                                              float* poly_losses) {
    extern __shared__ float2 acm_sm[];
    const int p = blockIdx.x, tid = threadIdx.x;
    int start, n, img;
    acm_poly(poly_slice, poly_batch, p, N, f.B, start, n, img);
    if (n > lds_len) return;                                   // uniform over the workgroup
    float2* buf[2] = {acm_sm, acm_sm + n};
    for (int v = tid; v < n; v += ACM_THREADS) buf[0][v] = pos[start + v];
    __syncthreads();
    acm_flags_t ep_bits = 0;                                   // this thread's vertices (at most ACM_LDS_CAP / ACM_THREADS = 16): endpoint flags, read once
    for (int v = tid, j = 0; v < n; v += ACM_THREADS, ++j) ep_bits |= (acm_flags_t)(is_endpoint[start + v] != 0 ? 1 : 0) << j;
    float s_al = 0.f, s_lv = 0.f, s_ln = 0.f;
    for (int k = 0; k < steps; ++k) {
        const float2* src = buf[k & 1];
        float2* dst = buf[(k + 1) & 1];
        const float lr = acm_lr(sched, first_iter + k);
        const bool last = poly_losses != nullptr && k == steps - 1;
        for (int v = tid, j = 0; v < n; v += ACM_THREADS, ++j) {
            const AcmVertex o = acm_vertex(f, img, src[v == 0 ? n - 1 : v - 1], src[v], src[v == n - 1 ? 0 : v + 1], ((ep_bits >> j) & 1) != 0, lr);
            dst[v] = make_float2(o.r, o.c);
            if (last) { s_al += o.align; s_lv += o.level; s_ln += o.length; }
        }
        __syncthreads();          // the only barrier of the step: step k + 1 overwrites the buffer step k read, and every read of it lies before this
    }
    const float2* fin = buf[steps & 1];
    for (int v = tid; v < n; v += ACM_THREADS) pos[start + v] = fin[v];
    if (poly_losses) {
        __syncthreads();          // the position buffers are free now: their head holds the wave partials
        ffl_reduce3<ACM_THREADS>(s_al, s_lv, s_ln, (float*)acm_sm, poly_losses + 3 * (int64_t)p);
    }
}

// fallback, one launch per step: blockIdx.x = polygon, blockIdx.y = chunk of ACM_THREADS vertices; src -> dst are `pos` and its workspace copy in turn
// The grid is P x ceil(longest / ACM_THREADS) workgroups per step, and all but those of the long polygons return at once: with one 5000-vertex polygon among 200
// that is ~4000 empty workgroups per launch, a few microseconds beside the launch itself.  Compacting the long polygons into a list would need a pass that
// reads poly_slice on the device first; not done for a path that contours of a 224 x 224 tile never reach.
__global__ __launch_bounds__(ACM_THREADS) void acm_global_kernel(const float2* src, float2* dst, int64_t N, const int32_t* poly_slice, const int32_t* poly_batch,
                                                                 const uint8_t* is_endpoint, AcmFields f, float lr, int lds_len, int force, float* vertex_losses) {
    int start, n, img;
    acm_poly(poly_slice, poly_batch, blockIdx.x, N, f.B, start, n, img);
    if (!force && n <= lds_len) return;
    const int v = blockIdx.y * ACM_THREADS + threadIdx.x;
    if (v >= n) return;
    const float2* s = src + start;
    const AcmVertex o = acm_vertex(f, img, s[v == 0 ? n - 1 : v - 1], s[v], s[v == n - 1 ? 0 : v + 1], is_endpoint[start + v] != 0, lr);
    dst[start + v] = make_float2(o.r, o.c);
    if (vertex_losses) {
        float* w = vertex_losses + 3 * (int64_t)(start + v);
        w[0] = o.align; w[1] = o.level; w[2] = o.length;
    }
}

// fallback epilogue, one workgroup per polygon: copy the result home after an odd number of steps, and reduce the per-vertex loss terms in the fast path's order
__global__ __launch_bounds__(ACM_THREADS) void acm_global_finish_kernel(const float2* ws, float2* pos, int64_t N, const int32_t* poly_slice,
                                                                        const int32_t* poly_batch, int B, int lds_len, int force, int copy_home,
                                                                        const float* vertex_losses, float* poly_losses) {
    __shared__ float red[3 * (ACM_THREADS / 64)];
    int start, n, img;
    acm_poly(poly_slice, poly_batch, blockIdx.x, N, B, start, n, img);
    if (!force && n <= lds_len) return;
    float s_al = 0.f, s_lv = 0.f, s_ln = 0.f;
    for (int v = threadIdx.x; v < n; v += ACM_THREADS) {
        if (copy_home) pos[start + v] = ws[start + v];
        if (poly_losses) {
            const float* w = vertex_losses + 3 * (int64_t)(start + v);
            s_al += w[0]; s_lv += w[1]; s_ln += w[2];
        }
    }
    if (poly_losses) ffl_reduce3<ACM_THREADS>(s_al, s_lv, s_ln, red, poly_losses + 3 * (int64_t)blockIdx.x);
}

extern "C" int64_t p3_acm_workspace_bytes(int64_t N) { return N > 0 ? N * (int64_t)(sizeof(float2) + 3 * sizeof(float)) : 0; }

extern "C" int p3_acm_optimize(float* pos, int64_t N, const int32_t* poly_slice, const int32_t* poly_batch, int P, const uint8_t* is_endpoint,
                               const float* indicator, const float* c0c2, int B, int H, int W, float data_coef, float length_coef, float crossfield_coef,
                               float data_level, double poly_lr, int warmup_iters, double warmup_factor, int first_iter, int steps, int max_len,
                               int force_fallback, float* poly_losses, void* workspace, void* stream) {
    P3_CHECK(P >= 0 && N >= 0 && N < ((int64_t)1 << 31) && steps >= 0 && first_iter >= 0, P3_ESHAPE, "p3_acm_optimize: bad sizes (0 <= N < 2^31, P, steps, first_iter >= 0)");
    if (P == 0 || steps == 0 || N == 0) return P3_OK;
    P3_CHECK(pos && poly_slice && poly_batch && is_endpoint && indicator && c0c2, P3_EINVAL, "p3_acm_optimize: null pointer");
    P3_CHECK(B > 0 && H > 0 && W > 0, P3_ESHAPE, "p3_acm_optimize: bad map sizes");
    const float csum = (float)((double)data_coef + (double)length_coef + (double)crossfield_coef);
    P3_CHECK(csum != 0.f, P3_EINVAL, "p3_acm_optimize: the three coefficients sum to 0");
    const int64_t longest = max_len > 0 ? (int64_t)max_len : N;                  // no bound from the caller: any polygon may hold all N vertices
    const bool fast = !force_fallback;
    const bool slow = force_fallback || longest > ACM_LDS_CAP;
    P3_CHECK(!slow || workspace, P3_EINVAL, "p3_acm_optimize: null workspace (polygons over the LDS cap, or the forced fallback, need p3_acm_workspace_bytes(N))");
    const int64_t chunks = (longest + ACM_THREADS - 1) / ACM_THREADS;
    P3_CHECK(!slow || chunks <= 65535, P3_ESHAPE, "p3_acm_optimize: a polygon of more than 65535 * 256 vertices");
    hipStream_t s = (hipStream_t)stream;
    AcmFields f;
    f.indicator = indicator; f.c0c2 = c0c2; f.B = B; f.H = H; f.W = W; f.level = data_level;
    const float inv = 1.0f / csum;                              // the reference divides the weighted sum by the coefficient sum: its backward scales by 1 / sum first
    f.wd = inv * data_coef; f.wl = inv * length_coef; f.wc = inv * crossfield_coef;
    AcmSched sc;
    sc.poly_lr = poly_lr; sc.warmup_factor = warmup_factor; sc.warmup_iters = warmup_iters;
    const int lds_len = fast ? (int)(longest < ACM_LDS_CAP ? longest : ACM_LDS_CAP) : 0;
    if (fast) {
        size_t lds = (size_t)lds_len * 2 * sizeof(float2);
        if (lds < 64) lds = 64;
        P3_TRY(p3_launch<acm_lds_kernel>("acm_lds_kernel", P, ACM_THREADS, lds, s, (float2*)pos, N, poly_slice, poly_batch, is_endpoint, f, sc, first_iter, steps, lds_len,
                                         poly_losses));
    }
    if (slow) {
        float2* ws = (float2*)workspace;
        float* vloss = poly_losses ? (float*)(ws + N) : nullptr;
        for (int k = 0; k < steps; ++k) {
            const float2* src = (k & 1) ? ws : (const float2*)pos;
            float2* dst = (k & 1) ? (float2*)pos : ws;
            const float lr = acm_lr(sc, first_iter + k);
            P3_TRY(p3_launch<acm_global_kernel>("acm_global_kernel", dim3(P, (unsigned)chunks), ACM_THREADS, 0, s, src, dst, N, poly_slice, poly_batch, is_endpoint, f, lr,
                                                lds_len, force_fallback, k == steps - 1 ? vloss : nullptr));
        }
        if ((steps & 1) || poly_losses)
            P3_TRY(p3_launch<acm_global_finish_kernel>(nullptr, P, ACM_THREADS, 0, s, ws, (float2*)pos, N, poly_slice, poly_batch, B, lds_len, force_fallback, steps & 1,
                                                       vloss, poly_losses));
    }
    return P3_OK;
}
