// p3hip kernels of the DINOv2 ViT-S/14 encoder: padded patchify (K = 588 -> a GEMM-legal leading dimension), bicubic resampling of the trained
// position table (forward gather + transposed gather backward: no atomics, bit-reproducible) and the LayerScale weight fold with its backward.
// All HBM-bound and small: 16-byte vector accesses wherever the layout allows.
#include "p3_common.h"

namespace {

// ---- padded patchify: one workgroup per patch, thread k < K = (c, py, px) gathers, K <= k < ldk writes the zero pad of the row ----
template <typename T>
__global__ void patchify_ld_kernel(const float* __restrict__ img, T* __restrict__ out, int Cin, int H, int W, int P, int ldk) {
    const int gw = W / P, gh = H / P, K = Cin * P * P;
    const int k = threadIdx.x;
    if (k >= ldk) return;
    const int row = blockIdx.x;
    float v = 0.f;
    if (k < K) {
        const int gx = row % gw, gy = (row / gw) % gh, b = row / (gw * gh);
        const int px = k % P, py = (k / P) % P, c = k / (P * P);
        v = img[(((int64_t)b * Cin + c) * H + gy * P + py) * W + gx * P + px];
    }
    out[(int64_t)row * ldk + k] = Cvt<T>::from_f(v);
}

// ---- position table resampling.  table [1 + n_in^2, D] (row 0 = CLS, passes through), out [1 + n_out^2, D];
//      wy / wx [n_out, n_in]: the separable bicubic taps (<= 4 non-zeros per row), built once on the host.
//      One workgroup per output token, one float4 of channels per thread; the taps are wave-uniform, zero taps are skipped. ----
__global__ void posembed_resample_kernel(const float* __restrict__ table, const float* __restrict__ wy, const float* __restrict__ wx,
                                         float* __restrict__ out, int n_in, int n_out, int D4) {
    const int t = blockIdx.x, c = threadIdx.x;
    if (c >= D4) return;
    const f32x4* tab = reinterpret_cast<const f32x4*>(table);
    f32x4* o = reinterpret_cast<f32x4*>(out);
    if (t == 0) { o[c] = tab[c]; return; }
    const int y = (t - 1) / n_out, x = (t - 1) % n_out;
    const float* ry = wy + (int64_t)y * n_in;
    const float* rx = wx + (int64_t)x * n_in;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < n_in; ++i) {
        const float a = ry[i];
        if (a == 0.f) continue;
        for (int j = 0; j < n_in; ++j) {
            const float b = rx[j];
            if (b == 0.f) continue;
            const float w = a * b;
            const f32x4 v = tab[(int64_t)(1 + i * n_in + j) * D4 + c];
            acc.x = fmaf(w, v.x, acc.x); acc.y = fmaf(w, v.y, acc.y); acc.z = fmaf(w, v.z, acc.z); acc.w = fmaf(w, v.w, acc.w);
        }
    }
    o[(int64_t)t * D4 + c] = acc;
}

// transposed gather: one workgroup per SOURCE cell (i, j) walks the outputs (y, x) whose taps touch it, in a fixed order
__global__ void posembed_resample_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ wy, const float* __restrict__ wx,
                                             float* __restrict__ dtable, int n_in, int n_out, int D4) {
    const int t = blockIdx.x, c = threadIdx.x;
    if (c >= D4) return;
    const f32x4* go = reinterpret_cast<const f32x4*>(dout);
    f32x4* gt = reinterpret_cast<f32x4*>(dtable);
    if (t == 0) { gt[c] = go[c]; return; }
    const int i = (t - 1) / n_in, j = (t - 1) % n_in;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int y = 0; y < n_out; ++y) {
        const float a = wy[(int64_t)y * n_in + i];
        if (a == 0.f) continue;
        for (int x = 0; x < n_out; ++x) {
            const float b = wx[(int64_t)x * n_in + j];
            if (b == 0.f) continue;
            const float w = a * b;
            const f32x4 v = go[(int64_t)(1 + y * n_out + x) * D4 + c];
            acc.x = fmaf(w, v.x, acc.x); acc.y = fmaf(w, v.y, acc.y); acc.z = fmaf(w, v.z, acc.z); acc.w = fmaf(w, v.w, acc.w);
        }
    }
    gt[(int64_t)t * D4 + c] = acc;
}

// ---- LayerScale fold: W'[n, :] = gamma[n] * W[n, :], b'[n] = gamma[n] * b[n].  One workgroup per output row. ----
__global__ void layerscale_fold_kernel(const float* __restrict__ gamma, const float* __restrict__ W, const float* __restrict__ b,
                                       float* __restrict__ Wf, float* __restrict__ bf, int K4) {
    const int n = blockIdx.x;
    const float g = gamma[n];
    const f32x4* src = reinterpret_cast<const f32x4*>(W) + (int64_t)n * K4;
    f32x4* dst = reinterpret_cast<f32x4*>(Wf) + (int64_t)n * K4;
    for (int k = threadIdx.x; k < K4; k += blockDim.x) {
        const f32x4 v = src[k];
        const f32x4 r = {g * v.x, g * v.y, g * v.z, g * v.w};
        dst[k] = r;
    }
    if (b && threadIdx.x == 0) bf[n] = g * b[n];
}

// backward: one wave per output row.  dW = gamma * dW', db = gamma * db', dgamma[n] = sum_k dW'[n, k] W[n, k] + db'[n] b[n] - from the products
// themselves (never a division by gamma: gamma may be zero); per-lane partial sums in k order, then the xor-butterfly: a fixed summation order.
__global__ void layerscale_fold_bwd_kernel(const float* __restrict__ gamma, const float* __restrict__ W, const float* __restrict__ b,
                                           const float* __restrict__ dWf, const float* __restrict__ dbf, float* __restrict__ dW,
                                           float* __restrict__ db, float* __restrict__ dgamma, int N, int K4) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (n >= N) return;                                   // whole waves leave together: no divergence inside wave_sum
    const float g = gamma[n];
    const f32x4* w = reinterpret_cast<const f32x4*>(W) + (int64_t)n * K4;
    const f32x4* gw = reinterpret_cast<const f32x4*>(dWf) + (int64_t)n * K4;
    f32x4* o = reinterpret_cast<f32x4*>(dW) + (int64_t)n * K4;
    float acc = 0.f;
    for (int k = lane; k < K4; k += 64) {
        const f32x4 a = gw[k], v = w[k];
        acc = fmaf(a.x, v.x, acc); acc = fmaf(a.y, v.y, acc); acc = fmaf(a.z, v.z, acc); acc = fmaf(a.w, v.w, acc);
        const f32x4 r = {g * a.x, g * a.y, g * a.z, g * a.w};
        o[k] = r;
    }
    acc = wave_sum(acc);
    if (lane == 0) {
        if (b) { acc = fmaf(dbf[n], b[n], acc); db[n] = g * dbf[n]; }
        dgamma[n] = acc;
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace

extern "C" int p3_patchify_ld(const float* img, void* out, int B, int Cin, int H, int W, int P, int ldk, int dtype_out, void* stream) {
    P3_CHECK(img && out && B > 0 && Cin > 0 && P > 0 && H > 0 && W > 0 && H % P == 0 && W % P == 0, P3_ESHAPE, "p3_patchify_ld: bad arguments");
    P3_CHECK(ldk >= Cin * P * P && ldk <= 1024, P3_ESHAPE, "p3_patchify_ld: need Cin*P*P <= ldk <= 1024");
    P3_CHECK((int64_t)B * (H / P) * (W / P) < (1ll << 31), P3_ESHAPE, "p3_patchify_ld: too many patches");
    hipStream_t s = (hipStream_t)stream;
    const dim3 gr((unsigned)(B * (H / P) * (W / P))), bl((unsigned)((ldk + 63) / 64 * 64));
    return p3_by_dtype(dtype_out, false, "p3_patchify_ld", [&](auto t) {
        using T = typename decltype(t)::type;
        return p3_launch<patchify_ld_kernel<T>>(p3_kname<T>("patchify_ld_kernel"), gr, bl, 0, s, img, (T*)out, Cin, H, W, P, ldk);
    });
}

static int resample_args_ok(const void* a, const void* wy, const void* wx, const void* o, int n_in, int n_out, int D) {
    return a && wy && wx && o && n_in > 0 && n_out > 0 && n_in <= 1024 && n_out <= 1024 && D > 0 && D % 4 == 0 && D <= 4096 && aligned16(a) && aligned16(o);
}

extern "C" int p3_posembed_resample(const float* table, const float* wy, const float* wx, float* out, int n_in, int n_out, int D, void* stream) {
    P3_CHECK(resample_args_ok(table, wy, wx, out, n_in, n_out, D), P3_ESHAPE, "p3_posembed_resample: bad arguments (D % 4 == 0, D <= 4096, 16-byte aligned)");
    if (p3_tracing()) p3_note_kernel("posembed_resample_kernel");
    const int D4 = D / 4;
    hipLaunchKernelGGL(posembed_resample_kernel, dim3((unsigned)(1 + n_out * n_out)), dim3((unsigned)((D4 + 63) / 64 * 64)), 0, (hipStream_t)stream,
                       table, wy, wx, out, n_in, n_out, D4);
    P3_LAUNCH_CHECK();
    return P3_OK;
}

extern "C" int p3_posembed_resample_bwd(const float* dout, const float* wy, const float* wx, float* dtable, int n_in, int n_out, int D, void* stream) {
    P3_CHECK(resample_args_ok(dout, wy, wx, dtable, n_in, n_out, D), P3_ESHAPE, "p3_posembed_resample_bwd: bad arguments (D % 4 == 0, D <= 4096, 16-byte aligned)");
    if (p3_tracing()) p3_note_kernel("posembed_resample_bwd_kernel");
    const int D4 = D / 4;
    hipLaunchKernelGGL(posembed_resample_bwd_kernel, dim3((unsigned)(1 + n_in * n_in)), dim3((unsigned)((D4 + 63) / 64 * 64)), 0, (hipStream_t)stream,
                       dout, wy, wx, dtable, n_in, n_out, D4);
    P3_LAUNCH_CHECK();
    return P3_OK;
}

extern "C" int p3_layerscale_fold(const float* gamma, const float* W, const float* b, float* Wf, float* bf, int N, int K, void* stream) {
    P3_CHECK(gamma && W && Wf && N > 0 && K > 0 && K % 4 == 0 && (!b || bf), P3_ESHAPE, "p3_layerscale_fold: bad arguments (K % 4 == 0)");
    P3_CHECK(aligned16(W) && aligned16(Wf), P3_EALIGN, "p3_layerscale_fold: W / W' must be 16-byte aligned");
    if (p3_tracing()) p3_note_kernel("layerscale_fold_kernel");
    hipLaunchKernelGGL(layerscale_fold_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, gamma, W, b, Wf, bf, K / 4);
    P3_LAUNCH_CHECK();
    return P3_OK;
}

extern "C" int p3_layerscale_fold_bwd(const float* gamma, const float* W, const float* b, const float* dWf, const float* dbf, float* dW, float* db,
                                      float* dgamma, int N, int K, void* stream) {
    P3_CHECK(gamma && W && dWf && dW && dgamma && N > 0 && K > 0 && K % 4 == 0 && (!b || (dbf && db)), P3_ESHAPE,
             "p3_layerscale_fold_bwd: bad arguments (K % 4 == 0)");
    P3_CHECK(aligned16(W) && aligned16(dWf) && aligned16(dW), P3_EALIGN, "p3_layerscale_fold_bwd: W / dW' / dW must be 16-byte aligned");
    if (p3_tracing()) p3_note_kernel("layerscale_fold_bwd_kernel");
    hipLaunchKernelGGL(layerscale_fold_bwd_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, (hipStream_t)stream, gamma, W, b, dWf, dbf, dW, db,
                       dgamma, N, K / 4);
    P3_LAUNCH_CHECK();
    return P3_OK;
}
