// p3hip — common device/host helpers (gfx950 / CDNA4 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <type_traits>

#include "../../include/p3hip.h"
#include "gfx950_asm.h"          // LDS-DMA, waits, lds_barrier(), the transposing LDS read: all shared inline asm

typedef uint16_t bf16_t;  // raw bfloat16 bits

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
// round-to-nearest-even like torch .to(bfloat16); native casts so that hipcc emits gfx950's v_cvt_pk_bf16_f32 (one VALU op per PAIR;
// the integer RNE sequence this replaces cost ~5 ops per element and sat in every epilogue and in the attention P / dS packing)
typedef float p3_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 p3_bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ bf16_t f2bf(float f) { return __builtin_bit_cast(bf16_t, (__bf16)f); }
__device__ __forceinline__ uint32_t pack_bf2(float lo, float hi) {
    const p3_f32x2 f = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, p3_bf16x2));
}

// 16-byte register views: four dwords as loaded / stored, the same bits as one bf16 MFMA operand
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
// one bf16 MFMA operand from the two halves of a transposing read (lds_read_tr16_b64: rows +0..3, then rows +4..7)
__device__ __forceinline__ bf16x8_t tr_frag(u32x2_t a, u32x2_t b) { return __builtin_bit_cast(bf16x8_t, u32x4_t{a.x, a.y, b.x, b.y}); }

// eight fp32 values -> bf16 hi plane (round to nearest even) and bf16 lo plane (the rounded remainder): the operand split of every fp32x3 kernel
__device__ __forceinline__ void split8(const float (&v)[8], u32x4_t& h, u32x4_t& l) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t hw = pack_bf2(v[2 * k], v[2 * k + 1]);
        h[k] = hw;
        l[k] = pack_bf2(v[2 * k] - __uint_as_float(hw << 16), v[2 * k + 1] - __uint_as_float(hw & 0xffff0000u));
    }
}

template <typename T> struct Cvt;
template <> struct Cvt<float> {
    static __device__ __forceinline__ float to_f(float v) { return v; }
    static __device__ __forceinline__ float from_f(float v) { return v; }
};
template <> struct Cvt<bf16_t> {
    static __device__ __forceinline__ float to_f(bf16_t v) { return bf2f(v); }
    static __device__ __forceinline__ bf16_t from_f(float v) { return f2bf(v); }
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// inclusive scan over the workgroup (whole waves), sum or maximum; total = over all threads.  red: one T per wave.  The exclusive sum is the result - v.
template <bool MAX, typename T>
__device__ __forceinline__ T wg_scan(T v, T* red, T& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o, 64);
        if (lane >= o) v = MAX ? (t > v ? t : v) : v + t;
    }
    if (lane == 63) red[w] = v;
    __syncthreads();
    T tot = red[0], base = red[0];
    for (int i = 1; i < nw; ++i) {
        const T s = red[i];
        tot = MAX ? (s > tot ? s : tot) : tot + s;
        if (i < w) base = MAX ? (s > base ? s : base) : base + s;
    }
    __syncthreads();          // red is free again
    total = tot;
    if (w == 0) return v;
    return MAX ? (base > v ? base : v) : base + v;
}
// one chunk of an exclusive sum that takes the workgroup several passes: the sum of everything in front of v (`carry`: the chunks before), then carry takes the chunk in
template <typename T>
__device__ __forceinline__ T wg_excl(T v, T* red, T& carry) {
    T total;
    const T ex = carry + wg_scan<false, T>(v, red, total) - v;
    carry += total;
    return ex;
}
// the maximum over the workgroup, in every thread
template <typename T>
__device__ __forceinline__ T wg_max(T v, T* red) {
    T total;
    wg_scan<true, T>(v, red, total);
    return total;
}
// two 32-bit counts that one 64-bit scan sums together (or a sort key and its payload), and a 64-bit total clamped into an int32 output
__device__ __forceinline__ unsigned long long p3_pack2(uint32_t hi, uint32_t lo) { return ((unsigned long long)hi << 32) | lo; }
__device__ __forceinline__ int p3_hi32(unsigned long long k) { return (int)(k >> 32); }
__device__ __forceinline__ int p3_lo32(unsigned long long k) { return (int)(k & 0xffffffffull); }
__device__ __forceinline__ int32_t p3_sat31(int64_t x) { return (int32_t)(x < 0x7fffffff ? x : 0x7fffffff); }

// ---- counter-based dropout (p3_dropout) ---------------------------------------------------------------------------------
// Element (row, col) of a site: bits = hash32(rowkey(row) ^ colkey(col >> 1)), 16 bits per element (low half: even col, high half:
// odd col); kept iff bits16 >= p * 65536.  A lane that owns one row (attention fwd / dQ, GEMM epilogue) pays one 2-multiply hash
// per TWO elements; v_mul_lo_u32 is quarter rate on CDNA, so the multiply count is what matters.
__device__ __forceinline__ uint32_t p3_hash32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
struct DropKey { uint32_t k0, k1, thresh; float inv_keep; bool on; };
__device__ __forceinline__ DropKey drop_key(const p3_dropout& dr) {
    DropKey k; k.on = dr.seed != nullptr && dr.p > 0.f; k.k0 = 0; k.k1 = 0; k.thresh = 0; k.inv_keep = 1.f;
    if (k.on) {
        const unsigned long long s = *dr.seed;
        k.k0 = p3_hash32((uint32_t)s ^ (dr.site * 0x9E3779B9u));
        k.k1 = p3_hash32((uint32_t)(s >> 32) + dr.site * 0x85EBCA6Bu + 0x1234567u);
        k.thresh = (uint32_t)(dr.p * 65536.f + 0.5f);
        if (k.thresh > 65535u) k.thresh = 65535u;
        k.inv_keep = 65536.f / (float)(65536u - k.thresh);
    }
    return k;
}
__device__ __forceinline__ uint32_t drop_rowkey(const DropKey& k, uint64_t row) {
    return (uint32_t)row * 0x9E3779B1u + (uint32_t)(row >> 32) * 0x7FEB352Du + k.k0;
}
__device__ __forceinline__ uint32_t drop_colkey(const DropKey& k, uint32_t col) { return (col >> 1) * 0x85EBCA77u + k.k1; }
__device__ __forceinline__ uint32_t drop_bits(uint32_t rowkey, uint32_t colkey) { return p3_hash32(rowkey ^ colkey); }
__device__ __forceinline__ bool drop_keep_lo(const DropKey& k, uint32_t bits) { return (bits & 0xffffu) >= k.thresh; }
__device__ __forceinline__ bool drop_keep_hi(const DropKey& k, uint32_t bits) { return (bits >> 16) >= k.thresh; }
__device__ __forceinline__ bool drop_keep(const DropKey& k, uint64_t row, uint32_t col) {
    const uint32_t bits = drop_bits(drop_rowkey(k, row), drop_colkey(k, col));
    return (col & 1u) ? drop_keep_hi(k, bits) : drop_keep_lo(k, bits);
}

// XCD-aware bijective block remap: hardware hands consecutive workgroup ids round-robin to the 8 XCDs (each with its own 4 MiB L2);
// this gives XCD x the CONSECUTIVE logical ids [x*n/8, (x+1)*n/8), so blocks that share operands (same attention head, same
// M-split of a weight gradient, same A row panel) run on one XCD and hit its L2 instead of fetching the operand 8 times.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg / 8, r = nwg % 8, xcd = bid % 8, idx = bid / 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// Attention launches: logical block id -> (128-row block, (batch, head) pair).  L = 785 = 6 x 128 + 17 (ViT) and 385 = 3 x 128 + 1 (decoder)
// leave a nearly empty last block per pair that still walks the whole key / query sequence: one wave live, a slot held for most of a full
// block's time, and a grid of 7/6 (4/3) x the full blocks - ViT forward: 2304 full blocks = exactly 3 rounds of the 768 resident slots, the
// 384 tail blocks mixed in made it 3.5.  mode 1: inside each XCD's consecutive id range (xcd_remap) the TAIL blocks come first - short, they
// finish while the first round of full blocks starts, and the launch ends on whole rounds of full blocks; the blocks of one pair stay on one
// XCD (K / V in one L2).  Needs pairs % 8 == 0 and a ragged last block; anything else keeps the pair-major order (mode 0).
__device__ __forceinline__ void attn_block_of(int lid, int nblk, int L, int pairs, int mode, int& blk, int& pair) {
    if (mode == 1 && nblk > 1 && (L & 127) != 0 && (pairs & 7) == 0) {
        const int p8 = pairs >> 3, per_xcd = p8 * nblk;
        const int x = lid / per_xcd, local = lid - x * per_xcd;
        if (local < p8) { pair = x * p8 + local; blk = nblk - 1; }
        else { const int l2 = local - p8; pair = x * p8 + l2 / (nblk - 1); blk = l2 % (nblk - 1); }
    } else { blk = lid % nblk; pair = lid / nblk; }
}
int p3_attn_order(void);      // host: always 1, tail blocks first (attention.hip)

// row index of accumulator register r of a 32x32 MFMA C/D fragment (col = lane & 31)
__device__ __forceinline__ int crow32(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// exact (erf) GELU and its derivative from ONE exponential: erf by Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7, below fp32 parity
// tolerances by four orders), exp(-z^2) with z = x/sqrt(2) is also the Gaussian pdf of GELU'.  ~20 VALU ops for both values; the
// libm erff + expf pair this replaces made the fc1 epilogue cost as much as its whole K = 384 main loop (r01: 146 vs 97 us).
__device__ __forceinline__ void gelu_and_grad(float x, float& h, float& g) {
    const float z = x * 0.70710678118654752440f;
    const float az = fabsf(z);
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, az, 1.0f));
    const float e = __expf(-z * z);
    const float poly = t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.061405429f, -1.453152027f), 1.421413741f), -0.284496736f), 0.254829592f);
    const float erf_abs = fmaf(-poly, e, 1.0f);
    const float cdf = 0.5f * (1.0f + copysignf(erf_abs, z));
    h = x * cdf;
    g = fmaf(x * 0.39894228040143267794f, e, cdf);
}
__device__ __forceinline__ float gelu_erf(float x) { float h, g; gelu_and_grad(x, h, g); return h; }

// a workgroup's partial of value idx (n values per workgroup): into `slab` [gridDim.x][n] - deterministic mode, summed in workgroup order in float64 by
// p3_det_reduce right behind the launch - or, without a slab, an fp32 atomic onto out[idx].  EVERY workgroup of the grid must commit every idx (zeros included).
__device__ __forceinline__ void p3_commit(float* out, float* slab, int n, int idx, float v) {
    if (slab) slab[(int64_t)blockIdx.x * n + idx] = v;
    else atomicAdd(out + idx, v);
}

static inline int p3_ceil_div(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
static inline int64_t p3_up256(int64_t v) { return (v + 255) & ~(int64_t)255; }          // workspace sections start on 256-byte boundaries
// A workspace cut into sections, in the order they are taken: take<T>(n) is the next section, n elements of T.  base == NULL measures - every section is NULL and
// `at` ends at the bytes the workspace needs - so one function over a P3Carve states each section's type and size once, for the size query and for the entry point.
struct P3Carve {
    char* base;
    int64_t at;
    void* take_bytes(int64_t bytes) {
        char* p = base ? base + at : nullptr;
        at += p3_up256(bytes);
        return p;
    }
    template <class T> T* take(int64_t n) { return (T*)take_bytes(n * (int64_t)sizeof(T)); }
};

void p3_set_error(const char* msg);
int p3_tracing(void);                     // p3_trace_kernels(1): launch sites record the kernel they picked (p3_last_kernel)
void p3_note_kernel(const char* name);
// deterministic reductions (det_reduce.hip): scratch for workgroup partials (NULL: atomics path) and the fixed-order float64 reduce
float* p3_det_scratch(int64_t floats, int dtype);
int p3_det_reduce(const float* parts, int nparts, int64_t stride, float* out, int nvals, int accumulate, hipStream_t s);
float* p3_reduce_scratch(int64_t floats);     // the registered scratch for any dtype (per-tile partials), NULL if none / too small
float* p3_reduce_park(int64_t floats, int nparts, int nvals, int split, float* out, float* out2);
float* p3_colsum_parts(int splits, int N, float* colsum, int dtype, int* parked);   // bias-gradient partial column sums: a parked slot (*parked = 1) or the deterministic scratch
   // deferred parameter-gradient reduce (det_reduce.hip): slot or NULL
int p3_det_reduce2(const float* parts, int nparts, int64_t stride, float* tmp, float* out, float* out2, int split, int nvals, int accumulate, hipStream_t s);
#define P3_CHECK(cond, code, msg) \
    do {                          \
        if (!(cond)) {            \
            p3_set_error(msg);    \
            return (code);        \
        }                         \
    } while (0)
#define P3_LAUNCH_CHECK()                              \
    do {                                               \
        hipError_t e_ = hipGetLastError();             \
        if (e_ != hipSuccess) {                        \
            p3_set_error(hipGetErrorString(e_));       \
            return (int)e_;                            \
        }                                              \
    } while (0)
// the status of a HIP runtime call (a memset, a copy) as an entry point returns it: P3_OK, or the hipError_t with its message in p3_set_error
static inline int p3_hip_status(hipError_t e) {
    if (e != hipSuccess) p3_set_error(hipGetErrorString(e));
    return (int)e;
}
// the array can be read by the host (no device allocation, or no device at all): the polygon stages refuse such index arrays, which their kernels would follow
static inline bool p3_host_array(const void* p) {
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) { (void)hipGetLastError(); return true; }
    return a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged && a.type != hipMemoryTypeArray;
}
static inline int p3_memset(void* p, int byte, int64_t bytes, hipStream_t s) { return p3_hip_status(hipMemsetAsync(p, byte, (size_t)bytes, s)); }
// a step that returns such a status - p3_launch, p3_memset: the first one that fails ends the entry point with its code
#define P3_TRY(status)                     \
    do {                                   \
        const int rc_ = (status);          \
        if (rc_ != P3_OK) return rc_;      \
    } while (0)

// ---- dtype code -> template argument ---------------------------------------------------------------------------------------------------------------
// p3_by_dtype(dtype, x3_is_f32, "p3_entry", [&](auto t) { using T = typename decltype(t)::type; ... return status; }): calls f(p3_type<bf16_t>{}) or
// f(p3_type<float>{}) by the STORAGE type of the code and returns f's int.  P3_F32X3 is fp32 storage and is taken only where `x3_is_f32` says the entry
// accepts it.  Any other code: "<who>: dtype", P3_EUNSUP, f is not called - so nothing launches.  Two dtypes nest two calls.
template <typename T> struct p3_type { using type = T; };
template <typename F>
static inline int p3_by_dtype(int dtype, bool x3_is_f32, const char* who, F&& f) {
    if (dtype == P3_BF16) return f(p3_type<bf16_t>{});
    if (dtype == P3_F32 || (dtype == P3_F32X3 && x3_is_f32)) return f(p3_type<float>{});
    char msg[96];
    snprintf(msg, sizeof(msg), "%s: dtype", who);
    p3_set_error(msg);
    return P3_EUNSUP;
}
template <typename T> constexpr const char* p3_dtype_name() { return sizeof(T) == sizeof(bf16_t) ? "bf16" : "float"; }
// the name a typed launch records while tracing, "kernel<bf16>" or "kernel<float, bf16>"; NULL (p3_launch records nothing) when nobody traces
template <typename T, typename T2 = void>
static inline const char* p3_kname(const char* kernel) {
    if (!p3_tracing()) return nullptr;
    static thread_local char s[96];
    if constexpr (!__is_same(T2, void)) snprintf(s, sizeof(s), "%s<%s, %s>", kernel, p3_dtype_name<T>(), p3_dtype_name<T2>());
    else snprintf(s, sizeof(s), "%s<%s>", kernel, p3_dtype_name<T>());
    return s;
}

// ---- one launch path for the kernels with more than the default dynamic LDS---------------------------------------------------------------------
// p3_launch<kernel>(name, grid, block, lds, stream, args...): raises the kernel's dynamic-LDS limit when the launch asks for more than the 64 KB every kernel
// may have and more than this helper already set for THIS kernel on the CURRENT device, records `name` while tracing (NULL: a site that records none),
// launches, and returns P3_OK or the hipError_t (message in p3_set_error).  Each kernel - every template instantiation - has its own table through the
// template argument.  The table is a plain int array: two threads that race on an entry at worst both set the attribute, which is harmless; a device index
// past the table sets it on every launch.
constexpr int P3_LAUNCH_DEVICES = 16;
template <auto Kernel, typename... Args>
static inline int p3_launch(const char* name, dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
    hipError_t e = hipSuccess;
    if (lds > 64 * 1024) {
        static int raised[P3_LAUNCH_DEVICES];          // largest limit set, per device
        int dev = -1;
        e = hipGetDevice(&dev);
        const bool known = e == hipSuccess && dev >= 0 && dev < P3_LAUNCH_DEVICES;
        if (e == hipSuccess && !(known && raised[dev] >= (int)lds)) {
            e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e == hipSuccess && known) raised[dev] = (int)lds;
        }
    }
    if (e == hipSuccess) {
        if (name && p3_tracing()) p3_note_kernel(name);
        hipLaunchKernelGGL(Kernel, grid, block, lds, s, args...);
        e = hipGetLastError();
    }
    if (e != hipSuccess) { p3_set_error(hipGetErrorString(e)); return (int)e; }
    return P3_OK;
}

// ---- internal functions that cross source files (everything here has C++ linkage and is not exported) ------------------------------------------
// The dedicated-kernel hooks of p3_gemm (gemm.hip) and p3_gemm_tn_ex (gemm_tn.hip): P3_SKIP when the problem is not one of the hook's shapes - the dispatcher
// goes on with the next hook, then its tile kernel - else the launch status (P3_OK, a P3_E* code or a hipError_t).
#define P3_SKIP 0x7fffffff
static_assert(P3_SKIP > 0xffff && P3_EUNSUP < 0, "P3_SKIP lies outside the P3_E* codes (negative) and the hipError_t values (small positive)");
int p3_rows_gemm_try(const void* A, const void* W, void* C, const p3_gemm_desc* d, hipStream_t s);        // rows_gemm.hip
int p3_pair_fwd_try(const void* U, const void* W, void* C, const p3_gemm_desc* d, hipStream_t s);         // pair_fwd_mma.hip
int p3_pair_fwd_x3_try(const void* U, const void* W, void* C, const p3_gemm_desc* d, hipStream_t s);      // pair_fwd_x3.hip: the P3_F32X3 form
int p3_rows_x3_try(const void* A, const void* W, void* C, const p3_gemm_desc* d, hipStream_t s);          // rows_x3.hip: conv3 forward, P3_F32X3
int p3_gemm_tn_dma_try(const void* A, const void* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, float* colsum, float* slabs, int max_slabs,
                       hipStream_t s);                                                                     // gemm_tn_dma.hip
int p3_pair_dw_try(const void* A, const void* U, float* C, int M, int N, int K, int lda, int ldb, int ldc, const float* scale, const float* shift,
                   const void* pair_V, int pair_n, float* slabs, int max_slabs, hipStream_t s);            // pair_dw_mma.hip
int p3_pair_dw_x3_try(const void* A, const void* U, float* C, int M, int N, int K, int lda, int ldb, int ldc, const float* scale, const float* shift,
                      const void* pair_V, int pair_n, float* slabs, int max_slabs, hipStream_t s);         // pair_dw_x3.hip: the P3_F32X3 form
int p3_mask2_dw_try(const void* A, const void* B, float* C, int M, int N, int Kb, int lda, int ldb, int ldc, const float* scale, const float* shift,
                    float* slabs, int max_slabs, hipStream_t s);                                           // mask2_dw_mma.hip
int p3_mask2_dw_x3_try(const void* A, const void* B, float* C, int M, int N, int Kb, int lda, int ldb, int ldc, const float* scale, const float* shift,
                       float* slabs, int max_slabs, hipStream_t s);                                        // mask2_dw_x3.hip: the P3_F32X3 form
void p3_tn_reduce_launch(const float* slabs, float* C, int N, int K, int ldc, int splits, hipStream_t s);  // gemm_tn.hip: float64 sum of the split-M partial tiles
float* p3_tn_park(float* C, int N, int K, int ldc, int splits);                                            // gemm_tn.hip: deferred reduce slot or NULL
// where one split-M weight-gradient launch puts its partials (gemm_tn.hip).  p3_tn_parts before the launch: slabs - the caller's `slabs` when there is more than
// one split, or a parked slot in its place (the reduce waits for p3_tn_flush); cs_slab - the bias column sums' partials, parked or deterministic scratch; NULL =
// atomics.  p3_tn_parts_reduce behind the launch: its status, then the reduces of what is not parked.
struct TnParts { float* slabs; float* cs_slab; bool parked; int cs_parked; };
TnParts p3_tn_parts(float* C, int N, int K, int ldc, int splits, float* slabs, float* colsum, int cs_dtype);
int p3_tn_parts_reduce(const TnParts& p, float* C, int N, int K, int ldc, int splits, float* colsum, hipStream_t s);
void p3_pair_dv_reduce_launch(const float* slab, float* dV, int nblk, int B, int N, int C, hipStream_t s); // scorenet_bwd.hip
int p3_gemm_dma_eligible(const p3_gemm_desc* d, const void* A, const void* W, const void* C);              // gemm_dma.hip
int p3_gemm_dma_launch(const void* A, const void* W, void* C, const p3_gemm_desc* d, int variant, hipStream_t s);
bool p3_gemm_x3_as_ok(const p3_gemm_x3_desc* d);                                                           // gemm_x3_as.hip
bool p3_gemm_x3_as_default(const p3_gemm_x3_desc* d);
int p3_gemm_x3_as(const p3_gemm_x3_desc* d, hipStream_t s);
