// p3hip HiSup inference after the heads (models/hisup/model_hisup.py:229-293 `EncoderDecoder.forward_val`, models/hisup/polygon.py:8-38):
//   p3_hisup_junctions  softmax + 3x3 non-maximum suppression + threshold + top-300 per junction class + sub-pixel offsets, whole batch
//   p3_hisup_regions    softmax + threshold + 8-connected component labels + per-region area / bounding box / mean probability
//   p3_hisup_val_loss   the five validation losses of :241-245 in one pass over the pixels
// Logit maps are addressed as base[b*sb + c*sc + pix*sp] so that NCHW fp32 tensors (sb = C*HW, sc = HW, sp = 1) and the token-major fp32
// rows the predictors write (sb = HW*ld, sc = 1, sp = ld) are read in place.
// Reproducibility: every selection runs on integers (64-bit keys, integer vector atomics whose result does not depend on their order, a
// final sort on unique keys); the one float sum (a region's mean probability) is accumulated as 32.32 fixed point with integer atomics.
#include "p3_common.h"
#include "hisup_loss_pixel.h"

namespace {

constexpr int JT = 16;                 // junction tile edge (one 256-lane workgroup per tile, halo of one pixel)
constexpr int TOPK = 300;              // polygon.py:29,33
constexpr int SORT_N = 512;            // bitonic sort width for the <= 300 survivors
constexpr float JTH = 0.008f;          // polygon.py:29,33

struct Strided {
    const float* p;
    int64_t sb, sc, sp;
    __device__ __forceinline__ float at(int b, int c, int pix) const { return p[b * sb + c * sc + pix * sp]; }
};

// key of a candidate: probability bits (positive floats order like their bit patterns) above the complemented flat index, so that the
// LARGEST key is the highest probability and, among equal probabilities, the lowest index.  Keys of one (image, class) are unique.
__device__ __forceinline__ unsigned long long make_key(float p, int idx) {
    return ((unsigned long long)__float_as_uint(p) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)idx);
}

// ---- junction candidates: grid (tiles_x * tiles_y, B), 256 lanes.  cand [B, 2, HW] keys (slot 0 = class 2, slot 1 = class 1), ncand [B, 2].
__global__ __launch_bounds__(256) void junc_candidates_kernel(Strided jloc, int H, int W, int tiles_x, unsigned long long* __restrict__ cand,
                                                              int32_t* __restrict__ ncand) {
    __shared__ float sp1[(JT + 2) * (JT + 2)], sp2[(JT + 2) * (JT + 2)];
    const int b = blockIdx.y, HW = H * W;
    const int ty0 = (blockIdx.x / tiles_x) * JT, tx0 = (blockIdx.x % tiles_x) * JT;
    for (int i = threadIdx.x; i < (JT + 2) * (JT + 2); i += 256) {
        const int y = ty0 + i / (JT + 2) - 1, x = tx0 + i % (JT + 2) - 1;
        float p1 = -1.f, p2 = -1.f;                     // outside the map: below every probability (max_pool2d pads with -inf)
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const int pix = y * W + x;
            const float l0 = jloc.at(b, 0, pix), l1 = jloc.at(b, 1, pix), l2 = jloc.at(b, 2, pix);
            const float m = fmaxf(l0, fmaxf(l1, l2));
            const float e0 = expf(l0 - m), e1 = expf(l1 - m), e2 = expf(l2 - m);
            const float s = e0 + e1 + e2;
            p1 = e1 / s; p2 = e2 / s;
        }
        sp1[i] = p1; sp2[i] = p2;
    }
    __syncthreads();
    const int ly = threadIdx.x / JT, lx = threadIdx.x % JT;
    const int y = ty0 + ly, x = tx0 + lx;
    if (y >= H || x >= W) return;
    const int c = (ly + 1) * (JT + 2) + lx + 1, pix = y * W + x;
#pragma unroll
    for (int slot = 0; slot < 2; ++slot) {
        const float* s = slot == 0 ? sp2 : sp1;
        const float v = s[c];
        float mx = v;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) mx = fmaxf(mx, s[c + dy * (JT + 2) + dx]);
        if (v == mx && v > JTH) {
            const int at = atomicAdd(ncand + b * 2 + slot, 1);
            if (at < HW) cand[((int64_t)b * 2 + slot) * HW + at] = make_key(v, pix);
        }
    }
}

// ---- junction selection: grid (2, B), 1024 lanes.  The 300 largest keys by an 8-pass byte radix select (LDS histogram, integer atomics),
// the survivors sorted descending by a bitonic network in LDS, coordinates from the offsets.  Class 2 block first, class 1 behind it.
__global__ __launch_bounds__(1024) void junc_select_kernel(const unsigned long long* __restrict__ cand, const int32_t* __restrict__ ncand,
                                                           Strided joff, int H, int W, float scale_x, float scale_y,
                                                           float* __restrict__ juncs, float* __restrict__ scores, int32_t* __restrict__ index,
                                                           int32_t* __restrict__ counts) {
    __shared__ unsigned long long skey[SORT_N];
    __shared__ int hist[256];
    __shared__ unsigned long long s_prefix;
    __shared__ int s_want, s_fill;
    const int slot = blockIdx.x, b = blockIdx.y, HW = H * W, tid = threadIdx.x;
    const int n = min(ncand[b * 2 + slot], HW);
    const int keep = min(n, TOPK);
    const int base = slot == 0 ? 0 : min(min(ncand[b * 2], HW), TOPK);
    const unsigned long long* keys = cand + ((int64_t)b * 2 + slot) * HW;
    if (tid == 0) { counts[b * 2 + slot] = keep; s_prefix = 0ull; s_want = keep; s_fill = 0; }
    for (int i = tid; i < SORT_N; i += 1024) skey[i] = 0ull;
    __syncthreads();
    if (n > TOPK) {                                     // threshold = the TOPK-th largest key
        for (int pass = 7; pass >= 0; --pass) {
            for (int i = tid; i < 256; i += 1024) hist[i] = 0;
            __syncthreads();
            const unsigned long long prefix = s_prefix;
            const int sh = pass * 8;
            for (int i = tid; i < n; i += 1024) {
                const unsigned long long k = keys[i];
                if (pass == 7 || (k >> (sh + 8)) == (prefix >> (sh + 8))) atomicAdd(&hist[(int)((k >> sh) & 0xFF)], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int want = s_want, bin = 255;
                for (; bin > 0; --bin) {
                    if (hist[bin] >= want) break;
                    want -= hist[bin];
                }
                s_want = want;
                s_prefix = prefix | ((unsigned long long)bin << sh);
            }
            __syncthreads();
        }
    }
    const unsigned long long thr = s_prefix;            // 0 when every candidate is kept
    for (int i = tid; i < n; i += 1024) {
        const unsigned long long k = keys[i];
        if (k >= thr) {
            const int at = atomicAdd(&s_fill, 1);
            if (at < SORT_N) skey[at] = k;
        }
    }
    __syncthreads();
    for (int k = 2; k <= SORT_N; k <<= 1)               // bitonic sort, descending
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (tid < SORT_N) {
                const int ixj = tid ^ j;
                if (ixj > tid) {
                    const unsigned long long a = skey[tid], c = skey[ixj];
                    const bool desc = (tid & k) == 0;
                    if (desc ? a < c : a > c) { skey[tid] = c; skey[ixj] = a; }
                }
            }
            __syncthreads();
        }
    if (tid < keep) {
        const unsigned long long k = skey[tid];
        const int idx = (int)(0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFull));
        const float p = __uint_as_float((uint32_t)(k >> 32));
        const float ox = 1.f / (1.f + expf(-joff.at(b, 0, idx))) - 0.5f;       // model_hisup.py:251
        const float oy = 1.f / (1.f + expf(-joff.at(b, 1, idx))) - 0.5f;
        const float x = ((float)(idx % W) + ox) + 0.5f, y = ((float)(idx / W) + oy) + 0.5f;   // polygon.py:19-20
        const int64_t o = (int64_t)b * 2 * TOPK + base + tid;
        juncs[o * 2] = x * scale_x;
        juncs[o * 2 + 1] = y * scale_y;
        scores[o] = p;
        index[o] = idx;
    }
}

// ================================================================================================ regions
__device__ __forceinline__ int ld_relaxed(const int32_t* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

__device__ __forceinline__ int uf_find(const int32_t* L, int x) {
    for (int p = ld_relaxed(L + x); p != x; p = ld_relaxed(L + x)) x = p;      // parents only ever decrease: terminates
    return x;
}

// link the trees of a and b; the larger root is hung below the smaller one, so a component's root is its first pixel in raster order
__device__ __forceinline__ void uf_union(int32_t* L, int a, int b) {
    bool done = false;
    while (!done) {
        a = uf_find(L, a); b = uf_find(L, b);
        if (a == b) break;
        if (a < b) { const int t = a; a = b; b = t; }   // a > b
        const int old = atomicMin(L + a, b);
        done = old == a;
        a = old;
    }
}

// mask = softmax(remask)[:, 1]; parent = own flat index on foreground (mask > 0.5), -1 elsewhere; region statistics reset
__global__ __launch_bounds__(256) void region_init_kernel(Strided remask, int B, int HW, int max_regions, float* __restrict__ mask,
                                                          int32_t* __restrict__ parent, int32_t* __restrict__ area, int32_t* __restrict__ bbox,
                                                          unsigned long long* __restrict__ sums) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, total = (int64_t)B * HW;
    for (int64_t r = gid; r < (int64_t)B * max_regions; r += (int64_t)gridDim.x * 256) {
        area[r] = 0; sums[r] = 0ull;
        bbox[r * 4] = 0x7fffffff; bbox[r * 4 + 1] = 0x7fffffff; bbox[r * 4 + 2] = 0; bbox[r * 4 + 3] = 0;
    }
    if (gid >= total) return;
    const int b = (int)(gid / HW), pix = (int)(gid % HW);
    const float l0 = remask.at(b, 0, pix), l1 = remask.at(b, 1, pix);
    const float m = fmaxf(l0, l1);
    const float e0 = expf(l0 - m), e1 = expf(l1 - m);
    const float p = e1 / (e0 + e1);
    mask[gid] = p;
    parent[gid] = p > 0.5f ? pix : -1;
}

// 8-connectivity: every foreground pixel joins its W, NW, N and NE neighbours (the other four are joined from their side)
__global__ __launch_bounds__(256) void region_merge_kernel(int32_t* __restrict__ parent, int B, int H, int W) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int HW = H * W;
    if (gid >= (int64_t)B * HW) return;
    int32_t* L = parent + (gid / HW) * HW;
    const int pix = (int)(gid % HW), y = pix / W, x = pix % W;
    if (ld_relaxed(L + pix) < 0) return;
    if (x > 0 && ld_relaxed(L + pix - 1) >= 0) uf_union(L, pix, pix - 1);
    if (y > 0) {
        if (ld_relaxed(L + pix - W) >= 0) uf_union(L, pix, pix - W);
        else {                                           // with N set, NW and NE are already joined through it
            if (x > 0 && ld_relaxed(L + pix - W - 1) >= 0) uf_union(L, pix, pix - W - 1);
            if (x + 1 < W && ld_relaxed(L + pix - W + 1) >= 0) uf_union(L, pix, pix - W + 1);
        }
    }
}

// one 1024-lane workgroup per image: number the roots 1..n in raster order (rank[root] = number), n_regions, status (1: n > max_regions)
__global__ __launch_bounds__(1024) void region_rank_kernel(const int32_t* __restrict__ parent, int32_t* __restrict__ rank, int HW, int max_regions,
                                                           int32_t* __restrict__ n_regions, int32_t* __restrict__ status) {
    __shared__ int part[1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int32_t* L = parent + (int64_t)b * HW;
    int32_t* R = rank + (int64_t)b * HW;
    const int per = (HW + 1023) / 1024;
    const int i0 = min(tid * per, HW), i1 = min(i0 + per, HW);
    int cnt = 0;
    for (int i = i0; i < i1; ++i) cnt += L[i] == i;
    part[tid] = cnt;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                // inclusive scan
        const int v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - cnt;
    for (int i = i0; i < i1; ++i) {
        const bool root = L[i] == i;
        run += root;
        R[i] = root ? run : 0;
    }
    if (tid == 1023) { n_regions[b] = part[1023]; status[b] = part[1023] > max_regions ? 1 : 0; }
}

// labels + statistics.  Integer atomics only; a wave whose foreground lanes all carry one label (the common case inside a building)
// combines in registers and issues one set of atomics.
__global__ __launch_bounds__(256) void region_final_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ rank,
                                                           const float* __restrict__ mask, int B, int H, int W, int max_regions,
                                                           int32_t* __restrict__ labels, int32_t* __restrict__ area, int32_t* __restrict__ bbox,
                                                           unsigned long long* __restrict__ sums) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int HW = H * W;
    const bool in = gid < (int64_t)B * HW;
    int lab = 0, b = 0, y = 0, x = 0;
    unsigned long long q = 0ull;
    if (in) {
        b = (int)(gid / HW);
        const int pix = (int)(gid % HW);
        y = pix / W; x = pix % W;
        const int32_t* L = parent + (int64_t)b * HW;
        if (L[pix] >= 0) {
            lab = rank[(int64_t)b * HW + uf_find(L, pix)];
            q = (unsigned long long)((double)mask[gid] * 4294967296.0 + 0.5);      // 32.32 fixed point, exact for an fp32 in (0.5, 1]
        }
        labels[gid] = lab;
    }
    const bool act = lab > 0 && lab <= max_regions;
    const int64_t key = act ? (int64_t)b * max_regions + (lab - 1) : -1;
    const unsigned long long ballot = __ballot(act);
    if (ballot == 0ull) return;
    const int leader = __ffsll((long long)ballot) - 1;
    const int64_t key0 = __shfl(key, leader, 64);
    if (__all(!act || key == key0)) {
        int a = act ? 1 : 0, y0 = act ? y : 0x7fffffff, x0 = act ? x : 0x7fffffff, y1 = act ? y + 1 : 0, x1 = act ? x + 1 : 0;
        unsigned long long s = act ? q : 0ull;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_xor(a, o, 64);
            s += __shfl_xor(s, o, 64);
            y0 = min(y0, __shfl_xor(y0, o, 64)); x0 = min(x0, __shfl_xor(x0, o, 64));
            y1 = max(y1, __shfl_xor(y1, o, 64)); x1 = max(x1, __shfl_xor(x1, o, 64));
        }
        if ((int)(threadIdx.x & 63) == leader) {
            atomicAdd(area + key0, a);
            atomicAdd(sums + key0, s);
            atomicMin(bbox + key0 * 4, y0); atomicMin(bbox + key0 * 4 + 1, x0);
            atomicMax(bbox + key0 * 4 + 2, y1); atomicMax(bbox + key0 * 4 + 3, x1);
        }
    } else if (act) {
        atomicAdd(area + key, 1);
        atomicAdd(sums + key, q);
        atomicMin(bbox + key * 4, y); atomicMin(bbox + key * 4 + 1, x);
        atomicMax(bbox + key * 4 + 2, y + 1); atomicMax(bbox + key * 4 + 3, x + 1);
    }
}

__global__ __launch_bounds__(256) void region_score_kernel(const int32_t* __restrict__ area, const unsigned long long* __restrict__ sums,
                                                           float* __restrict__ score, int32_t* __restrict__ bbox, int64_t n) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int a = area[r];
    score[r] = a > 0 ? (float)((double)sums[r] * (1.0 / 4294967296.0) / (double)a) : 0.f;
    if (a == 0) { bbox[r * 4] = 0; bbox[r * 4 + 1] = 0; }
}

// ================================================================================================ validation losses
// the per-pixel arithmetic lives in hisup_loss_pixel.h, shared with p3_hisup_train_loss (hisup_loss.hip)
constexpr int VL_PIX = hisup_px::PIX;
constexpr int VL_N = hisup_px::NPART;

// grid (ceil(HW / VL_PIX), B); parts [B, nblk, VL_N]
__global__ __launch_bounds__(256) void val_loss_partial_kernel(const float* __restrict__ jloc, const float* __restrict__ joff,
                                                               const float* __restrict__ mask, const float* __restrict__ afm,
                                                               const float* __restrict__ remask, const int64_t* __restrict__ t_jloc,
                                                               const float* __restrict__ t_joff, const float* __restrict__ t_mask,
                                                               const float* __restrict__ t_afm, int HW, float* __restrict__ parts) {
    __shared__ float red[4][VL_N];
    const int b = blockIdx.y;
    float acc[VL_N] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int p0 = blockIdx.x * VL_PIX;
    for (int k = 0; k < VL_PIX / 256; ++k) {
        const int pix = p0 + k * 256 + threadIdx.x;
        if (pix >= HW) break;
        const int64_t o1 = (int64_t)b * HW + pix, o2 = (int64_t)b * 2 * HW + pix, o3 = (int64_t)b * 3 * HW + pix;
        const int64_t tj = t_jloc[o1];
        acc[0] += hisup_px::ce3(jloc[o3], jloc[o3 + HW], jloc[o3 + 2 * (int64_t)HW], tj);
        const int tm = hisup_px::mask_class(t_mask[o1]);
        acc[1] += hisup_px::ce2(mask[o2], mask[o2 + HW], tm);
        acc[2] += hisup_px::ce2(remask[o2], remask[o2 + HW], tm);
        acc[3] += fabsf(afm[o2] - t_afm[o2]) + fabsf(afm[o2 + HW] - t_afm[o2 + HW]);
        if (hisup_px::is_junction(tj)) {
            acc[4] += fabsf(hisup_px::joff_residual(hisup_px::sigmoidf(joff[o2]), t_joff[o2])) +
                      fabsf(hisup_px::joff_residual(hisup_px::sigmoidf(joff[o2 + HW]), t_joff[o2 + HW]));
            acc[5] += 1.f;
        }
    }
#pragma unroll
    for (int i = 0; i < VL_N; ++i) {
        const float v = wave_sum(acc[i]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < VL_N)
        parts[((int64_t)b * gridDim.x + blockIdx.x) * VL_N + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// one workgroup: partials summed in workgroup order in float64 -> out[5] = loss_jloc, loss_joff, loss_mask, loss_afm, loss_remask
__global__ __launch_bounds__(256) void val_loss_final_kernel(const float* __restrict__ parts, int B, int nblk, int HW, float* __restrict__ out) {
    __shared__ double tot[VL_N];
    if (threadIdx.x < VL_N) {
        const int i = threadIdx.x;
        double t = 0.0;
        for (int b = 0; b < B; ++b) {
            double s = 0.0, c = 0.0;
            for (int k = 0; k < nblk; ++k) {
                s += (double)parts[((int64_t)b * nblk + k) * VL_N + i];
                if (i == 4) c += (double)parts[((int64_t)b * nblk + k) * VL_N + 5];
            }
            if (i == 4 && c > 0.0) s = s * (double)HW / c;     // sigmoid_l1_loss: loss * t / w, w = share of junction pixels, w == 0 -> 1
            t += s;
        }
        tot[i] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double n1 = (double)B * HW, n2 = 2.0 * n1;
        out[0] = (float)(tot[0] / n1);
        out[1] = (float)(tot[4] / n2);
        out[2] = (float)(tot[1] / n1);
        out[3] = (float)(tot[3] / n2);
        out[4] = (float)(tot[2] / n1);
    }
}

constexpr int64_t MAX_HW = 1 << 22;

}  // namespace

extern "C" int64_t p3_hisup_junctions_workspace_bytes(int B, int H, int W) {
    return (int64_t)B * 2 * H * W * 8 + (int64_t)B * 2 * 4;
}

extern "C" int p3_hisup_junctions(const float* jloc, int64_t jloc_sb, int64_t jloc_sc, int64_t jloc_sp, const float* joff, int64_t joff_sb,
                                  int64_t joff_sc, int64_t joff_sp, int B, int H, int W, float scale_x, float scale_y, float* juncs,
                                  float* scores, int32_t* index, int32_t* counts, void* workspace, void* stream) {
    P3_CHECK(jloc && joff && juncs && scores && index && counts && workspace, P3_EINVAL, "p3_hisup_junctions: null pointer");
    P3_CHECK(B > 0 && H > 0 && W > 0 && (int64_t)H * W <= MAX_HW, P3_ESHAPE, "p3_hisup_junctions: bad sizes (H * W <= 2^22)");
    hipStream_t s = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W;
    unsigned long long* cand = (unsigned long long*)workspace;
    int32_t* ncand = (int32_t*)(cand + (int64_t)B * 2 * HW);
    hipError_t e = hipMemsetAsync(ncand, 0, (size_t)B * 2 * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(juncs, 0, (size_t)B * 2 * TOPK * 2 * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(scores, 0, (size_t)B * 2 * TOPK * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(index, 0xFF, (size_t)B * 2 * TOPK * 4, s);
    if (e != hipSuccess) { p3_set_error(hipGetErrorString(e)); return (int)e; }
    const int tx = p3_ceil_div(W, JT), ty = p3_ceil_div(H, JT);
    const Strided jl{jloc, jloc_sb, jloc_sc, jloc_sp}, jo{joff, joff_sb, joff_sc, joff_sp};
    hipLaunchKernelGGL(junc_candidates_kernel, dim3(tx * ty, B), dim3(256), 0, s, jl, H, W, tx, cand, ncand);
    P3_LAUNCH_CHECK();
    hipLaunchKernelGGL(junc_select_kernel, dim3(2, B), dim3(1024), 0, s, cand, ncand, jo, H, W, scale_x, scale_y, juncs, scores, index, counts);
    P3_LAUNCH_CHECK();
    return P3_OK;
}

extern "C" int64_t p3_hisup_regions_workspace_bytes(int B, int H, int W, int max_regions) {
    return (int64_t)B * H * W * 4 * 2 + (int64_t)B * max_regions * 8;
}

extern "C" int p3_hisup_regions(const float* remask, int64_t sb, int64_t sc, int64_t sp, int B, int H, int W, int max_regions, float* mask,
                                int32_t* labels, int32_t* n_regions, int32_t* area, int32_t* bbox, float* score, int32_t* status,
                                void* workspace, void* stream) {
    P3_CHECK(remask && mask && labels && n_regions && area && bbox && score && status && workspace, P3_EINVAL, "p3_hisup_regions: null pointer");
    P3_CHECK(B > 0 && H > 0 && W > 0 && (int64_t)H * W <= MAX_HW && max_regions > 0, P3_ESHAPE, "p3_hisup_regions: bad sizes (H * W <= 2^22)");
    hipStream_t s = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W, total = (int64_t)B * HW;
    unsigned long long* sums = (unsigned long long*)workspace;
    int32_t* parent = (int32_t*)(sums + (int64_t)B * max_regions);
    int32_t* rank = parent + total;
    const int grid = p3_ceil_div(total, 256);
    const Strided rm{remask, sb, sc, sp};
    hipLaunchKernelGGL(region_init_kernel, dim3(grid), dim3(256), 0, s, rm, B, (int)HW, max_regions, mask, parent, area, bbox, sums);
    P3_LAUNCH_CHECK();
    hipLaunchKernelGGL(region_merge_kernel, dim3(grid), dim3(256), 0, s, parent, B, H, W);
    P3_LAUNCH_CHECK();
    hipLaunchKernelGGL(region_rank_kernel, dim3(B), dim3(1024), 0, s, parent, rank, (int)HW, max_regions, n_regions, status);
    P3_LAUNCH_CHECK();
    hipLaunchKernelGGL(region_final_kernel, dim3(grid), dim3(256), 0, s, parent, rank, mask, B, H, W, max_regions, labels, area, bbox, sums);
    P3_LAUNCH_CHECK();
    hipLaunchKernelGGL(region_score_kernel, dim3(p3_ceil_div((int64_t)B * max_regions, 256)), dim3(256), 0, s, area, sums, score, bbox,
                       (int64_t)B * max_regions);
    P3_LAUNCH_CHECK();
    return P3_OK;
}

extern "C" int64_t p3_hisup_val_loss_workspace_bytes(int B, int H, int W) {
    return (int64_t)B * p3_ceil_div((int64_t)H * W, VL_PIX) * VL_N * 4;
}

extern "C" int p3_hisup_val_loss(const float* jloc, const float* joff, const float* mask, const float* afm, const float* remask,
                                 const int64_t* t_jloc, const float* t_joff, const float* t_mask, const float* t_afm, int B, int H, int W,
                                 float* losses, void* workspace, void* stream) {
    P3_CHECK(jloc && joff && mask && afm && remask && t_jloc && t_joff && t_mask && t_afm && losses && workspace, P3_EINVAL,
             "p3_hisup_val_loss: null pointer");
    P3_CHECK(B > 0 && H > 0 && W > 0 && (int64_t)H * W <= MAX_HW, P3_ESHAPE, "p3_hisup_val_loss: bad sizes (H * W <= 2^22)");
    hipStream_t s = (hipStream_t)stream;
    const int HW = H * W, nblk = p3_ceil_div(HW, VL_PIX);
    hipLaunchKernelGGL(val_loss_partial_kernel, dim3(nblk, B), dim3(256), 0, s, jloc, joff, mask, afm, remask, t_jloc, t_joff, t_mask, t_afm, HW,
                       (float*)workspace);
    P3_LAUNCH_CHECK();
    hipLaunchKernelGGL(val_loss_final_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, B, nblk, HW, losses);
    P3_LAUNCH_CHECK();
    return P3_OK;
}
