// p3hip weight-gradient GEMM on PLANES (include/p3hip.h, p3_gemm_tn_x3):  C[N,K] += (a_hi + a_lo)[M,N]^T (b_hi + b_lo)[M,K], three bf16 MFMAs per product
//
// gemm_tn_dma.hip's schedule on tn_dma_tile.h with both operands arriving split (the producers wrote hi = bf16(x), lo = bf16(x - hi)): every plane is an image
// of its own, a wave reads the four fragment sets and accumulates a_lo b_hi + a_hi b_lo + a_hi b_hi: the P3_F32X3 arithmetic (gemm_tn.hip SPLIT: fp32 operands
// split while they are staged through registers, 248 - 250 us per fc1 / fc2 weight gradient) at the bf16 kernel's memory path.  Two kernels, both with FOUR
// steps of 32 KB in LDS, three in flight (r05 PMC of the two-step 64-row form: waves parked 37 % of their cycles in s_waitcnt / s_barrier, the matrix pipe
// 40 % busy), one workgroup of 512 threads per CU:
//   gemm_tn_x3_kernel       128 x 128 tile, 32-row steps of four images (a_hi | a_lo | b_hi | b_lo); two groups of four waves on the SAME output tile,
//                           group g multiplies rows 16 g .. 16 g + 15 of every step, the groups fold through LDS at the end;
//   gemm_tn_x3_wide_kernel  128 x 384 tile, 16-row steps of eight images, every wave on all rows (below).
#include <stdlib.h>

#include "tn_dma_tile.h"

namespace {

constexpr int TD_BM = 32;                       // rows of m per step
constexpr int TD_IMG = TD_BM * 256;             // one operand image of a step
constexpr int TD_STEP_BYTES = 4 * TD_IMG;       // a_hi | a_lo | b_hi | b_lo

template <int NBUF>
__global__ __launch_bounds__(512, 2) void gemm_tn_x3_kernel(TnDmaArgs g) {
    constexpr int LA = NBUF - 1;
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, w4 = wave & 3, wm = w4 >> 1, wn = w4 & 1;
    const TnTile t = tn_tile_of<TD_BM>(g);
    const uint32_t lds_addr = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)lds_raw);

    // ---- staging: an image = 8 pieces; wave w issues the four pieces (w & 1) * 4 .. + 3 of image w >> 1 (a_hi, a_lo, b_hi, b_lo)
    const int img = wave >> 1;
    const bf16_t* src = img == 0 ? g.A : (img == 1 ? g.Al : (img == 2 ? g.B : g.Bl));
    const int sld = img < 2 ? g.lda : g.ldb, scol = img < 2 ? t.tn * 128 : td_conv_b(g, t.tk * 128, src);
    uint32_t voff[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) voff[q] = tn_piece_src(lane, ((wave & 1) * 4 + q) * 4, sld, scol);
    auto stage = [&](int st) __attribute__((always_inline)) {      // step st -> buffer st % NBUF (caller: st < nsteps)
        const int64_t m0 = (int64_t)t.m_beg + (int64_t)st * TD_BM;
        const uint32_t da = lds_addr + (uint32_t)((st % NBUF) * TD_STEP_BYTES + wave * 4096);
        lds_dma16x2(src + m0 * sld, da, voff[0], voff[1]);
        lds_dma16x2(src + m0 * sld, da + 2048, voff[2], voff[3]);
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // ---- fragments: wave (wm, wn) of group grp multiplies the 32-column blocks wm * 2 + i of A and wn * 2 + j of B over the step's rows 16 grp .. + 15
    // (one 16-deep MFMA block); the lo image lies TD_IMG behind the hi image
    uint32_t offA[2], offB[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        offA[i] = lds_addr + tn_tr_off(lane, grp * 16, wm * 2 + i);
        offB[i] = lds_addr + 2 * TD_IMG + tn_tr_off(lane, grp * 16, wn * 2 + i);
    }
    // bias gradient: column sums of A = a_hi + a_lo by the tk == 0 tiles (thread -> chunk tid % 16 of row tid / 16 of both images)
    const bool do_cs = g.colsum != nullptr && t.tk == 0;
    float csum[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) csum[q] = 0.f;

    tn_pipe_fill<LA>(t.nsteps, stage);
    for (int st = 0; st < t.nsteps; ++st) {
        tn_pipe_wait<LA>(st, t.nsteps);
        __builtin_amdgcn_s_barrier();
        if (st + LA < t.nsteps) stage(st + LA);
        const uint32_t bo = (uint32_t)((st % NBUF) * TD_STEP_BYTES);
        if (do_cs) {
#pragma unroll
            for (int im = 0; im < 2; ++im) tn_colsum_add(csum, lds_raw + bo + im * TD_IMG, tid >> 4, tid & 15);
        }
        u32x2_t fah[2][2], fal[2][2], fbh[2][2], fbl[2][2];            // [32-column block][rows +0..3 | +4..7]
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const uint32_t ro = bo + (uint32_t)(hh * 4 * 256);
                lds_read_tr16_b64(fah[i][hh], offA[i] + ro);
                lds_read_tr16_b64(fal[i][hh], offA[i] + ro + TD_IMG);
                lds_read_tr16_b64(fbh[i][hh], offB[i] + ro);
                lds_read_tr16_b64(fbl[i][hh], offB[i] + ro + TD_IMG);
            }
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(fah[0][0]), "+v"(fah[0][1]), "+v"(fah[1][0]), "+v"(fah[1][1]), "+v"(fal[0][0]), "+v"(fal[0][1]), "+v"(fal[1][0]), "+v"(fal[1][1]),
                       "+v"(fbh[0][0]), "+v"(fbh[0][1]), "+v"(fbh[1][0]), "+v"(fbh[1][1]), "+v"(fbl[0][0]), "+v"(fbl[0][1]), "+v"(fbl[1][0]), "+v"(fbl[1][1]));
        __builtin_amdgcn_sched_barrier(0);
        bf16x8_t ah[2], al[2], bh[2], bl[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            ah[i] = tr_frag(fah[i][0], fah[i][1]);
            al[i] = tr_frag(fal[i][0], fal[i][1]);
            bh[i] = tr_frag(fbh[i][0], fbh[i][1]);
            bl[i] = tr_frag(fbl[i][0], fbl[i][1]);
        }
        tn_mma_x3(acc, ah, al, bh, bl);
    }
    wait_vm_lgkm0<0>();
    __builtin_amdgcn_s_barrier();                   // every wave is done with the operand images: the epilogue reuses the LDS

    float* red = reinterpret_cast<float*>(lds_raw);
    if (do_cs) {                                     // wave-uniform (tk is)
        tn_colsum_fold<32>(g, t, red, csum, tid);
        __syncthreads();                             // the group exchange takes `red`
    }
    f32x16 out[2];                                   // group grp finishes the row block i = grp of its waves' tiles
    if (grp == 0) tn_fold_groups<0>(out, acc, red, w4, lane);
    else tn_fold_groups<1>(out, acc, red, w4, lane);
#pragma unroll
    for (int j = 0; j < 2; ++j) tn_commit(g, t.split, t.tn * 128 + wm * 64 + grp * 32, t.tk * 128 + wn * 64 + j * 32, out[j], lane);
}

// ---- the WIDE tile: 128 (n) x 384 (k) per workgroup, every wave on all rows ---------------------------------------------------------------------------------
// What bounds the 128 x 128 kernel above is the CU's address path: a 32-row step is 32 LDS-DMA pieces (1 KB each, ~40 cycles of that path per piece) for 96 MFMAs
// - 1280 cycles of staging against 768 of matrix pipe per SIMD (r05 PMC: pipe 39 % busy).  Here the two wave groups no longer split the ROWS of one tile (which
// staged every byte for half the MFMAs): the 8 waves tile a 128 x 384 output as 2 x 4 sub-tiles of 64 x 96, a step is 16 rows = one 16-deep MFMA block of
// EIGHT images (a_hi, a_lo, three 128-column blocks of b_hi and of b_lo) = 32 pieces for 8 x 18 MFMAs: 1280 cycles of staging against 1152 of pipe.  No fold
// between groups at the end.  Shapes: N % 128 == 0, K % 384 == 0 - fc1 (1536 x 384), fc2 (384 x 1536), qkv (1152 x 384) of the timm Block.
constexpr int TW_BM = 16;                       // rows of m per step
constexpr int TW_IMG = TW_BM * 256;             // one image of a step: 16 rows x 128 columns
constexpr int TW_STEP_BYTES = 8 * TW_IMG;       // 32 KB

template <int NBUF>
__global__ __launch_bounds__(512, 2) void gemm_tn_x3_wide_kernel(TnDmaArgs g) {
    constexpr int LA = NBUF - 1;
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;          // sub-tile: rows wm * 64 .. + 63 of n, columns wn * 96 .. + 95 of k
    const TnTile t = tn_tile_of<TW_BM>(g);
    const uint32_t lds_addr = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)lds_raw);

    // ---- staging: an image = 4 pieces; wave w stages image w of every step (0: a_hi, 1: a_lo, 2 + 2 c: b_hi block c, 3 + 2 c: b_lo block c)
    const bf16_t* src = wave == 0 ? g.A : (wave == 1 ? g.Al : ((wave & 1) ? g.Bl : g.B));
    const int sld = wave < 2 ? g.lda : g.ldb, scol = wave < 2 ? t.tn * 128 : td_conv_b(g, t.tk * 384, src) + ((wave - 2) >> 1) * 128;
    uint32_t voff[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) voff[q] = tn_piece_src(lane, q * 4, sld, scol);
    auto stage = [&](int st) __attribute__((always_inline)) {
        const int64_t m0 = (int64_t)t.m_beg + (int64_t)st * TW_BM;
        const uint32_t da = lds_addr + (uint32_t)((st % NBUF) * TW_STEP_BYTES + wave * TW_IMG);
        lds_dma16x2(src + m0 * sld, da, voff[0], voff[1]);
        lds_dma16x2(src + m0 * sld, da + 2048, voff[2], voff[3]);
    };

    f32x16 acc[2][3];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // ---- fragments: the wave's A blocks are granules wm * 2 + i of image 0 / 1; its B blocks: column c = wn * 96 + j * 32 -> image 2 + 2 (c / 128),
    // granule (c % 128) / 32; the lo image lies TW_IMG behind the hi image
    uint32_t offA[2], offB[3];
#pragma unroll
    for (int i = 0; i < 2; ++i) offA[i] = lds_addr + tn_tr_off(lane, 0, wm * 2 + i);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int c = wn * 96 + j * 32;
        offB[j] = lds_addr + (uint32_t)((2 + 2 * (c >> 7)) * TW_IMG) + tn_tr_off(lane, 0, (c & 127) >> 5);
    }
    // bias gradient: column sums of A by the tk == 0 tiles (thread -> chunk tid % 16 of row tid / 16 of both images: threads 0..255 cover the 16 rows)
    const bool do_cs = g.colsum != nullptr && t.tk == 0;
    float csum[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) csum[q] = 0.f;

    tn_pipe_fill<LA>(t.nsteps, stage);
    for (int st = 0; st < t.nsteps; ++st) {
        tn_pipe_wait<LA>(st, t.nsteps);
        __builtin_amdgcn_s_barrier();
        if (st + LA < t.nsteps) stage(st + LA);
        const uint32_t bo = (uint32_t)((st % NBUF) * TW_STEP_BYTES);
        if (do_cs && tid < 256) {
#pragma unroll
            for (int im = 0; im < 2; ++im) tn_colsum_add(csum, lds_raw + bo + im * TW_IMG, tid >> 4, tid & 15);
        }
        u32x2_t fah[2][2], fal[2][2], fbh[3][2], fbl[3][2];            // [32-column block][rows +0..3 | +4..7]
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const uint32_t ro = bo + (uint32_t)(hh * 4 * 256);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                lds_read_tr16_b64(fah[i][hh], offA[i] + ro);
                lds_read_tr16_b64(fal[i][hh], offA[i] + ro + TW_IMG);
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                lds_read_tr16_b64(fbh[j][hh], offB[j] + ro);
                lds_read_tr16_b64(fbl[j][hh], offB[j] + ro + TW_IMG);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(fah[0][0]), "+v"(fah[0][1]), "+v"(fah[1][0]), "+v"(fah[1][1]), "+v"(fal[0][0]), "+v"(fal[0][1]), "+v"(fal[1][0]), "+v"(fal[1][1]),
                       "+v"(fbh[0][0]), "+v"(fbh[0][1]), "+v"(fbh[1][0]), "+v"(fbh[1][1]), "+v"(fbh[2][0]), "+v"(fbh[2][1]),
                       "+v"(fbl[0][0]), "+v"(fbl[0][1]), "+v"(fbl[1][0]), "+v"(fbl[1][1]), "+v"(fbl[2][0]), "+v"(fbl[2][1]));
        __builtin_amdgcn_sched_barrier(0);
        bf16x8_t ah[2], al[2], bh[3], bl[3];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            ah[i] = tr_frag(fah[i][0], fah[i][1]);
            al[i] = tr_frag(fal[i][0], fal[i][1]);
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            bh[j] = tr_frag(fbh[j][0], fbh[j][1]);
            bl[j] = tr_frag(fbl[j][0], fbl[j][1]);
        }
        tn_mma_x3(acc, ah, al, bh, bl);
    }
    wait_vm_lgkm0<0>();
    __builtin_amdgcn_s_barrier();                   // every wave is done with the operand images: the bias fold reuses the LDS

    if (do_cs) tn_colsum_fold<TW_BM>(g, t, reinterpret_cast<float*>(lds_raw), csum, tid);          // wave-uniform (tk is)
    // ---- the wave's 64 x 96 sub-tile
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) tn_commit(g, t.split, t.tn * 128 + wm * 64 + i * 32, t.tk * 384 + wn * 96 + j * 32, acc[i][j], lane);
}

}  // namespace

static int g_tn_wide = 1;
extern "C" int p3_gemm_tn_x3_wide(int on) { const int was = g_tn_wide; g_tn_wide = on; return was; }

static int tn_x3_launch(const void* a_hi, const void* a_lo, int lda, const void* b_hi, const void* b_lo, int ldb, float* C, int ldc, int M, int N, int K,
                        float* colsum, float* slabs, int max_slabs, int conv_ci, int conv_pw, void* stream) {
    P3_CHECK(a_hi && a_lo && b_hi && b_lo && C && M > 0 && N > 0 && K > 0, P3_EINVAL, "p3_gemm_tn_x3: bad arguments");
    P3_CHECK(M % TD_BM == 0 && N % 128 == 0 && K % 128 == 0, P3_ESHAPE, "p3_gemm_tn_x3: M % 32 == 0, N % 128 == 0, K % 128 == 0");
    P3_CHECK(lda % 8 == 0 && ldb % 8 == 0 && ((uintptr_t)a_hi | (uintptr_t)a_lo | (uintptr_t)b_hi | (uintptr_t)b_lo) % 16 == 0, P3_EALIGN, "p3_gemm_tn_x3: 16-byte rows");
    P3_CHECK((int64_t)TD_BM * lda * 2 + 256 < (1ll << 31) && (int64_t)TD_BM * ldb * 2 + 256 < (1ll << 31), P3_EUNSUP, "p3_gemm_tn_x3: row stride beyond the 32-bit DMA offsets");
    hipStream_t s = (hipStream_t)stream;
    TnDmaArgs g;
    g.A = (const bf16_t*)a_hi; g.Al = (const bf16_t*)a_lo; g.B = (const bf16_t*)b_hi; g.Bl = (const bf16_t*)b_lo; g.C = C;
    g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.colsum = colsum;
    g.conv_ci = conv_ci; g.conv_pw = conv_pw;
    const int tiles_n = N / 128;
    // the wide tile (128 x 384, every wave on all rows) where K is a multiple of 384 and there are enough tiles for its split count to stay moderate
    // (p3_gemm_tn_x3_wide(0) switches it off: same-box A/B, tools/mb_x3.py)
    const bool wide = g_tn_wide && K % 384 == 0 && tiles_n * (K / 384) >= 8 && conv_ci % 384 == 0;       // conv: a column tile lies inside one tap
    g.tiles_k = wide ? K / 384 : K / 128;
    const int tiles = tiles_n * g.tiles_k;
    P3_CHECK(tiles <= 256, P3_EUNSUP, "p3_gemm_tn_x3: more than 256 output tiles");
    // the wide kernel's plan counts in the 32-row steps of the 128 x 128 kernel too, although its own are 16 rows: its splits are never shorter than 64 rows and
    // a multiple of 32.  That is what it was measured with and what the deterministic results are pinned to; it stays.
    const TnSplitPlan plan = tn_split_plan(M, tiles, TD_BM, slabs != nullptr, max_slabs);
    g.splits = plan.splits; g.rows_per_split = plan.rows_per_split;
    const TnParts parts = p3_tn_parts(C, N, K, ldc, plan.splits, slabs, colsum, P3_F32);
    g.slabs = parts.slabs; g.cs_slab = parts.cs_slab;
    constexpr int NBUF = 4;
    const size_t lds = (size_t)NBUF * TD_STEP_BYTES;       // 4 x 32 KB (>= the 64 KB the fold needs); the wide kernel's steps are 32 KB too
    static_assert(TW_STEP_BYTES == TD_STEP_BYTES, "one LDS size for both kernels");
    dim3 grid(tiles * plan.splits), block(512);
    const int rc = !wide ? p3_launch<gemm_tn_x3_kernel<NBUF>>("gemm_tn_x3_kernel<4>", grid, block, lds, s, g)
                         : p3_launch<gemm_tn_x3_wide_kernel<NBUF>>("gemm_tn_x3_wide_kernel<4>", grid, block, lds, s, g);
    if (rc != P3_OK) return rc;
    return p3_tn_parts_reduce(parts, C, N, K, ldc, plan.splits, colsum, s);
}

extern "C" int p3_gemm_tn_x3(const void* a_hi, const void* a_lo, int lda, const void* b_hi, const void* b_lo, int ldb, float* C, int ldc, int M, int N, int K,
                             float* colsum, float* slabs, int max_slabs, void* stream) {
    return tn_x3_launch(a_hi, a_lo, lda, b_hi, b_lo, ldb, C, ldc, M, N, K, colsum, slabs, max_slabs, 0, 0, stream);
}

// the nine taps of a 3 x 3 convolution's weight gradient as column tiles of ONE launch (include/p3hip.h): K = 9 * Ci output columns, the B rows of a tile shifted by
// its tap's constant row offset in the zero-bordered row space.  The caller owns the Pw + 1 zero guard rows in front of and behind B.
extern "C" int p3_gemm_tn_x3_conv(const void* a_hi, const void* a_lo, int lda, const void* b_hi, const void* b_lo, int ldb, float* C, int ldc, int M, int N, int Ci,
                                  int Pw, float* slabs, int max_slabs, void* stream) {
    P3_CHECK(Ci > 0 && Ci % 128 == 0 && Pw >= 3, P3_ESHAPE, "p3_gemm_tn_x3_conv: Ci % 128 == 0, Pw >= 3");
    P3_CHECK(M % 64 == 0, P3_ESHAPE, "p3_gemm_tn_x3_conv: M % 64 == 0");
    return tn_x3_launch(a_hi, a_lo, lda, b_hi, b_lo, ldb, C, ldc, M, N, 9 * Ci, nullptr, slabs, max_slabs, Ci, Pw, stream);
}
