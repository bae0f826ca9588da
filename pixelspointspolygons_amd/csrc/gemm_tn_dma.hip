// p3hip weight-gradient GEMM, LDS-DMA form:  C[N,K] += A[M,N]^T * B[M,K]  (bf16 operands, fp32 accumulate, split over M), on tn_dma_tile.h
//
// The register-staged kernel of gemm_tn.hip (128 x 128 tile, 4 waves, two workgroups per CU) pays per 64-row step and workgroup 32 KB of
// ds_write_b128 at the LDS store rate (~13 cycles per wave-instruction: ~830 cycles per CU and step pair) next to 512 cycles of transposing
// reads - the LDS pipe, not the MFMA pipe (1024 cycles), is its busiest unit - and ends in one fp32 atomic per accumulator of EVERY resident
// workgroup (448 x 16 K = 7.3 M per launch whose lines migrate between the XCDs' L2s: 15 - 20 us of a 60 - 80 us launch, r03).  Here:
//   * the operands arrive by LDS-DMA (the tile header's image); a step = 64 rows of m = an A image | a B image, 16 KB each;
//   * ONE 512-thread workgroup per CU = two groups of four waves that work on the SAME output tile: group g multiplies rows 32 g .. 32 g + 31 of
//     every step; at the end the groups exchange halves of their accumulators through LDS, so a CU issues 16 K atomics instead of 32 K at the
//     same number of resident waves (the M split count halves);
//   * NBUF steps in LDS (32 KB each), NBUF - 1 in flight.
// Shapes: M % 64 == 0, N % 128 == 0, K % 128 == 0 (every plain-operand weight gradient of the path at its bench batch); anything else, the fp32
// parity mode and the generated-B forms stay on gemm_tn.hip.  The arithmetic per output element is the same fp32 MFMA accumulation in ascending m
// inside a split; the split boundaries differ from the register-staged kernel's, so results agree to fp32 summation order, not bit for bit.
#include <stdlib.h>

#include "tn_dma_tile.h"

namespace {

constexpr int TD_BM = 64;                       // rows of m per step
constexpr int TD_IMG = TD_BM * 256;             // one operand image of a step
constexpr int TD_STEP_BYTES = 2 * TD_IMG;       // A image | B image

template <int NBUF>
__global__ __launch_bounds__(512, 2) void gemm_tn_dma_kernel(TnDmaArgs g) {
    constexpr int LA = NBUF - 1;
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2, w4 = wave & 3, wm = w4 >> 1, wn = w4 & 1;
    const TnTile t = tn_tile_of<TD_BM>(g);
    const uint32_t lds_addr = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)lds_raw);

    // ---- staging: an image = 16 pieces; wave w issues pieces 2w, 2w + 1 of A and of B
    uint32_t voffA[2], voffB[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        voffA[q] = tn_piece_src(lane, (wave * 2 + q) * 4, g.lda, t.tn * 128);
        voffB[q] = tn_piece_src(lane, (wave * 2 + q) * 4, g.ldb, t.tk * 128);
    }
    auto stage = [&](int st) __attribute__((always_inline)) {      // step st -> buffer st % NBUF (caller: st < nsteps)
        const int64_t m0 = (int64_t)t.m_beg + (int64_t)st * TD_BM;
        const uint32_t da = lds_addr + (uint32_t)((st % NBUF) * TD_STEP_BYTES + wave * 2048);
        lds_dma16x2(g.A + m0 * g.lda, da, voffA[0], voffA[1]);
        lds_dma16x2(g.B + m0 * g.ldb, da + TD_IMG, voffB[0], voffB[1]);
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // ---- fragments: wave (wm, wn) of group grp multiplies the 32-column blocks wm * 2 + i of A and wn * 2 + j of B over the step's rows 32 grp .. + 31
    uint32_t offA[2], offB[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        offA[i] = lds_addr + tn_tr_off(lane, grp * 32, wm * 2 + i);
        offB[i] = lds_addr + TD_IMG + tn_tr_off(lane, grp * 32, wn * 2 + i);
    }
    // bias gradient: column sums of A by the tk == 0 tiles (thread -> chunk tid % 16 of rows tid / 16 and tid / 16 + 32)
    const bool do_cs = g.colsum != nullptr && t.tk == 0;
    float csum[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) csum[q] = 0.f;

    tn_pipe_fill<LA>(t.nsteps, stage);
    // (r04, measured and dropped: a software pipeline over the steps - the fragments of step s + 1 read from LDS while the MFMAs of step s run
    // from a second fragment register set, 240 VGPRs - ran 8 - 11 % SLOWER on every shape: fc1 94 vs 85 us, qkv 71 vs 64)
    for (int st = 0; st < t.nsteps; ++st) {
        tn_pipe_wait<LA>(st, t.nsteps);
        __builtin_amdgcn_s_barrier();
        if (st + LA < t.nsteps) stage(st + LA);
        const uint32_t bo = (uint32_t)((st % NBUF) * TD_STEP_BYTES);
        u32x2_t fa[2][2][2], fb[2][2][2];            // [kk][32-column block][rows +0..3 | +4..7]
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const uint32_t ro = bo + (uint32_t)((kk * 16 + hh * 4) * 256);
                    lds_read_tr16_b64(fa[kk][i][hh], offA[i] + ro);
                    lds_read_tr16_b64(fb[kk][i][hh], offB[i] + ro);
                }
        if (do_cs) {
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) tn_colsum_add(csum, lds_raw + bo, (tid >> 4) + 32 * h2, tid & 15);
        }
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(fa[0][0][0]), "+v"(fa[0][0][1]), "+v"(fa[0][1][0]), "+v"(fa[0][1][1]), "+v"(fb[0][0][0]), "+v"(fb[0][0][1]), "+v"(fb[0][1][0]), "+v"(fb[0][1][1]),
                       "+v"(fa[1][0][0]), "+v"(fa[1][0][1]), "+v"(fa[1][1][0]), "+v"(fa[1][1][1]), "+v"(fb[1][0][0]), "+v"(fb[1][0][1]), "+v"(fb[1][1][0]), "+v"(fb[1][1][1]));
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8_t af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                af[i] = tr_frag(fa[kk][i][0], fa[kk][i][1]);
                bf[i] = tr_frag(fb[kk][i][0], fb[kk][i][1]);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
        __builtin_amdgcn_s_setprio(0);
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

}  // namespace

// returns P3_OK when the launch was taken, P3_SKIP when the shape / mode is not this kernel's (the caller then runs gemm_tn.hip's kernel)
int p3_gemm_tn_dma_try(const void* A, const void* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, float* colsum, float* slabs, int max_slabs,
                       hipStream_t s) {
    static int on = -1;                              // P3_TN_DMA=0: every weight gradient on gemm_tn.hip's register-staged kernel (A/B: profiles/r04_mb_tn.txt)
    if (on < 0) { const char* e = getenv("P3_TN_DMA"); on = (e && e[0] == '0') ? 0 : 1; }
    if (!on || M % TD_BM != 0 || N % 128 != 0 || K % 128 != 0 || lda % 8 != 0 || ldb % 8 != 0) return P3_SKIP;
    if (((uintptr_t)A % 16) != 0 || ((uintptr_t)B % 16) != 0) return P3_SKIP;
    if ((int64_t)TD_BM * lda * 2 + 256 >= (1ll << 31) || (int64_t)TD_BM * ldb * 2 + 256 >= (1ll << 31)) return P3_SKIP;     // 32-bit DMA offsets inside a step
    TnDmaArgs g = {};
    g.A = (const bf16_t*)A; g.B = (const bf16_t*)B; g.C = C; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.colsum = colsum;
    g.tiles_k = K / 128;
    const int tiles = (N / 128) * g.tiles_k;
    if (tiles > 256) return P3_SKIP;
    const TnSplitPlan plan = tn_split_plan(M, tiles, TD_BM, slabs != nullptr, max_slabs);
    g.splits = plan.splits; g.rows_per_split = plan.rows_per_split;
    const TnParts parts = p3_tn_parts(C, N, K, ldc, plan.splits, slabs, colsum, P3_BF16);
    g.slabs = parts.slabs; g.cs_slab = parts.cs_slab;
    constexpr int NBUF = 4;                          // three steps in flight (NBUF = 3 measured 2 % slower, profiles/r04_mb_tn.txt)
    const size_t lds = (size_t)NBUF * TD_STEP_BYTES;       // >= the 64 KB the fold needs
    const int rc = p3_launch<gemm_tn_dma_kernel<NBUF>>("gemm_tn_dma_kernel<4>", dim3(tiles * plan.splits), dim3(512), lds, s, g);
    if (rc != P3_OK) return rc;
    return p3_tn_parts_reduce(parts, C, N, K, ldc, plan.splits, colsum, s);
}
