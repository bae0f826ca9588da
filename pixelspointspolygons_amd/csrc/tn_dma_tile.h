// The LDS-DMA weight-gradient tile:  C[N,K] += A[M,N]^T B[M,K], split over M.  What gemm_tn_dma.hip (bf16) and gemm_tn_x3.hip (planes, two tiles) share, once:
// the tile / split decode, the operand image in LDS with its swizzle (written by the DMA, read by the transposing reads and the column sums), the step
// pipeline, the fp32x3 product, the bias column sums, the epilogue, and the host's split plan.  A kernel on top of this spells out only its schedule and
// what is its own: how many images a step has, which wave stages which image, and how the waves tile the output.
//
// The operand image: an image is the operand tile AS IT LIES IN MEMORY, [rows of m][128 columns] bf16 = 256-byte rows, unpadded, staged global -> LDS by
// LDS-DMA in 1 KB pieces of 4 rows (no staging registers, no ds_write pass).  The destination of an LDS-DMA is lane-linear, so the swizzle goes onto the
// SOURCE address.  All asm is gfx950_asm.h's; its rules hold here: the DMA base pointer and the LDS destination a kernel hands to lds_dma16x2 must be
// provably wave-uniform (kernel arguments, the readfirstlane'd wave index and LDS base) - nothing below computes either of them.
#pragma once
#include "p3_common.h"

struct TnDmaArgs {
    const bf16_t* A; const bf16_t* Al; const bf16_t* B; const bf16_t* Bl; float* C;       // Al / Bl: the lo planes (unused by the bf16 kernel)
    int M, N, K, lda, ldb, ldc, rows_per_split, tiles_k, splits;
    float* slabs;       // optional [splits][N][K]: partial tiles stored instead of atomics (deterministic mode)
    float* colsum;      // optional [N]: += column sums of A (bias gradient) from the tk == 0 tiles
    float* cs_slab;     // deterministic mode: [splits][N]
    int conv_ci, conv_pw;   // p3_gemm_tn_x3_conv (conv_ci > 0): column tile -> tap t = column / conv_ci, B rows shifted by (t / 3 - 1) * conv_pw + (t % 3 - 1); else 0
};

// B side of a column tile that starts at output column c0: plain product - column c0 of B; 3 x 3 convolution - the tile lies inside ONE tap (the host checks
// conv_ci % tile width == 0): the tap's constant row shift goes onto the scalar base pointer, the column is the channel inside the tap
__device__ __forceinline__ int td_conv_b(const TnDmaArgs& g, int c0, const bf16_t*& src) {
    if (g.conv_ci == 0) return c0;
    const int t = c0 / g.conv_ci;
    src += (int64_t)((t / 3 - 1) * g.conv_pw + (t % 3 - 1)) * g.ldb;
    return c0 - t * g.conv_ci;
}

// ---- workgroup -> (row tile tn, column tile tk, M split) and the split's steps of BM rows -----------------------------------------------------------
// all (n, k) tiles of one M split run on ONE XCD (they read the same rows of A and B).  rows_per_split and M are multiples of BM.
struct TnTile { int tn, tk, split, m_beg, nsteps; };
template <int BM>
__device__ __forceinline__ TnTile tn_tile_of(const TnDmaArgs& g) {
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int tiles_all = gridDim.x / g.splits;
    const int tile = lid % tiles_all, split = lid / tiles_all;
    const int tn = tile / g.tiles_k;
    const int m_beg = split * g.rows_per_split;
    const int m_end = min(g.M, m_beg + g.rows_per_split);
    return {tn, tile - tn * g.tiles_k, split, m_beg, (m_end - m_beg) / BM};
}

// ---- the swizzle, and its three users ----------------------------------------------------------------------------------------------------------------
// A transposing read (ds_read_b64_tr_b16: per 16 lanes, 4 rows x 32 bytes) touches four consecutive rows at ONE column offset; in plain 256-byte rows they
// would share their banks.  So the 16-byte chunk c of row r lies in slot c ^ ((r & 3) << 2) of the row: the 64-byte granule is XORed with r & 3, and the
// four rows of a read lie on four different quarters of the 64 banks.  The XOR is its own inverse: the DMA applies it to the source, the reads to the LDS
// address.  Pieces, fragments and steps start on multiples of 4 rows, so r & 3 is the row inside the piece and never changes with a "+4 rows = +1024 bytes".
__device__ __forceinline__ int tn_swz(int chunk, int row) { return chunk ^ ((row & 3) << 2); }
// DMA source: the byte offset of this lane's 16 bytes of the 1 KB piece (4 rows) whose first row is row0 (% 4 == 0) of the step, from the step's first row of an
// operand of row stride ld (elements) whose tile starts at column col0.  Lane -> (row lane / 16, slot lane % 16) of the piece: it goes to LDS byte 16 * lane.
__device__ __forceinline__ uint32_t tn_piece_src(int lane, int row0, int ld, int col0) {
    const int prow = lane >> 4, slot = lane & 15;
    return (uint32_t)(((int64_t)(row0 + prow) * ld + col0 + tn_swz(slot, prow) * 8) * 2);
}
// transposing read: this lane's byte offset inside an image for the 32-column block `gran` (the row's 64-byte granule) of the 16 rows row0 (% 4 == 0) .. + 15:
// lane -> (row block g4 >> 1, row li >> 2, 32-byte half g4 & 1, 8-byte piece li & 3); a second read 4 rows further (+1024) completes the 8 m of a row block
__device__ __forceinline__ uint32_t tn_tr_off(int lane, int row0, int gran) {
    const int g4 = lane >> 4, li = lane & 15;
    const int lrow = (g4 >> 1) * 8 + (li >> 2), lin = (g4 & 1) * 32 + (li & 3) * 8;
    return (uint32_t)((row0 + lrow) * 256 + tn_swz(gran * 4 + (lin >> 4), lrow) * 16 + (lin & 15));
}
// bias gradient, per step: += the eight columns of chunk `chunk` of row `row` of the A image at `img`
__device__ __forceinline__ void tn_colsum_add(float (&csum)[8], const unsigned char* img, int row, int chunk) {
    const u32x4_t v = *reinterpret_cast<const u32x4_t*>(img + row * 256 + tn_swz(chunk, row) * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) { csum[2 * q] += __uint_as_float(v[q] << 16); csum[2 * q + 1] += __uint_as_float(v[q] & 0xffff0000u); }
}

// ---- the step pipeline: NBUF step buffers in LDS, LA = NBUF - 1 steps in flight, one counted vmcnt and one barrier per step ---------------------------
//     tn_pipe_fill<LA>(nsteps, stage);
//     for (st = 0; st < nsteps; ++st) { tn_pipe_wait<LA>(st, nsteps); s_barrier; if (st + LA < nsteps) stage(st + LA); read buffer st % NBUF; multiply; }
// stage(st) issues this wave's pieces of step st into buffer st % NBUF: TN_DMA_PER_STEP DMA instructions, the same number in every wave and step - the count
// below rests on it.  RAW: this wave's pieces of step st have landed once at most `ahead` younger steps stay in flight (loads retire in order; nothing else
// is outstanding); the barrier extends that to every wave's pieces.  WAR: a wave reaches the barrier of step st after its reads of step st - 1, whose buffer
// step st + LA takes.  A split shorter than LA steps fills less and waits for fewer: ahead = min(LA - 1, steps behind st).  The ladder tests `ahead` from
// the top down on purpose: tested from 0 up, hipcc emits the whole step loop three times (two peeled copies that still carry the full ladder).
constexpr int TN_DMA_PER_STEP = 4;
template <int LA, typename Stage>
__device__ __forceinline__ void tn_pipe_fill(int nsteps, Stage&& stage) {
#pragma unroll
    for (int p = 0; p < LA; ++p)
        if (p < nsteps) stage(p);
}
template <int AHEAD>
__device__ __forceinline__ void tn_wait_ahead(int ahead) {          // at most `ahead` (<= AHEAD) steps still in flight
    if constexpr (AHEAD == 0) wait_vm<0>();
    else if (ahead >= AHEAD) wait_vm<TN_DMA_PER_STEP * AHEAD>();
    else tn_wait_ahead<AHEAD - 1>(ahead);
}
template <int LA>
__device__ __forceinline__ void tn_pipe_wait(int st, int nsteps) { tn_wait_ahead<LA - 1>(min(LA - 1, nsteps - 1 - st)); }

// ---- fp32x3 product of an NI x NJ block of 32 x 32 accumulators over one 16-deep block: a_lo b_hi + a_hi b_lo + a_hi b_hi, small terms first ----------
template <int NI, int NJ>
__device__ __forceinline__ void tn_mma_x3(f32x16 (&acc)[NI][NJ], const bf16x8_t (&ah)[NI], const bf16x8_t (&al)[NI], const bf16x8_t (&bh)[NJ], const bf16x8_t (&bl)[NJ]) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
}

// ---- epilogue (the operand images are dead: `red` is the LDS from its start) --------------------------------------------------------------------------
// bias gradient: threads (row = tid / 16 < ROWS, chunk = tid % 16) hold tn_colsum_add's sums; fold the ROWS row lanes of a column through LDS and commit one
// value per column of the row tile - into the split's cs_slab row, or an fp32 atomic.  Call under a wave-uniform condition; `red` is free after the NEXT barrier.
template <int ROWS>
__device__ __forceinline__ void tn_colsum_fold(const TnDmaArgs& g, const TnTile& t, float* red, const float (&csum)[8], int tid) {
    if (tid < ROWS * 16) {
#pragma unroll
        for (int q = 0; q < 8; ++q) red[tid * 8 + q] = csum[q];          // [row][chunk][q] = [row][128 columns]
    }
    __syncthreads();
    if (tid < 128) {
        float a = 0.f;
        for (int r = 0; r < ROWS; ++r) a += red[r * 128 + tid];
        if (g.cs_slab) g.cs_slab[(int64_t)t.split * g.N + t.tn * 128 + tid] = a;
        else atomicAdd(g.colsum + t.tn * 128 + tid, a);
    }
}
// two groups of four waves hold partial sums of the SAME 2 x 2 accumulator blocks (they multiplied different rows of every step): group KEEP finishes the
// row block i = KEEP of its waves' tiles, out[j] = its own + the other group's, and hands the other row block over through LDS ([group][wave][j][r][lane]
// fp32: conflict-free ds_write_b32 / ds_read_b32).  KEEP is a template parameter: a run-time accumulator index would put acc into scratch.
template <int KEEP>
__device__ __forceinline__ void tn_fold_groups(f32x16 (&out)[2], const f32x16 (&acc)[2][2], float* red, int w4, int lane) {
    float* x = red + (KEEP * 4 + w4) * (2 * 16 * 64);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) x[(j * 16 + r) * 64 + lane] = acc[1 - KEEP][j][r];
    __syncthreads();
    const float* y = red + ((KEEP ^ 1) * 4 + w4) * (2 * 16 * 64);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[j][r] = acc[KEEP][j][r] + y[(j * 16 + r) * 64 + lane];
}
// one 32 x 32 accumulator whose first element is (row0, col0) of the output: the partial tile into the split's slab, or fp32 atomics onto C
__device__ __forceinline__ void tn_commit(const TnDmaArgs& g, int split, int row0, int col0, const f32x16& v, int lane) {
    const int col = col0 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = row0 + crow32(r, lane >> 5);
        if (g.slabs) g.slabs[((int64_t)split * g.N + row) * g.K + col] = v[r];
        else atomicAdd(g.C + (int64_t)row * g.ldc + col, v[r]);
    }
}

// ---- host: the split plan -----------------------------------------------------------------------------------------------------------------------------
// one workgroup per CU and ONE resident round: splits = 256 / tiles (the r03 finding for the register-staged kernel - the best grids fill one resident
// round - holds here by construction); never fewer than two steps of step_rows per split; at most max_slabs splits where the partial tiles go to slabs.
struct TnSplitPlan { int splits, rows_per_split; };
static inline TnSplitPlan tn_split_plan(int M, int tiles, int step_rows, bool slabs, int max_slabs) {
    int splits = 256 / tiles;
    if (splits < 1) splits = 1;
    const int max_splits = M / (2 * step_rows) > 0 ? M / (2 * step_rows) : 1;
    if (splits > max_splits) splits = max_splits;
    if (slabs && splits > max_slabs) splits = max_slabs;
    const int rows_per_split = p3_ceil_div(p3_ceil_div(M, splits), step_rows) * step_rows;
    return {p3_ceil_div(M, rows_per_split), rows_per_split};
}
