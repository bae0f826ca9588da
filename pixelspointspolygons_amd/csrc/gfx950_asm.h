// gfx950 inline-asm primitives of the dense kernels: every asm statement that more than one source file uses lives here, once.  Included by p3_common.h.
//
// hipcc treats an asm statement as ONE opaque instruction: it allocates the operands, and neither counts the memory operations inside nor pads their hazards
// (cdna_hip_programming.md, section 5.7 "Inline asm in a HIP kernel: what hipcc does not do").  A mistake here gives wrong values on some waves of some
// launches, with no fault and no message.  The rules for everything below:
//   * m0 is the LDS-DMA destination base.  It is compiler-reserved and not preserved around a statement: it is saved, written and restored inside the SAME
//     statement that reads it (`keep`), never across two.
//   * a statement that steps m0 with s_add_u32 overwrites SCC and says so ("scc" in its clobber list): hipcc keeps a scalar compare alive across an asm
//     statement that does not (the conv-tap state of gemm_x3.hip - a compare, the DMA statements, then the s_cselect - read the s_add's carry instead).
//   * `s_nop 0` stands between every write of m0 and the DMA instruction that reads it; hipcc pads nothing inside the string, so wait states belong in it.
//   * "s" operands (the base pointer, the LDS destination) must be provably wave-uniform: a kernel argument, a blockIdx expression, or a
//     __builtin_amdgcn_readfirstlane.  The per-lane part of the source address is the "v" byte offset.
//   * hipcc counts none of this.  An LDS-DMA writes 64 lanes x 16 bytes to [lds_dst, lds_dst + 1 KB) in lane order and is outstanding on the VM counter:
//     the data is readable only after the issuing wave's own wait_vm<N>() (N = the DMA instructions that may stay in flight), THEN a barrier, THEN the read.
//     __syncthreads() does not stand in for the wait.
//   * the transposing read has two forms.  lds_read_tr16_b64 (asm) where the wait is placed by hand: the kernel follows a group of reads with its own
//     `s_waitcnt lgkmcnt(0)` statement that names every destination "+v".  __builtin_amdgcn_ds_read_tr16_b64_v4i16 (attn_tile.h, pair_dw_x3.hip) where the
//     compiler's counter should track the read.
// A new kernel calls these; it does not paste the string.  tests/test_asm_header_cpu.py holds the list of what may stay outside this file.
//
// Deliberately left in the kernel files:
//   * statements used in one place: the sc1 stores, the v_xor / v_mbcnt and the one-dword DMA of gemm_x3_as.hip, the s_memtime probe;
//   * the empty `asm volatile("" : "+v"(...))` register barriers;
//   * the `s_waitcnt lgkmcnt(0)` statements that carry a "+v" operand list: the list is the point of each of them and differs per site.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- LDS-DMA: global -> LDS, 16 bytes per lane, no VGPR destination ------------------------------------------------------------------------------
// one 1 KB piece: lane l's 16 bytes at base + voff go to lds_dst + 16 l
__device__ __forceinline__ void lds_dma16(const void* base, uint32_t lds_dst, uint32_t voff) {
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep) : "v"(voff), "s"(base), "s"(lds_dst) : "memory");
}
// two pieces from one base, consecutive in LDS: the second at lds_dst + 0x400
__device__ __forceinline__ void lds_dma16x2(const void* base, uint32_t lds_dst, uint32_t v0, uint32_t v1) {
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %4\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\t"
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %3\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep) : "v"(v0), "v"(v1), "s"(base), "s"(lds_dst) : "memory", "scc");
}
// one piece from base_a to dst_a, then three consecutive pieces from base_b starting at dst_b (the 128 x 384 tile of gemm_dma.hip: A panel | W panel)
__device__ __forceinline__ void lds_dma16x1p3(const void* base_a, uint32_t dst_a, uint32_t va, const void* base_b, uint32_t dst_b, uint32_t v0, uint32_t v1,
                                              uint32_t v2) {
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %7\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %5\n\t"
        "s_mov_b32 m0, %8\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %6\n\t"
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %6\n\t"
        "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, %6\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep) : "v"(va), "v"(v0), "v"(v1), "v"(v2), "s"(base_a), "s"(base_b), "s"(dst_a), "s"(dst_b) : "memory", "scc");
}

// ---- waits ---------------------------------------------------------------------------------------------------------------------------------------
// at most N of this wave's vector-memory operations (LDS-DMA pieces included) still outstanding; they retire in issue order
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// the same, and this wave's LDS reads done (before the barrier that hands a buffer back to the DMA)
template <int N> __device__ __forceinline__ void wait_vm_lgkm0() { asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// workgroup barrier that waits for this wave's LDS traffic only: global loads (LDS-DMA included) stay in flight across it, unlike __syncthreads()
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// vmcnt(0) through the builtin (0x0F70: vmcnt = 0, every other counter at its maximum).  pair_dw_x3.hip and pair_bwd_x3.hip issue ordinary global loads
// (the V rows), which the compiler counts, AHEAD of their DMA pieces, which it does not.  An asm wait is invisible to its counter model: it would keep the
// V loads pending and place a wait of its own at their first use, inside the next step's products - a wait that retires in order and so also drains the DMA
// pieces queued behind them.  The builtin is a wait the compiler sees: behind it its model knows the V loads are complete.  Put it on EVERY path.
__device__ __forceinline__ void wait_vm0_tracked() { __builtin_amdgcn_s_waitcnt(0x0F70); }

// ---- transposing LDS read (asm form; see the note at the top) --------------------------------------------------------------------------------------
// ds_read_b64_tr_b16: per 16 lanes, 4 rows x 32 bytes; lanes 4j..4j+3 point at row j's 16 elements and lane i receives column i of those 4 rows.
// dst is NOT valid until the caller's lgkmcnt wait that names it.
template <typename V2> __device__ __forceinline__ void lds_read_tr16_b64(V2& dst, uint32_t lds_addr) {
    static_assert(sizeof(V2) == 8, "two dwords per lane");
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(dst) : "v"(lds_addr));
}
