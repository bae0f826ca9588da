// p3hip HiSup polygons (models/hisup/polygon.py:56-93,111-169 `ext_c_to_poly_coco`, `diagonal_to_square`, `simple_polygon`, `get_poly_crowdai` with
// test_inria = False): the outer polygon of every region p3_hisup_regions found, from its label map, its bounding box and the junctions of its image.
//   hp_lds_kernel      one workgroup per (image, label): filled mask, corner grid, border walk, junction match and simplification with all bitmaps and
//                      the ring in LDS; a region whose padded box or ring does not fit is marked for the second kernel
//   hp_ws_kernel       the same device function over per-workgroup slabs of `workspace` for the marked regions (all of them with force_fallback)
//   hp_offsets_kernel  one workgroup: exclusive scan of the vertex counts in (image, label) order -> poly_slice, n_vertices, counts, status
//   hp_pack_kernel     staged vertices -> pos / src at their final offsets
// Reproducibility: a region's vertices are staged wherever an integer atomic hands out room, and are copied to offsets that come from the scan alone;
// the junction vote is an integer atomicMin; everything else is a function of the region's own inputs.  Distances and angles are float64 without fused
// multiply-add (the restatement in tests/hisup_polygon_ref.py computes the same roundings).
#include <stdlib.h>

#include "p3_common.h"

namespace {

constexpr int HP_NT = 256;
constexpr int HP_MAXJ = 600;           // 2 x top-300 of p3_hisup_junctions
constexpr int HP_BOX_LDS = 16384;      // cells of the padded box (h + 3) x (w + 3) that run in LDS: one byte each in two bitmaps
constexpr int HP_RING_LDS = 5120;      // ring points in LDS (packed x | y << 16)
constexpr int HP_SLABS = 64;           // workgroups (and workspace slabs) of the second form
constexpr int HP_NONE = 0x7fffffff;
constexpr int HP_MAX_EDGE = 32766;     // ring coordinates are packed into 16 bits each

struct HpArgs {
    const int32_t* labels; const int32_t* n_regions; const int32_t* bbox; const float* juncs; const int32_t* junc_counts;
    int B, H, W, max_regions, max_vertices;
    int stop;                                                    // measurement only (P3_HISUP_POLY_STOP): 1 return before the border walk, 2 right after it
    int32_t* nv; int32_t* stage_base; int32_t* defer;            // per region, in the workspace
    unsigned long long* alloc;                                   // staging entries handed out
    float* stage_pos; int32_t* stage_src;
    int32_t* poly_flags; int32_t* hole_pixels; int32_t* status;
};

struct HpShared {
    float jx[HP_MAXJ], jy[HP_MAXJ];
    int first[HP_MAXJ], order[HP_MAXJ];
    int red[HP_NT / 64];
    int p0, changed, m, over, base;
};

// direction s: 0 E, 1 NE, 2 N, 3 NW, 4 W, 5 SW, 6 S, 7 SE (y grows downwards); dx + 1 and dy + 1 as 2-bit fields
constexpr uint32_t HP_DX = 2u | 2u << 2 | 1u << 4 | 0u << 6 | 0u << 8 | 0u << 10 | 1u << 12 | 2u << 14;
constexpr uint32_t HP_DY = 1u | 0u << 2 | 0u << 4 | 0u << 6 | 1u << 8 | 2u << 10 | 2u << 12 | 2u << 14;
__device__ __forceinline__ int hp_dx(int s) { return (int)((HP_DX >> (2 * s)) & 3u) - 1; }
__device__ __forceinline__ int hp_dy(int s) { return (int)((HP_DY >> (2 * s)) & 3u) - 1; }

__device__ __forceinline__ double hp_dist2(double px, double py, float jx, float jy) {
#pragma clang fp contract(off)
    const double dx = px - (double)jx, dy = py - (double)jy;
    const double xx = dx * dx, yy = dy * dy;
    return xx + yy;
}

__device__ __forceinline__ double hp_angle(double ey, double ex) {
#pragma clang fp contract(off)
    return atan2(ey, ex) * 180.0 / 3.14159265358979323846;
}

// the sequence that is simplified: the ring (integer corner coordinates) or the matched junctions in the order of their first ring point
struct HpSeq {
    const uint32_t* ring; const HpShared* sh; bool junc;
    __device__ __forceinline__ void at(int i, double& x, double& y) const {
        if (junc) { const int j = sh->order[i]; x = (double)sh->jx[j]; y = (double)sh->jy[j]; }
        else { const uint32_t p = ring[i]; x = (double)(p & 0xffffu); y = (double)(p >> 16); }
    }
    __device__ __forceinline__ bool keep(int v, int k) const {
#pragma clang fp contract(off)
        double x0, y0, x1, y1, x2, y2;
        at(v == 0 ? k - 1 : v - 1, x0, y0); at(v, x1, y1); at(v + 1 == k ? 0 : v + 1, x2, y2);
        const double t = fabs(hp_angle(y1 - y0, x1 - x0) - hp_angle(y2 - y1, x2 - x1));
        return t > 10.0 && t < 350.0;
    }
};

// one region (image b, label l, clamped box): every thread of the workgroup calls it.  st / T: bitmaps of (bh + 3) x (bw + 3) bytes, ring: ring_cap points;
// LDS or global memory.  kWs: the second form (a ring past ring_cap is an error there, in the first form the region is handed on).
template <bool kWs>
__device__ void hp_region(const HpArgs& a, HpShared& sh, uint8_t* st, uint8_t* T, uint32_t* ring, int ring_cap, int b, int l, int y0, int x0, int bh, int bw) {
    const int tid = threadIdx.x;
    const int P = bw + 3, rows = bh + 3, cells = rows * P;
    const int64_t r = (int64_t)b * a.max_regions + (l - 1);
    const int32_t* lab = a.labels + (int64_t)b * a.H * a.W;
    if (tid == 0) { sh.p0 = HP_NONE; sh.m = 0; sh.over = 0; sh.base = 0; }
    // ---- A. region pixels 1, background 0, outside the box 2; the 2 spreads over 4-connected background; what stays 0 is a hole
    int zeros = 0;
    for (int i = tid; i < cells; i += HP_NT) {
        const int ly = i / P, lx = i - ly * P;
        uint8_t v = 2;
        if (ly >= 1 && ly <= bh && lx >= 1 && lx <= bw) {
            v = lab[(int64_t)(y0 + ly - 1) * a.W + (x0 + lx - 1)] == l ? 1 : 0;
            zeros += v == 0;
        }
        st[i] = v;
    }
    int total;
    wg_scan<false>(zeros, sh.red, total);
    int holes = 0;
    if (total > 0) {
        for (;;) {                                       // row sweeps, column sweeps, until nothing changes (the fixed point does not depend on the order)
            if (tid == 0) sh.changed = 0;
            __syncthreads();
            bool ch = false;
            for (int rr = tid; rr < bh; rr += HP_NT) {
                uint8_t* row = st + (rr + 1) * P;
                uint8_t prev = 2;
                for (int x = 1; x <= bw; ++x) { uint8_t c = row[x]; if (c == 0 && prev == 2) { row[x] = c = 2; ch = true; } prev = c; }
                prev = 2;
                for (int x = bw; x >= 1; --x) { uint8_t c = row[x]; if (c == 0 && prev == 2) { row[x] = c = 2; ch = true; } prev = c; }
            }
            __syncthreads();
            for (int cc = tid; cc < bw; cc += HP_NT) {
                uint8_t* col = st + cc + 1;
                uint8_t prev = 2;
                for (int y = 1; y <= bh; ++y) { uint8_t c = col[y * P]; if (c == 0 && prev == 2) { col[y * P] = c = 2; ch = true; } prev = c; }
                prev = 2;
                for (int y = bh; y >= 1; --y) { uint8_t c = col[y * P]; if (c == 0 && prev == 2) { col[y * P] = c = 2; ch = true; } prev = c; }
            }
            if (ch) sh.changed = 1;
            __syncthreads();
            const bool again = sh.changed != 0;
            __syncthreads();
            if (!again) break;
        }
        int h = 0;
        for (int i = tid; i < cells; i += HP_NT) h += st[i] == 0;
        wg_scan<false>(h, sh.red, holes);
    }
    // ---- B. corner grid: T(y, x) = F(y, x) | F(y-1, x) | F(y, x-1) | F(y-1, x-1) in the same local frame; its first set cell in raster order
    for (int i = tid; i < cells; i += HP_NT) {
        const int ly = i / P, lx = i - ly * P;
        bool t = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int yy = ly - (k >> 1), xx = lx - (k & 1);
            t = t || (yy >= 1 && yy <= bh && xx >= 1 && xx <= bw && st[yy * P + xx] != 2);
        }
        T[i] = t ? 1 : 0;
        if (t) atomicMin(&sh.p0, i);
    }
    __syncthreads();
    if (a.stop == 1) {
        if (tid == 0) { a.nv[r] = 0; a.stage_base[r] = -1; a.poly_flags[r] = 4; a.hole_pixels[r] = holes; }
        return;
    }
    // ---- C + D. border walk of one lane, diagonal steps squared as they are emitted.  Every neighbour of a set cell lies inside the grid (T's rows 0 and
    // bh + 2 and columns 0 and bw + 2 are empty).
    if (tid == 0 && sh.p0 != HP_NONE) {
        const int p0 = sh.p0;
        int s = 4, tries = 0;
        do { s = (s + 7) & 7; } while (!T[p0 + hp_dy(s) * P + hp_dx(s)] && ++tries < 8);
        int m = 0;
        bool over = tries >= 8;
        if (!over) {
            const int p1 = p0 + hp_dy(s) * P + hp_dx(s);
            const int64_t max_steps = 8 * (int64_t)cells;          // (cell, direction) -> successor is one-to-one: no state comes twice
            int p = p0;
            for (int64_t step = 0;; ++step) {
                int q;
                do { s = (s + 1) & 7; q = p + hp_dy(s) * P + hp_dx(s); } while (!T[q]);
                const int py = p / P, px = p - py * P;
                const int gx = x0 + px - 1, gy = y0 + py - 1;
                if (m < ring_cap) ring[m] = (uint32_t)gx | (uint32_t)gy << 16;
                ++m;
                if (s & 1) {                                     // SE: (x+1, y)  NW: (x-1, y)  NE: (x, y-1)  SW: (x, y+1)
                    const int ix = s == 7 ? gx + 1 : (s == 3 ? gx - 1 : gx), iy = s == 1 ? gy - 1 : (s == 5 ? gy + 1 : gy);
                    if (m < ring_cap) ring[m] = (uint32_t)ix | (uint32_t)iy << 16;
                    ++m;
                }
                if (q == p0 && p == p1) break;
                if (step >= max_steps || m > ring_cap) { over = true; break; }
                p = q; s = (s + 4) & 7;
            }
        }
        sh.m = m; sh.over = over || m > ring_cap ? 1 : 0;
    }
    __syncthreads();
    const int m = sh.m;
    int flags = holes > 0 ? 2 : 0;
    if (a.stop == 2) {
        if (tid == 0) { a.nv[r] = 0; a.stage_base[r] = -1; a.poly_flags[r] = flags | 4; a.hole_pixels[r] = holes; }
        return;
    }
    if (sh.over) {
        if (!kWs) { if (tid == 0) a.defer[r] = 1; return; }
        if (tid == 0) { atomicOr(a.status, 2); a.nv[r] = 0; a.stage_base[r] = -1; a.poly_flags[r] = flags | 4; a.hole_pixels[r] = holes; }
        return;
    }
    if (m == 0) {
        if (tid == 0) { a.nv[r] = 0; a.stage_base[r] = -1; a.poly_flags[r] = flags | 4; a.hole_pixels[r] = holes; }
        return;
    }
    // ---- E. every ring point votes for its nearest junction when that is closer than 5
    const int64_t nj64 = (int64_t)max(a.junc_counts[b * 2], 0) + (int64_t)max(a.junc_counts[b * 2 + 1], 0);
    const int nj = (int)(nj64 < HP_MAXJ ? nj64 : HP_MAXJ);
    for (int j = tid; j < nj; j += HP_NT) {
        sh.jx[j] = a.juncs[((int64_t)b * HP_MAXJ + j) * 2];
        sh.jy[j] = a.juncs[((int64_t)b * HP_MAXJ + j) * 2 + 1];
        sh.first[j] = HP_NONE;
    }
    __syncthreads();
    int voted = 0;
    if (nj > 0) {
        for (int i = tid; i < m; i += HP_NT) {
            const uint32_t p = ring[i];
            const double px = (double)(p & 0xffffu), py = (double)(p >> 16);
            double bs = hp_dist2(px, py, sh.jx[0], sh.jy[0]);
            int bj = 0;
            for (int j = 1; j < nj; ++j) {
                const double s = hp_dist2(px, py, sh.jx[j], sh.jy[j]);
                // the root is monotonic: s >= bs cannot give a smaller distance, s below bs by more than a few ulps must; in between the roots decide
                // (equal roots keep the lower index)
                if (s < bs && (s * 1.0000000000000018 < bs || sqrt(s) < sqrt(bs))) { bs = s; bj = j; }
            }
            if (sqrt(bs) < 5.0) atomicMin(&sh.first[bj], i);
        }
        __syncthreads();
        int v = 0;
        for (int j = tid; j < nj; j += HP_NT) v += sh.first[j] != HP_NONE;
        wg_scan<false>(v, sh.red, voted);
    }
    const bool junc = voted > 2;
    if (junc) {
        flags |= 1;
        for (int j = tid; j < nj; j += HP_NT) {
            const int f = sh.first[j];
            if (f == HP_NONE) continue;
            int rank = 0;
            for (int k = 0; k < nj; ++k) rank += sh.first[k] < f;
            sh.order[rank] = j;
        }
        __syncthreads();
    }
    // ---- F. vertices at which the direction turns by more than 10 degrees, in ascending index, the first one once more at the end
    const int k = junc ? voted : m;
    const HpSeq seq{ring, &sh, junc};
    int mine = 0;
    for (int v = tid; v < k; v += HP_NT) mine += seq.keep(v, k);
    int kept;
    wg_scan<false>(mine, sh.red, kept);
    if (kept == 0) {
        if (tid == 0) { a.nv[r] = 0; a.stage_base[r] = -1; a.poly_flags[r] = flags | 4; a.hole_pixels[r] = holes; }
        return;
    }
    const int nv = kept + 1;
    if (tid == 0) {
        const unsigned long long at = atomicAdd(a.alloc, (unsigned long long)nv);
        const bool fits = at + (unsigned long long)nv <= (unsigned long long)a.max_vertices;
        sh.base = fits ? (int)at : -1;
        a.nv[r] = nv; a.stage_base[r] = sh.base; a.poly_flags[r] = flags; a.hole_pixels[r] = holes;
    }
    __syncthreads();
    const int base = sh.base;
    int running = 0;
    for (int v0 = 0; v0 < k; v0 += HP_NT) {
        const int v = v0 + tid;
        const int f = v < k && seq.keep(v, k) ? 1 : 0;
        int tot;
        const int at = running + wg_scan<false>(f, sh.red, tot) - f;
        if (f && base >= 0) {
            float x, y;
            int src;
            if (junc) { src = sh.order[v]; x = sh.jx[src]; y = sh.jy[src]; }
            else { const uint32_t p = ring[v]; src = v; x = (float)(p & 0xffffu); y = (float)(p >> 16); }
            a.stage_pos[(int64_t)(base + at) * 2] = x; a.stage_pos[(int64_t)(base + at) * 2 + 1] = y; a.stage_src[base + at] = src;
            if (at == 0) { a.stage_pos[(int64_t)(base + kept) * 2] = x; a.stage_pos[(int64_t)(base + kept) * 2 + 1] = y; a.stage_src[base + kept] = src; }
        }
        running += tot;
    }
}

// the region of workgroup slot r: false when the label is past the image's regions; the box clamped into the image
__device__ __forceinline__ bool hp_box(const HpArgs& a, int64_t r, int& b, int& l, int& y0, int& x0, int& bh, int& bw) {
    b = (int)(r / a.max_regions); l = (int)(r % a.max_regions) + 1;
    if (l > min(max(a.n_regions[b], 0), a.max_regions)) return false;
    const int32_t* bx = a.bbox + r * 4;
    y0 = min(max(bx[0], 0), a.H - 1); x0 = min(max(bx[1], 0), a.W - 1);
    bh = min(max(bx[2], y0 + 1), a.H) - y0; bw = min(max(bx[3], x0 + 1), a.W) - x0;
    return true;
}

__global__ __launch_bounds__(HP_NT) void hp_lds_kernel(HpArgs a, int force_fallback) {
    __shared__ HpShared sh;
    __shared__ uint8_t st[HP_BOX_LDS], T[HP_BOX_LDS];
    __shared__ uint32_t ring[HP_RING_LDS];
    const int64_t r = blockIdx.x;
    int b, l, y0, x0, bh, bw;
    if (!hp_box(a, r, b, l, y0, x0, bh, bw)) {
        if (threadIdx.x == 0) { a.nv[r] = 0; a.stage_base[r] = -1; a.defer[r] = 0; a.poly_flags[r] = 0; a.hole_pixels[r] = 0; }
        return;
    }
    const bool later = force_fallback != 0 || (int64_t)(bh + 3) * (bw + 3) > HP_BOX_LDS;
    if (threadIdx.x == 0) { a.defer[r] = later ? 1 : 0; if (later) { a.nv[r] = 0; a.stage_base[r] = -1; } }
    if (later) return;
    hp_region<false>(a, sh, st, T, ring, HP_RING_LDS, b, l, y0, x0, bh, bw);
}

__global__ __launch_bounds__(HP_NT) void hp_ws_kernel(HpArgs a, uint8_t* slabs, int64_t slab_bytes, int64_t map_bytes, int ring_cap) {
    __shared__ HpShared sh;
    uint8_t* st = slabs + blockIdx.x * slab_bytes;
    uint8_t* T = st + map_bytes;
    uint32_t* ring = (uint32_t*)(T + map_bytes);
    const int64_t R = (int64_t)a.B * a.max_regions;
    for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
        if (!a.defer[r]) continue;
        int b, l, y0, x0, bh, bw;
        if (!hp_box(a, r, b, l, y0, x0, bh, bw)) continue;
        hp_region<true>(a, sh, st, T, ring, ring_cap, b, l, y0, x0, bh, bw);
        __syncthreads();
    }
}

__global__ __launch_bounds__(1024) void hp_offsets_kernel(const int32_t* __restrict__ nv, int B, int max_regions, int max_vertices, int stop, int64_t* __restrict__ poly_slice,
                                                          int32_t* __restrict__ n_vertices, int32_t* __restrict__ counts, int32_t* __restrict__ status) {
    __shared__ long long red[16];
    __shared__ int redm[16];
    const int tid = threadIdx.x;
    const int64_t R = (int64_t)B * max_regions;
    long long running = 0;
    int longest = 0;
    for (int64_t i0 = 0; i0 < R; i0 += 1024) {
        const int64_t i = i0 + tid;
        const int v = i < R ? nv[i] : 0;
        long long tot;
        const long long incl = wg_scan<false>((long long)v, red, tot);
        if (i < R) { poly_slice[i * 2] = running + incl - v; poly_slice[i * 2 + 1] = running + incl; }
        running += tot;
        longest = max(longest, v);
    }
    int lm;
    wg_scan<true>(longest, redm, lm);
    __syncthreads();
    for (int b = tid; b < B; b += 1024)
        n_vertices[b] = (int32_t)(poly_slice[((int64_t)b * max_regions + max_regions - 1) * 2 + 1] - poly_slice[(int64_t)b * max_regions * 2]);
    if (tid == 0) {
        counts[0] = (int32_t)(running < 0x7fffffffLL ? running : 0x7fffffffLL);
        counts[1] = lm;
        if (running > max_vertices) atomicOr(status, 1);
        if (stop != 0) atomicOr(status, 4);                  // a run cut short for a measurement never passes for a result
    }
}

// one wave per region; nothing is copied when the capacity was too small (the staging area then holds only some of the regions)
__global__ __launch_bounds__(HP_NT) void hp_pack_kernel(const int32_t* __restrict__ nv, const int32_t* __restrict__ stage_base, const int64_t* __restrict__ poly_slice,
                                                        const float* __restrict__ stage_pos, const int32_t* __restrict__ stage_src, const int32_t* __restrict__ status,
                                                        int64_t R, int max_vertices, float* __restrict__ pos, int32_t* __restrict__ src) {
    const int64_t r = (int64_t)blockIdx.x * (HP_NT / 64) + (threadIdx.x >> 6);
    if (r >= R || (status[0] & 1)) return;
    const int n = nv[r], sb = stage_base[r];
    const int64_t o = poly_slice[r * 2];
    if (n <= 0 || sb < 0 || o + n > max_vertices) return;
    for (int i = threadIdx.x & 63; i < n; i += 64) {
        pos[(o + i) * 2] = stage_pos[(int64_t)(sb + i) * 2];
        pos[(o + i) * 2 + 1] = stage_pos[(int64_t)(sb + i) * 2 + 1];
        src[o + i] = stage_src[sb + i];
    }
}

struct HpLayout { int64_t nv, stage_base, defer, stage_pos, stage_src, slabs, total, slab_bytes, map_bytes; int n_slabs, ring_cap; };

HpLayout hp_layout(int B, int H, int W, int max_regions, int max_vertices) {
    HpLayout L;
    const int64_t R = (int64_t)B * max_regions;
    int64_t o = 256;                                     // the staging counter
    L.nv = o; o += p3_up256(R * 4);
    L.stage_base = o; o += p3_up256(R * 4);
    L.defer = o; o += p3_up256(R * 4);
    L.stage_pos = o; o += p3_up256((int64_t)max_vertices * 8);
    L.stage_src = o; o += p3_up256((int64_t)max_vertices * 4);
    L.map_bytes = p3_up256((int64_t)(H + 3) * (W + 3));
    L.ring_cap = (int)(2 * ((int64_t)H * (W + 1) + (int64_t)W * (H + 1)) + 8);        // the ring bound of the header
    L.slab_bytes = 2 * L.map_bytes + p3_up256((int64_t)L.ring_cap * 4);
    const int64_t fit = ((int64_t)1 << 30) / L.slab_bytes;                          // at most 1 GiB of slabs
    L.n_slabs = (int)(R < HP_SLABS ? R : HP_SLABS);
    if (L.n_slabs > fit) L.n_slabs = fit < 1 ? 1 : (int)fit;
    if (L.n_slabs < 1) L.n_slabs = 1;
    L.slabs = o; o += L.n_slabs * L.slab_bytes;
    L.total = o;
    return L;
}

}  // namespace

extern "C" int64_t p3_hisup_polygons_workspace_bytes(int B, int H, int W, int max_regions, int max_vertices) {
    if (B <= 0 || H <= 0 || W <= 0 || max_regions <= 0 || max_vertices <= 0) return 0;
    return hp_layout(B, H, W, max_regions, max_vertices).total;
}

extern "C" int p3_hisup_polygons(const int32_t* labels, const int32_t* n_regions, const int32_t* bbox, const float* juncs, const int32_t* junc_counts, int B,
                                 int H, int W, int max_regions, int max_vertices, int force_fallback, float* pos, int32_t* src, int64_t* poly_slice,
                                 int32_t* poly_flags, int32_t* hole_pixels, int32_t* n_vertices, int32_t* counts, int32_t* status, void* workspace,
                                 void* stream) {
    P3_CHECK(B >= 0 && max_regions >= 0, P3_ESHAPE, "p3_hisup_polygons: negative B or max_regions");
    if (B == 0 || max_regions == 0) return P3_OK;
    P3_CHECK(labels && n_regions && bbox && juncs && junc_counts && pos && src && poly_slice && poly_flags && hole_pixels && n_vertices && counts && status &&
                 workspace, P3_EINVAL, "p3_hisup_polygons: null pointer");
    P3_CHECK(H > 0 && W > 0 && H <= HP_MAX_EDGE && W <= HP_MAX_EDGE && (int64_t)H * W <= ((int64_t)1 << 22) && max_vertices > 0 &&
                 (int64_t)B * max_regions < ((int64_t)1 << 31), P3_ESHAPE, "p3_hisup_polygons: bad sizes (H, W <= 32766, H * W <= 2^22, max_vertices > 0)");
    hipStream_t s = (hipStream_t)stream;
    const HpLayout L = hp_layout(B, H, W, max_regions, max_vertices);
    uint8_t* ws = (uint8_t*)workspace;
    hipError_t e = hipMemsetAsync(ws, 0, 256, s);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, 4, s);
    if (e != hipSuccess) { p3_set_error(hipGetErrorString(e)); return (int)e; }
    HpArgs a;
    a.labels = labels; a.n_regions = n_regions; a.bbox = bbox; a.juncs = juncs; a.junc_counts = junc_counts;
    a.B = B; a.H = H; a.W = W; a.max_regions = max_regions; a.max_vertices = max_vertices;
    const char* stop = getenv("P3_HISUP_POLY_STOP");            // tools/bench_hisup_polygons.py: the share of the single-lane walk
    a.stop = stop && (stop[0] == '1' || stop[0] == '2') && stop[1] == 0 ? stop[0] - '0' : 0;          // "1" and "2" only: anything else is a full run
    a.nv = (int32_t*)(ws + L.nv); a.stage_base = (int32_t*)(ws + L.stage_base); a.defer = (int32_t*)(ws + L.defer);
    a.alloc = (unsigned long long*)ws;
    a.stage_pos = (float*)(ws + L.stage_pos); a.stage_src = (int32_t*)(ws + L.stage_src);
    a.poly_flags = poly_flags; a.hole_pixels = hole_pixels; a.status = status;
    const int64_t R = (int64_t)B * max_regions;
    int rc = p3_launch<hp_lds_kernel>("hisup_polygons_lds", dim3((unsigned)R), dim3(HP_NT), 0, s, a, force_fallback);
    if (rc != P3_OK) return rc;
    rc = p3_launch<hp_ws_kernel>("hisup_polygons_ws", dim3(L.n_slabs), dim3(HP_NT), 0, s, a, ws + L.slabs, L.slab_bytes, L.map_bytes, L.ring_cap);
    if (rc != P3_OK) return rc;
    rc = p3_launch<hp_offsets_kernel>(nullptr, dim3(1), dim3(1024), 0, s, (const int32_t*)a.nv, B, max_regions, max_vertices, a.stop, poly_slice, n_vertices, counts, status);
    if (rc != P3_OK) return rc;
    return p3_launch<hp_pack_kernel>(nullptr, dim3(p3_ceil_div(R, HP_NT / 64)), dim3(HP_NT), 0, s, (const int32_t*)a.nv, (const int32_t*)a.stage_base,
                                     (const int64_t*)poly_slice, (const float*)a.stage_pos, (const int32_t*)a.stage_src, (const int32_t*)status, R, max_vertices,
                                     pos, src);
}
