// p3hip HiSup polygons (models/hisup/polygon.py:56-169 `ext_c_to_poly_coco`, `inn_c_to_poly_coco`, `diagonal_to_square`, `simple_polygon`,
// `get_poly_crowdai` with test_inria = False): the outer polygon of every region p3_hisup_regions found, from its label map, its bounding box and the
// junctions of its image (p3_hisup_polygons), and with them the inner rings of its holes (p3_hisup_polygons_rings).
//   hp_lds_kernel          one workgroup per (image, label): filled mask, corner grid, border walk, junction match and simplification with all bitmaps and
//                          the ring in LDS, then hole after hole of the region; a region whose padded box or ring does not fit is marked for the second kernel
//   hp_ws_kernel           the same device function over per-workgroup slabs of `workspace` for the marked regions (all of them with force_fallback)
//   hp_offsets_kernel      one workgroup: exclusive scan of the vertex counts in (image, label) order -> poly_slice, n_vertices, counts, status
//   hp_pack_kernel         staged vertices -> pos / src at their final offsets (outer polygons, and once more for the rings)
//   hp_ring_offsets_kernel one workgroup: scan of the regions' ring counts -> region_rings, the staged ring records to (image, label, hole) order, scan of
//                          their vertex counts -> ring_slice, ring_counts, status
// Reproducibility: a region's vertices and ring records are staged wherever an integer atomic hands out room, and are copied to offsets that come from the
// scans alone; the junction vote and the hole seed are integer atomicMin; everything else is a function of the region's own inputs.  Distances and angles
// are float64 without fused multiply-add (the restatements in tests/hisup_polygon_ref.py and tests/hisup_rings_ref.py compute the same roundings).
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
constexpr int HP_AREA2_MIN = 100;      // a hole gives a ring when its border encloses an area of at least 50
constexpr int HP_REC = 6;              // ints of a staged ring record: region, ordinal in the region, vertices, staging base, flags, area2

struct HpArgs {
    const int32_t* labels; const int32_t* n_regions; const int32_t* bbox; const float* juncs; const int32_t* junc_counts;
    int B, H, W, max_regions, max_vertices;
    int stop;                                                    // measurement only (P3_HISUP_POLY_STOP): 1 return before the border walk, 2 right after it
    int32_t* nv; int32_t* stage_base; int32_t* defer;            // per region, in the workspace; defer: 1 the whole region, 2 its holes from r_done on
    unsigned long long* alloc;                                   // staging entries handed out
    float* stage_pos; int32_t* stage_src;
    int32_t* poly_flags; int32_t* hole_pixels; int32_t* status;
    // the inner rings (p3_hisup_polygons_rings only)
    int max_rings, max_ring_vertices;
    int32_t* n_holes;
    int32_t* r_n; int32_t* r_nv; int32_t* r_long; int32_t* r_done;          // per region, in the workspace: kept rings, their vertices, the longest, holes finished
    unsigned long long* r_alloc; unsigned int* r_slots;                    // ring vertices and ring records handed out
    int32_t* r_rec;                                                          // [max_rings][HP_REC]
    float* r_stage_pos; int32_t* r_stage_src;
};

struct HpShared {
    float jx[HP_MAXJ], jy[HP_MAXJ];
    int first[HP_MAXJ], order[HP_MAXJ];
    int red[HP_NT / 64];
    int p0, changed, m, over, base;
    int a2, ymin, ymax, xmin, xmax, start;                       // of the hole in hand: twice its border's area, the border's box, where its ring starts
};

// where a polygon's vertices are staged
struct HpStage { unsigned long long* alloc; int cap; float* pos; int32_t* src; };

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

// the flood of step A, by every thread of the workgroup: cells of value `from` in rows ylo .. yhi and columns xlo .. xhi of the map (row pitch P) become `to`
// when a 4-connected path of such cells joins them to a cell that holds `to`; the cells just outside that range are read, never written.  Row sweeps, column
// sweeps, until nothing changes (the fixed point does not depend on the order).
__device__ void hp_flood(HpShared& sh, uint8_t* map, int P, int ylo, int yhi, int xlo, int xhi, uint8_t from, uint8_t to) {
    const int tid = threadIdx.x;
    for (;;) {
        if (tid == 0) sh.changed = 0;
        __syncthreads();
        bool ch = false;
        for (int y = ylo + tid; y <= yhi; y += HP_NT) {
            uint8_t* row = map + y * P;
            uint8_t prev = row[xlo - 1];
            for (int x = xlo; x <= xhi; ++x) { uint8_t c = row[x]; if (c == from && prev == to) { row[x] = c = to; ch = true; } prev = c; }
            prev = row[xhi + 1];
            for (int x = xhi; x >= xlo; --x) { uint8_t c = row[x]; if (c == from && prev == to) { row[x] = c = to; ch = true; } prev = c; }
        }
        __syncthreads();
        for (int x = xlo + tid; x <= xhi; x += HP_NT) {
            uint8_t* col = map + x;
            uint8_t prev = col[(ylo - 1) * P];
            for (int y = ylo; y <= yhi; ++y) { uint8_t c = col[y * P]; if (c == from && prev == to) { col[y * P] = c = to; ch = true; } prev = c; }
            prev = col[(yhi + 1) * P];
            for (int y = yhi; y >= ylo; --y) { uint8_t c = col[y * P]; if (c == from && prev == to) { col[y * P] = c = to; ch = true; } prev = c; }
        }
        if (ch) sh.changed = 1;
        __syncthreads();
        const bool again = sh.changed != 0;
        __syncthreads();
        if (!again) break;
    }
}

// the border follower of step C, by one lane: over the cells of the map that hold 1, from the set cell p0 with the start direction s0.  emit(p, q, s, last)
// is called for every border cell p with its successor q in direction s (last: this is the closing step) and returns false to give up.  Every neighbour
// of a set cell has to lie inside the map.  -> false: p0 has no neighbour, emit gave up, or more steps than there are (cell, direction) states.
template <typename Emit>
__device__ __forceinline__ bool hp_follow(const uint8_t* map, int P, int cells, int p0, int s0, Emit emit) {
    int s = s0, tries = 0;
    do { s = (s + 7) & 7; } while (map[p0 + hp_dy(s) * P + hp_dx(s)] != 1 && ++tries < 8);
    if (tries >= 8) return false;
    const int p1 = p0 + hp_dy(s) * P + hp_dx(s);
    const int64_t max_steps = 8 * (int64_t)cells;          // (cell, direction) -> successor is one-to-one: no state comes twice
    int p = p0;
    for (int64_t step = 0;; ++step) {
        int q;
        do { s = (s + 1) & 7; q = p + hp_dy(s) * P + hp_dx(s); } while (map[q] != 1);
        const bool last = q == p0 && p == p1;
        if (!emit(p, q, s, last)) return false;
        if (last) return true;
        if (step >= max_steps) return false;
        p = q; s = (s + 4) & 7;
    }
}

// steps E and F, by every thread of the workgroup: the polygon of the ring of m > 0 points of image b, staged through stg.  -> its vertices (the first one
// twice), 0 when nothing is kept; flags gets bit 0 for a junction polygon; base: where it is staged, -1 when the staging area is full
__device__ int hp_polygon(const HpArgs& a, HpShared& sh, const uint32_t* ring, int m, int b, const HpStage& stg, int& flags, int& base) {
    const int tid = threadIdx.x;
    __syncthreads();
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
    base = -1;
    if (kept == 0) return 0;
    const int nv = kept + 1;
    if (tid == 0) {
        const unsigned long long at = atomicAdd(stg.alloc, (unsigned long long)nv);
        const bool fits = at + (unsigned long long)nv <= (unsigned long long)stg.cap;
        sh.base = fits ? (int)at : -1;
    }
    __syncthreads();
    base = sh.base;
    int running = 0;
    for (int v0 = 0; v0 < k; v0 += HP_NT) {
        const int v = v0 + tid;
        const int f = v < k && seq.keep(v, k) ? 1 : 0;
        const int at = wg_excl(f, sh.red, running);
        if (f && base >= 0) {
            float x, y;
            int src;
            if (junc) { src = sh.order[v]; x = sh.jx[src]; y = sh.jy[src]; }
            else { const uint32_t p = ring[v]; src = v; x = (float)(p & 0xffffu); y = (float)(p >> 16); }
            stg.pos[(int64_t)(base + at) * 2] = x; stg.pos[(int64_t)(base + at) * 2 + 1] = y; stg.src[base + at] = src;
            if (at == 0) { stg.pos[(int64_t)(base + kept) * 2] = x; stg.pos[(int64_t)(base + kept) * 2 + 1] = y; stg.src[base + kept] = src;
            }
        }
    }
    return nv;
}

// steps B to F for the outer polygon of region r once step A has filled st.  -> false: the region is finished here (cut short for a measurement, handed
// to the second form, no ring); true: the outer polygon is settled and its holes may follow
template <bool kWs>
__device__ bool hp_outer(const HpArgs& a, HpShared& sh, const uint8_t* st, uint8_t* T, uint32_t* ring, int ring_cap, int b, int64_t r, int y0, int x0, int bh,
                         int bw, int holes) {
    const int tid = threadIdx.x;
    const int P = bw + 3, rows = bh + 3, cells = rows * P;
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
        return false;
    }
    // ---- C + D. border walk of one lane, diagonal steps squared as they are emitted.  Every neighbour of a set cell lies inside the grid (T's rows 0 and
    // bh + 2 and columns 0 and bw + 2 are empty).
    if (tid == 0 && sh.p0 != HP_NONE) {
        int m = 0;
        const bool ok = hp_follow(T, P, cells, sh.p0, 4, [&](int p, int, int s, bool) {
            const int py = p / P, px = p - py * P;
            const int gx = x0 + px - 1, gy = y0 + py - 1;
            if (m < ring_cap) ring[m] = (uint32_t)gx | (uint32_t)gy << 16;
            ++m;
            if (s & 1) {                                     // SE: (x+1, y)  NW: (x-1, y)  NE: (x, y-1)  SW: (x, y+1)
                const int ix = s == 7 ? gx + 1 : (s == 3 ? gx - 1 : gx), iy = s == 1 ? gy - 1 : (s == 5 ? gy + 1 : gy);
                if (m < ring_cap) ring[m] = (uint32_t)ix | (uint32_t)iy << 16;
                ++m;
            }
            return m <= ring_cap;
        });
        sh.m = m; sh.over = ok ? 0 : 1;
    }
    __syncthreads();
    const int m = sh.m;
    int flags = holes > 0 ? 2 : 0;
    if (a.stop == 2) {
        if (tid == 0) { a.nv[r] = 0; a.stage_base[r] = -1; a.poly_flags[r] = flags | 4; a.hole_pixels[r] = holes; }
        return false;
    }
    if (sh.over) {
        if (!kWs) { if (tid == 0) a.defer[r] = 1; return false; }
        if (tid == 0) { atomicOr(a.status, 2); a.nv[r] = 0; a.stage_base[r] = -1; a.poly_flags[r] = flags | 4; a.hole_pixels[r] = holes; }
        return false;
    }
    if (m == 0) {
        if (tid == 0) { a.nv[r] = 0; a.stage_base[r] = -1; a.poly_flags[r] = flags | 4; a.hole_pixels[r] = holes; }
        return false;
    }
    int base;
    const int nv = hp_polygon(a, sh, ring, m, b, HpStage{a.alloc, a.max_vertices, a.stage_pos, a.stage_src}, flags, base);
    if (tid == 0) { a.nv[r] = nv; a.stage_base[r] = base; a.poly_flags[r] = nv > 0 ? flags : flags | 4; a.hole_pixels[r] = holes; }
    return true;
}

// steps G to I, then E and F, for the holes of region r one after another: st holds 1 on the region, 0 on its holes and 2 on everything else; T and the
// ring are free.  A finished hole holds 3.  resume: the second form takes the region over from the first at hole r_done[r] (the holes before it are only
// flooded again).
template <bool kWs>
__device__ void hp_holes(const HpArgs& a, HpShared& sh, uint8_t* st, uint8_t* T, uint32_t* ring, int ring_cap, int b, int64_t r, int y0, int x0, int bh, int bw,
                         bool resume) {
    const int tid = threadIdx.x;
    const int P = bw + 3, cells = (bh + 3) * P;
    const int skip = resume ? a.r_done[r] : 0;
    int n = resume ? a.r_n[r] : 0, nvs = resume ? a.r_nv[r] : 0, longest = resume ? a.r_long[r] : 0;
    int h = 0, from = 0;
    for (;; ++h) {
        // ---- G. the first cell in raster order that is still 0, and its 4-connected component
        __syncthreads();
        if (tid == 0) sh.p0 = HP_NONE;
        __syncthreads();
        for (int i = from + tid; i < cells; i += HP_NT)
            if (st[i] == 0) { atomicMin(&sh.p0, i); break; }
        __syncthreads();
        const int seed = sh.p0;
        if (seed == HP_NONE) break;
        from = seed + 1;
        if (tid == 0) st[seed] = 3;
        // the flood in a window below the seed that grows until no finished cell on its edge has an unfilled neighbour outside it: most holes are a few
        // cells, and a full sweep for each of them would cost the whole box every time.  (A finished cell of an earlier hole never touches an unfilled one.)
        const int sy = seed / P, sx = seed - sy * P;
        for (int k = 8;; k *= 4) {
            const int yhi = min(bh, sy + k), xlo = max(1, sx - k), xhi = min(bw, sx + k);
            hp_flood(sh, st, P, sy, yhi, xlo, xhi, 0, 3);
            if (yhi == bh && xlo == 1 && xhi == bw) break;
            bool more = false;
            for (int x = xlo + tid; x <= xhi; x += HP_NT) more = more || (st[yhi * P + x] == 3 && st[(yhi + 1) * P + x] == 0);
            for (int y = sy + tid; y <= yhi; y += HP_NT)
                more = more || (st[y * P + xlo] == 3 && st[y * P + xlo - 1] == 0) || (st[y * P + xhi] == 3 && st[y * P + xhi + 1] == 0);
            if (more) sh.changed = 1;                        // hp_flood left it 0
            __syncthreads();
            const bool grow = sh.changed != 0;
            __syncthreads();
            if (!grow) break;
        }
        if (h < skip) continue;
        // ---- H. the hole border: the follower on the region's pixels from the pixel left of the seed, s = 0; twice its area and its box.  Its cells are
        // noted in the ring buffer, which is free here, as long as they fit.
        if (tid == 0) {
            long long area = 0;
            int ymin = HP_NONE, ymax = -1, xmin = HP_NONE, xmax = -1, cnt = 0;
            hp_follow(st, P, cells, seed - 1, 0, [&](int p, int q, int, bool) {
                const int py = p / P, px = p - py * P, qy = q / P, qx = q - qy * P;
                area += (long long)px * qy - (long long)qx * py;
                ymin = min(ymin, py); ymax = max(ymax, py); xmin = min(xmin, px); xmax = max(xmax, px);
                if (cnt < ring_cap) ring[cnt] = (uint32_t)p;
                cnt += cnt <= ring_cap;
                return true;
            });
            if (area < 0) area = -area;
            sh.a2 = p3_sat31(area);
            sh.ymin = ymin; sh.ymax = ymax; sh.xmin = xmin; sh.xmax = xmax; sh.m = cnt;
        }
        __syncthreads();
        const int a2 = sh.a2, ymin = sh.ymin, ymax = sh.ymax, xmin = sh.xmin, xmax = sh.xmax, noted = sh.m;
        if (a2 < HP_AREA2_MIN) continue;
        // ---- I. K = the border's cells and what they enclose, in T over the border's box and one cell around it (2 there, the flood of step A inwards)
        const int ew = xmax - xmin + 3, eh = ymax - ymin + 3;              // 1 <= ymin, ymax <= bh and 1 <= xmin, xmax <= bw: the frame lies inside the map
        for (int i = tid; i < eh * ew; i += HP_NT) {
            const int ey = i / ew, ex = i - ey * ew;
            T[(ymin - 1 + ey) * P + (xmin - 1 + ex)] = ey == 0 || ey == eh - 1 || ex == 0 || ex == ew - 1 ? 2 : 0;
        }
        __syncthreads();
        if (noted <= ring_cap) {
            for (int i = tid; i < noted; i += HP_NT) T[ring[i]] = 1;
        } else if (tid == 0) {                               // a border longer than the ring buffer is walked once more
            hp_follow(st, P, cells, seed - 1, 0, [&](int p, int, int, bool) { T[p] = 1; return true; });
        }
        hp_flood(sh, T, P, ymin, ymax, xmin, xmax, 0, 2);
        // K' = K without its first row and its first column; afterwards T is 1 on K' and 0 around it
        if (tid == 0) sh.p0 = HP_NONE;
        __syncthreads();
        for (int i = tid; i < eh * ew; i += HP_NT) {
            const int ey = i / ew, ex = i - ey * ew;
            const int c = (ymin - 1 + ey) * P + (xmin - 1 + ex);
            const bool in = ey >= 2 && ey < eh - 1 && ex >= 2 && ex < ew - 1 && T[c] != 2;
            T[c] = in ? 1 : 0;
            if (in) atomicMin(&sh.p0, c);
        }
        __syncthreads();
        // the outer border of K' (step C as it stands), reversed, then step D on the reversed sequence: the lane writes from the end of the ring downwards, so
        // that reading upwards reverses; what step D inserts after a reversed step q -> p is emitted with p; the insertion of the closing step comes last in
        // the reversed order and has the slot at the very end
        if (tid == 0) {
            int m = 0, w = ring_cap - 2, tail = 0;
            bool ok = sh.p0 != HP_NONE;
            if (ok) ok = hp_follow(T, P, cells, sh.p0, 4, [&](int p, int q, int s, bool last) {
                const int py = p / P, px = p - py * P;
                if (w >= 0) ring[w] = (uint32_t)(x0 + px - 1) | (uint32_t)(y0 + py - 1) << 16;
                --w; ++m;
                if (s & 1) {                                 // the step back from q: NW (s = 7): (x-1, y)  SE (3): (x+1, y)  SW (1): (x, y+1)  NE (5): (x, y-1)
                    const int qy = q / P, qx = q - qy * P;
                    const int gx = x0 + qx - 1, gy = y0 + qy - 1;
                    const int ix = s == 7 ? gx - 1 : (s == 3 ? gx + 1 : gx), iy = s == 1 ? gy + 1 : (s == 5 ? gy - 1 : gy);
                    const int slot = last ? ring_cap - 1 : w--;
                    if (slot >= 0) ring[slot] = (uint32_t)ix | (uint32_t)iy << 16;
                    ++m; tail |= last ? 1 : 0;
                }
                return w >= -1;                              // nothing was dropped
            });
            sh.m = ok ? m : 0; sh.over = ok ? 0 : 1; sh.start = tail ? ring_cap - m : ring_cap - 1 - m;
        }
        __syncthreads();
        if (sh.over) {
            if (!kWs) {                                      // the ring does not fit in LDS: the second form goes on from this hole
                if (tid == 0) { a.defer[r] = 2; a.r_done[r] = h; a.r_n[r] = n; a.r_nv[r] = nvs; a.r_long[r] = longest; }
                return;
            }
            if (tid == 0) atomicOr(a.status, 2);
        }
        int flags = 0, base = -1, nv = 0;
        if (!sh.over && sh.m > 0) nv = hp_polygon(a, sh, ring + sh.start, sh.m, b, HpStage{a.r_alloc, a.max_ring_vertices, a.r_stage_pos, a.r_stage_src}, flags, base);
        if (tid == 0) {
            const unsigned int slot = atomicAdd(a.r_slots, 1u);
            if (slot < (unsigned int)a.max_rings) {
                int32_t* rec = a.r_rec + (int64_t)slot * HP_REC;
                rec[0] = (int32_t)r; rec[1] = n; rec[2] = nv; rec[3] = base; rec[4] = nv > 0 ? flags : flags | 4; rec[5] = a2;
            }
        }
        ++n; nvs += nv; longest = max(longest, nv);
    }
    if (tid == 0) { a.n_holes[r] = h; a.r_n[r] = n; a.r_nv[r] = nvs; a.r_long[r] = longest; }
}

// one region (image b, label l, clamped box): every thread of the workgroup calls it.  st / T: bitmaps of (bh + 3) x (bw + 3) bytes, ring: ring_cap points;
// LDS or global memory.  kWs: the second form (a ring past ring_cap is an error there, in the first form the region is handed on); mode: 1 the whole region,
// 2 (second form, rings) the outer polygon is settled and the holes go on where the first form stopped.  kRings: the holes follow the outer polygon.
template <bool kWs, bool kRings>
__device__ void hp_region(const HpArgs& a, HpShared& sh, uint8_t* st, uint8_t* T, uint32_t* ring, int ring_cap, int b, int l, int y0, int x0, int bh, int bw, int mode) {
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
        hp_flood(sh, st, P, 1, bh, 1, bw, 0, 2);
        int h = 0;
        for (int i = tid; i < cells; i += HP_NT) h += st[i] == 0;
        wg_scan<false>(h, sh.red, holes);
    }
    const bool resume = kWs && kRings && mode == 2;
    if (!resume && !hp_outer<kWs>(a, sh, st, T, ring, ring_cap, b, r, y0, x0, bh, bw, holes)) return;
    if (kRings && holes > 0) hp_holes<kWs>(a, sh, st, T, ring, ring_cap, b, r, y0, x0, bh, bw, resume);
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

template <bool kRings>
__global__ __launch_bounds__(HP_NT) void hp_lds_kernel(HpArgs a, int force_fallback) {
    __shared__ HpShared sh;
    __shared__ uint8_t st[HP_BOX_LDS], T[HP_BOX_LDS];
    __shared__ uint32_t ring[HP_RING_LDS];
    const int64_t r = blockIdx.x;
    if (kRings && threadIdx.x == 0) { a.n_holes[r] = 0; a.r_n[r] = 0; a.r_nv[r] = 0; a.r_long[r] = 0; a.r_done[r] = 0; }
    int b, l, y0, x0, bh, bw;
    if (!hp_box(a, r, b, l, y0, x0, bh, bw)) {
        if (threadIdx.x == 0) { a.nv[r] = 0; a.stage_base[r] = -1; a.defer[r] = 0; a.poly_flags[r] = 0; a.hole_pixels[r] = 0; }
        return;
    }
    const bool later = force_fallback != 0 || (int64_t)(bh + 3) * (bw + 3) > HP_BOX_LDS;
    if (threadIdx.x == 0) { a.defer[r] = later ? 1 : 0; if (later) { a.nv[r] = 0; a.stage_base[r] = -1; } }
    if (later) return;
    hp_region<false, kRings>(a, sh, st, T, ring, HP_RING_LDS, b, l, y0, x0, bh, bw, 1);
}

template <bool kRings>
__global__ __launch_bounds__(HP_NT) void hp_ws_kernel(HpArgs a, uint8_t* slabs, int64_t slab_bytes, int64_t map_bytes, int ring_cap) {
    __shared__ HpShared sh;
    uint8_t* st = slabs + blockIdx.x * slab_bytes;
    uint8_t* T = st + map_bytes;
    uint32_t* ring = (uint32_t*)(T + map_bytes);
    const int64_t R = (int64_t)a.B * a.max_regions;
    for (int64_t r = blockIdx.x; r < R; r += gridDim.x) {
        const int mode = a.defer[r];
        if (!mode) continue;
        int b, l, y0, x0, bh, bw;
        if (!hp_box(a, r, b, l, y0, x0, bh, bw)) continue;
        hp_region<true, kRings>(a, sh, st, T, ring, ring_cap, b, l, y0, x0, bh, bw, mode);
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
        const long long lo = wg_excl((long long)v, red, running);
        if (i < R) { poly_slice[i * 2] = lo; poly_slice[i * 2 + 1] = lo + v; }
        longest = max(longest, v);
    }
    const int lm = wg_max(longest, redm);
    __syncthreads();
    for (int b = tid; b < B; b += 1024)
        n_vertices[b] = (int32_t)(poly_slice[((int64_t)b * max_regions + max_regions - 1) * 2 + 1] - poly_slice[(int64_t)b * max_regions * 2]);
    if (tid == 0) {
        counts[0] = p3_sat31(running);
        counts[1] = lm;
        if (running > max_vertices) atomicOr(status, 1);
        if (stop != 0) atomicOr(status, 4);                  // a run cut short for a measurement never passes for a result
    }
}

// one workgroup.  The regions' ring counts -> region_rings and the totals; with room for every ring: the staged records -> ring_region, ring_flags,
// ring_area2 and (fin_nv, fin_base) at region_rings[region] + ordinal, then the scan of fin_nv -> ring_slice
__global__ __launch_bounds__(1024) void hp_ring_offsets_kernel(const int32_t* __restrict__ r_n, const int32_t* __restrict__ r_nv, const int32_t* __restrict__ r_long,
                                                               const int32_t* __restrict__ rec, int64_t R, int max_rings, int max_ring_vertices,
                                                               int32_t* __restrict__ region_rings, int64_t* __restrict__ ring_slice, int32_t* __restrict__ ring_region,
                                                               int32_t* __restrict__ ring_flags, int32_t* __restrict__ ring_area2, int32_t* __restrict__ fin_nv,
                                                               int32_t* __restrict__ fin_base, int32_t* __restrict__ ring_counts, int32_t* __restrict__ status) {
    __shared__ long long red[16];
    __shared__ int redm[16];
    const int tid = threadIdx.x;
    long long rings = 0, verts = 0;
    int longest = 0;
    for (int64_t i0 = 0; i0 < R; i0 += 1024) {
        const int64_t i = i0 + tid;
        const int v = i < R ? r_n[i] : 0;
        const long long lo = wg_excl((long long)v, red, rings);
        if (i < R) { region_rings[i * 2] = p3_sat31(lo); region_rings[i * 2 + 1] = p3_sat31(lo + v); }
        __syncthreads();
        wg_excl((long long)(i < R ? r_nv[i] : 0), red, verts);          // the total alone
        longest = max(longest, i < R ? r_long[i] : 0);
        __syncthreads();
    }
    const int lm = wg_max(longest, redm);
    if (tid == 0) {
        ring_counts[0] = p3_sat31(rings);
        ring_counts[1] = p3_sat31(verts);
        ring_counts[2] = lm;
        if (rings > max_rings) atomicOr(status, 8);
        if (verts > max_ring_vertices) atomicOr(status, 16);
    }
    __syncthreads();
    if (rings > max_rings) return;                           // some records were never staged: no ring is written
    const int Q = (int)rings;
    for (int s = tid; s < Q; s += 1024) {
        const int32_t* c = rec + (int64_t)s * HP_REC;
        const int q = region_rings[(int64_t)c[0] * 2] + c[1];
        ring_region[q] = c[0]; fin_nv[q] = c[2]; fin_base[q] = c[3]; ring_flags[q] = c[4]; ring_area2[q] = c[5];
    }
    __threadfence();
    __syncthreads();
    long long running = 0;
    for (int i0 = 0; i0 < Q; i0 += 1024) {
        const int i = i0 + tid;
        const int v = i < Q ? fin_nv[i] : 0;
        const long long lo = wg_excl((long long)v, red, running);
        if (i < Q) { ring_slice[(int64_t)i * 2] = lo; ring_slice[(int64_t)i * 2 + 1] = lo + v; }
        __syncthreads();
    }
}

// one wave per polygon; nothing is copied when a capacity was too small (status & mask: the staging area then holds only some of the polygons)
__global__ __launch_bounds__(HP_NT) void hp_pack_kernel(const int32_t* __restrict__ nv, const int32_t* __restrict__ stage_base, const int64_t* __restrict__ poly_slice,
                                                        const float* __restrict__ stage_pos, const int32_t* __restrict__ stage_src, const int32_t* __restrict__ status,
                                                        int mask, const int32_t* __restrict__ count, int64_t R, int max_vertices, float* __restrict__ pos,
                                                        int32_t* __restrict__ src) {
    const int64_t r = (int64_t)blockIdx.x * (HP_NT / 64) + (threadIdx.x >> 6);
    if (r >= R || (status[0] & mask) || (count && r >= count[0])) return;
    const int n = nv[r], sb = stage_base[r];
    const int64_t o = poly_slice[r * 2];
    if (n <= 0 || sb < 0 || o + n > max_vertices) return;
    for (int i = threadIdx.x & 63; i < n; i += 64) {
        pos[(o + i) * 2] = stage_pos[(int64_t)(sb + i) * 2];
        pos[(o + i) * 2 + 1] = stage_pos[(int64_t)(sb + i) * 2 + 1];
        src[o + i] = stage_src[sb + i];
    }
}

struct HpWs {
    unsigned long long* counters;                        // 256 bytes: staging entries handed out - vertices [0], ring vertices [1] - and ring records (a uint at byte 16)
    int32_t *nv, *stage_base, *defer;
    float* stage_pos; int32_t* stage_src;
    int32_t *r_n, *r_nv, *r_long, *r_done, *r_rec, *fin_nv, *fin_base;                 // with rings only
    float* r_stage_pos; int32_t* r_stage_src;
    uint8_t* slabs;
    int64_t slab_bytes, map_bytes;
    int n_slabs, ring_cap;
};

// max_rings == 0: the workspace of p3_hisup_polygons
HpWs hp_carve(int B, int H, int W, int max_regions, int max_vertices, int max_rings, int max_ring_vertices, P3Carve& c) {
    HpWs L = {};
    const int64_t R = (int64_t)B * max_regions;
    L.counters = (unsigned long long*)c.take_bytes(256);
    L.nv = c.take<int32_t>(R);
    L.stage_base = c.take<int32_t>(R);
    L.defer = c.take<int32_t>(R);
    L.stage_pos = c.take<float>(2 * (int64_t)max_vertices);
    L.stage_src = c.take<int32_t>(max_vertices);
    if (max_rings > 0) {
        L.r_n = c.take<int32_t>(R);
        L.r_nv = c.take<int32_t>(R);
        L.r_long = c.take<int32_t>(R);
        L.r_done = c.take<int32_t>(R);
        L.r_rec = c.take<int32_t>((int64_t)max_rings * HP_REC);
        L.fin_nv = c.take<int32_t>(max_rings);
        L.fin_base = c.take<int32_t>(max_rings);
        L.r_stage_pos = c.take<float>(2 * (int64_t)max_ring_vertices);
        L.r_stage_src = c.take<int32_t>(max_ring_vertices);
    }
    L.map_bytes = p3_up256((int64_t)(H + 3) * (W + 3));
    L.ring_cap = (int)(2 * ((int64_t)H * (W + 1) + (int64_t)W * (H + 1)) + 8);        // the ring bound of the header; an inner ring stays below it
    L.slab_bytes = 2 * L.map_bytes + p3_up256((int64_t)L.ring_cap * 4);
    const int64_t fit = ((int64_t)1 << 30) / L.slab_bytes;                          // at most 1 GiB of slabs
    L.n_slabs = (int)(R < HP_SLABS ? R : HP_SLABS);
    if (L.n_slabs > fit) L.n_slabs = fit < 1 ? 1 : (int)fit;
    if (L.n_slabs < 1) L.n_slabs = 1;
    L.slabs = (uint8_t*)c.take_bytes(L.n_slabs * L.slab_bytes);
    return L;
}
int64_t hp_bytes(int B, int H, int W, int max_regions, int max_vertices, int max_rings, int max_ring_vertices) {
    P3Carve c = {nullptr, 0};
    hp_carve(B, H, W, max_regions, max_vertices, max_rings, max_ring_vertices, c);
    return c.at;
}

struct HpRingOut {
    float* ring_pos; int32_t* ring_src; int64_t* ring_slice; int32_t* ring_region; int32_t* ring_flags; int32_t* ring_area2; int32_t* region_rings;
    int32_t* n_holes; int32_t* ring_counts;
};

// both entries: ro == nullptr is p3_hisup_polygons
template <bool kRings>
int hp_run(const int32_t* labels, const int32_t* n_regions, const int32_t* bbox, const float* juncs, const int32_t* junc_counts, int B, int H, int W,
           int max_regions, int max_vertices, int max_rings, int max_ring_vertices, int force_fallback, float* pos, int32_t* src, int64_t* poly_slice,
           int32_t* poly_flags, int32_t* hole_pixels, int32_t* n_vertices, int32_t* counts, int32_t* status, const HpRingOut* ro, void* workspace, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    P3Carve carve = {(char*)workspace, 0};
    const HpWs L = hp_carve(B, H, W, max_regions, max_vertices, max_rings, max_ring_vertices, carve);
    P3_TRY(p3_memset(L.counters, 0, 256, s));
    P3_TRY(p3_memset(status, 0, 4, s));
    HpArgs a = {};
    a.labels = labels; a.n_regions = n_regions; a.bbox = bbox; a.juncs = juncs; a.junc_counts = junc_counts;
    a.B = B; a.H = H; a.W = W; a.max_regions = max_regions; a.max_vertices = max_vertices;
    const char* stop = getenv("P3_HISUP_POLY_STOP");            // tools/bench_hisup_polygons.py: the share of the single-lane walk
    a.stop = stop && (stop[0] == '1' || stop[0] == '2') && stop[1] == 0 ? stop[0] - '0' : 0;          // "1" and "2" only: anything else is a full run
    a.nv = L.nv; a.stage_base = L.stage_base; a.defer = L.defer;
    a.alloc = L.counters;
    a.stage_pos = L.stage_pos; a.stage_src = L.stage_src;
    a.poly_flags = poly_flags; a.hole_pixels = hole_pixels; a.status = status;
    if (kRings) {
        a.max_rings = max_rings; a.max_ring_vertices = max_ring_vertices; a.n_holes = ro->n_holes;
        a.r_n = L.r_n; a.r_nv = L.r_nv; a.r_long = L.r_long; a.r_done = L.r_done;
        a.r_alloc = L.counters + 1; a.r_slots = (unsigned int*)(L.counters + 2);
        a.r_rec = L.r_rec; a.r_stage_pos = L.r_stage_pos; a.r_stage_src = L.r_stage_src;
    }
    const int64_t R = (int64_t)B * max_regions;
    P3_TRY(p3_launch<hp_lds_kernel<kRings>>(kRings ? "hisup_polygons_rings_lds" : "hisup_polygons_lds", (unsigned)R, HP_NT, 0, s, a, force_fallback));
    P3_TRY(p3_launch<hp_ws_kernel<kRings>>(kRings ? "hisup_polygons_rings_ws" : "hisup_polygons_ws", L.n_slabs, HP_NT, 0, s, a, L.slabs, L.slab_bytes, L.map_bytes,
                                           L.ring_cap));
    P3_TRY(p3_launch<hp_offsets_kernel>(nullptr, 1, 1024, 0, s, a.nv, B, max_regions, max_vertices, a.stop, poly_slice, n_vertices, counts, status));
    const int32_t* every = nullptr;
    P3_TRY(p3_launch<hp_pack_kernel>(nullptr, p3_ceil_div(R, HP_NT / 64), HP_NT, 0, s, a.nv, a.stage_base, poly_slice, a.stage_pos, a.stage_src, status, 1, every, R,
                                     max_vertices, pos, src));
    if (!kRings) return P3_OK;
    P3_TRY(p3_launch<hp_ring_offsets_kernel>(nullptr, 1, 1024, 0, s, a.r_n, a.r_nv, a.r_long, a.r_rec, R, max_rings, max_ring_vertices, ro->region_rings, ro->ring_slice,
                                             ro->ring_region, ro->ring_flags, ro->ring_area2, L.fin_nv, L.fin_base, ro->ring_counts, status));
    return p3_launch<hp_pack_kernel>(nullptr, p3_ceil_div(max_rings, HP_NT / 64), HP_NT, 0, s, L.fin_nv, L.fin_base, ro->ring_slice, a.r_stage_pos, a.r_stage_src, status,
                                     8 | 16, ro->ring_counts, (int64_t)max_rings, max_ring_vertices, ro->ring_pos, ro->ring_src);
}

}  // namespace

extern "C" int64_t p3_hisup_polygons_workspace_bytes(int B, int H, int W, int max_regions, int max_vertices) {
    if (B <= 0 || H <= 0 || W <= 0 || max_regions <= 0 || max_vertices <= 0) return 0;
    return hp_bytes(B, H, W, max_regions, max_vertices, 0, 0);
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
    return hp_run<false>(labels, n_regions, bbox, juncs, junc_counts, B, H, W, max_regions, max_vertices, 0, 0, force_fallback, pos, src, poly_slice, poly_flags,
                         hole_pixels, n_vertices, counts, status, nullptr, workspace, stream);
}

extern "C" int64_t p3_hisup_polygons_rings_workspace_bytes(int B, int H, int W, int max_regions, int max_vertices, int max_rings, int max_ring_vertices) {
    if (B <= 0 || H <= 0 || W <= 0 || max_regions <= 0 || max_vertices <= 0 || max_rings <= 0 || max_ring_vertices <= 0) return 0;
    return hp_bytes(B, H, W, max_regions, max_vertices, max_rings, max_ring_vertices);
}

extern "C" int p3_hisup_polygons_rings(const int32_t* labels, const int32_t* n_regions, const int32_t* bbox, const float* juncs, const int32_t* junc_counts,
                                       int B, int H, int W, int max_regions, int max_vertices, int max_rings, int max_ring_vertices, int force_fallback,
                                       float* pos, int32_t* src, int64_t* poly_slice, int32_t* poly_flags, int32_t* hole_pixels, int32_t* n_vertices,
                                       int32_t* counts, float* ring_pos, int32_t* ring_src, int64_t* ring_slice, int32_t* ring_region, int32_t* ring_flags,
                                       int32_t* ring_area2, int32_t* region_rings, int32_t* n_holes, int32_t* ring_counts, int32_t* status, void* workspace,
                                       void* stream) {
    P3_CHECK(B >= 0 && max_regions >= 0, P3_ESHAPE, "p3_hisup_polygons_rings: negative B or max_regions");
    if (B == 0 || max_regions == 0) return P3_OK;
    P3_CHECK(labels && n_regions && bbox && juncs && junc_counts && pos && src && poly_slice && poly_flags && hole_pixels && n_vertices && counts && ring_pos &&
                 ring_src && ring_slice && ring_region && ring_flags && ring_area2 && region_rings && n_holes && ring_counts && status && workspace, P3_EINVAL,
             "p3_hisup_polygons_rings: null pointer");
    P3_CHECK(H > 0 && W > 0 && H <= HP_MAX_EDGE && W <= HP_MAX_EDGE && (int64_t)H * W <= ((int64_t)1 << 22) && max_vertices > 0 && max_rings > 0 &&
                 max_ring_vertices > 0 && (int64_t)B * max_regions < ((int64_t)1 << 31), P3_ESHAPE,
             "p3_hisup_polygons_rings: bad sizes (H, W <= 32766, H * W <= 2^22, max_vertices, max_rings, max_ring_vertices > 0)");
    const HpRingOut ro = {ring_pos, ring_src, ring_slice, ring_region, ring_flags, ring_area2, region_rings, n_holes, ring_counts};
    return hp_run<true>(labels, n_regions, bbox, juncs, junc_counts, B, H, W, max_regions, max_vertices, max_rings, max_ring_vertices, force_fallback, pos, src,
                        poly_slice, poly_flags, hole_pixels, n_vertices, counts, status, &ro, workspace, stream);
}
