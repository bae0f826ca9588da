// p3hip — what the ring-set scoring stages share (poly_metrics.hip: p3_polygon_metrics; coco_metrics.hip: p3_coco_metrics; mta_metrics.hip: p3_max_tangent_angle; mask_metrics.hip: p3_mask_metrics): the ring set, the ring
// validity routine with its workspace record, the rings of an image by binary search, the even-odd crossing rule at pixel centres and the filled union mask of a set (pm_raster_set).  DESIGN.md section 21
// holds the definition.  Every floating-point value is a double made of the fp32 coordinates; contraction is off from here on, so that a product and the sum
// behind it round as the float64 restatements round them.
#pragma once
#include "p3_common.h"

#pragma clang fp contract(off)

constexpr int PM_THREADS = 256;
constexpr int PM_EDGE_CHUNK = 32;          // edges of a ring staged through LDS at a time (raster: their end points; pair: their sample counts, prefix-summed)
constexpr double PM_MAX_COORD = 32768.0;   // a ring with a coordinate beyond it is invalid: per-edge sample counts stay far inside int32
constexpr int64_t PM_MAX_HW = (int64_t)1 << 18;

struct PmSet {
    const float2* pos;
    const int64_t* slice;
    const int32_t* image;
    int64_t V;
    int R;
};
// per ring of one set (workspace): state 1 valid, 0 invalid (counted per image), -1 left out; n vertices from `first`; box = (min x, min y, w, h)
struct PmRings {
    int32_t* state;
    int32_t* n;
    int64_t* first;
    double* box;          // [R, 4]
};

__device__ __forceinline__ double pm_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
// first index whose image is >= b: ring_image is non-decreasing, so the rings of image b are [pm_lower(b), pm_lower(b + 1))
__device__ __forceinline__ int pm_lower(const int32_t* image, int R, int b) {
    int lo = 0, hi = R;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (image[mid] < b) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- rings ----------------------------------------------------------------------------------------------------------------------------------------------
__device__ inline void pm_ring(const PmSet& s, const PmRings& w, int r, int B, int32_t* status) {
    const int64_t a = s.slice[2 * r], e = s.slice[2 * r + 1];
    const int img = s.image[r];
    w.first[r] = 0;
    w.n[r] = 0;
    for (int k = 0; k < 4; ++k) w.box[4 * (int64_t)r + k] = 0.0;
    if (img < 0 || img >= B || a < 0 || e < a || e > s.V || e - a >= ((int64_t)1 << 30)) {
        w.state[r] = -1;
        atomicOr(status, 2);
        return;
    }
    const int n = (int)(e - a);
    bool ok = n >= 3;
    double x0 = 0, x1 = 0, y0 = 0, y1 = 0;
    for (int i = 0; i < n && ok; ++i) {
        const float2 p = s.pos[a + i];
        const double x = (double)p.x, y = (double)p.y;
        if (!(fabs(x) <= PM_MAX_COORD && fabs(y) <= PM_MAX_COORD)) ok = false;          // NaN and the infinities fail the comparison too
        if (i == 0) { x0 = x1 = x; y0 = y1 = y; }
        x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1;
        y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
    }
    if (!ok) {
        w.state[r] = 0;
        atomicOr(status, 1);
        return;
    }
    w.state[r] = 1;
    w.n[r] = n;
    w.first[r] = a;
    double* box = w.box + 4 * (int64_t)r;
    box[0] = x0; box[1] = y0; box[2] = x1 - x0; box[3] = y1 - y0;
}

// ---- the crossing rule ----------------------------------------------------------------------------------------------------------------------------------
struct PmEdge { double ax, ay, bx, by; };

// the rows and columns whose pixel centres can lie inside a ring of this box, clipped to the H x W image (clamped in double before the conversion); false: none
__device__ __forceinline__ bool pm_pixel_box(const double* box, int H, int W, int& r0, int& r1, int& c0, int& c1) {
    const double fr0 = floor(box[1] - 0.5), fr1 = ceil(box[1] + box[3] - 0.5), fc0 = floor(box[0] - 0.5), fc1 = ceil(box[0] + box[2] - 0.5);
    if (fr1 < 0.0 || fc1 < 0.0 || fr0 > (double)(H - 1) || fc0 > (double)(W - 1)) return false;
    r0 = (int)fmax(fr0, 0.0); r1 = (int)fmin(fr1, (double)(H - 1)); c0 = (int)fmax(fc0, 0.0); c1 = (int)fmin(fc1, (double)(W - 1));
    return true;
}
// the centres of row py cross the edge
__device__ __forceinline__ bool pm_crossed(const PmEdge& ed, double py) { return (ed.ay <= py) != (ed.by <= py); }
// the crossing of an edge that row py crosses lies to the right of the centre (px, py); t1 = (b.x - a.x)(py - a.y) and ey = b.y - a.y, once per edge and row
__device__ __forceinline__ bool pm_right_of(const PmEdge& ed, double t1, double ey, double px) {
    const double cr = t1 - (px - ed.ax) * ey;
    return ey > 0.0 ? cr > 0.0 : cr < 0.0;
}
// edges e0 .. e0 + cnt of a ring into LDS, one per thread (the caller puts the barriers around it)
__device__ __forceinline__ void pm_stage_edges(const float2* pos, int64_t first, int n, int e0, int cnt, PmEdge* edges) {
    const int tid = threadIdx.x;
    if (tid < cnt) {
        const int i = e0 + tid, j = i + 1 == n ? 0 : i + 1;
        const float2 pa = pos[first + i], pb = pos[first + j];
        edges[tid] = {(double)pa.x, (double)pa.y, (double)pb.x, (double)pb.y};
    }
}

// ---- the filled mask of a set ---------------------------------------------------------------------------------------------------------------------------
// the rings of one set of image b into `mask` (bit r W + c of the packed words): the parity of each valid ring, ORed in.  Every thread of a workgroup of
// PM_THREADS calls it; `edges`: PM_EDGE_CHUNK of them in LDS; the caller clears the mask before and puts a barrier behind the call
__device__ inline void pm_raster_set(const PmSet& s, const PmRings& w, int b, int H, int W, uint32_t* mask, PmEdge* edges) {
    const int tid = threadIdx.x;
    const int r_lo = pm_lower(s.image, s.R, b), r_hi = pm_lower(s.image, s.R, b + 1);
    for (int r = r_lo; r < r_hi; ++r) {
        if (w.state[r] != 1) continue;          // uniform over the workgroup
        const int n = w.n[r];
        const int64_t first = w.first[r];
        int r0, r1, c0, c1;          // rows and columns whose centres can lie inside
        if (!pm_pixel_box(w.box + 4 * (int64_t)r, H, W, r0, r1, c0, c1)) continue;
        const int per_row = ((c1 - c0) >> 5) + 2;          // words a row's [c0, c1] can touch
        const int units = (r1 - r0 + 1) * per_row;
        for (int base = 0; base < units; base += PM_THREADS) {
            const int u = base + tid;
            const int row = r0 + u / per_row;
            const int bit0 = row * W + c0, bit1 = row * W + c1;          // H W <= 2^18: no overflow
            const int word = (bit0 >> 5) + u % per_row;
            const bool active = u < units && word <= (bit1 >> 5);
            const int lo = bit0 > (word << 5) ? bit0 : (word << 5), hi = bit1 < (word << 5) + 31 ? bit1 : (word << 5) + 31;
            const double py = (double)row + 0.5;
            uint32_t parity = 0;
            for (int e0 = 0; e0 < n; e0 += PM_EDGE_CHUNK) {
                const int cnt = n - e0 < PM_EDGE_CHUNK ? n - e0 : PM_EDGE_CHUNK;
                __syncthreads();          // the last chunk has been read
                pm_stage_edges(s.pos, first, n, e0, cnt, edges);
                __syncthreads();
                if (!active) continue;
                for (int k = 0; k < cnt; ++k) {
                    const PmEdge ed = edges[k];
                    if (!pm_crossed(ed, py)) continue;          // not crossed by this row's centres
                    const double ex = ed.bx - ed.ax, ey = ed.by - ed.ay, wy = py - ed.ay;
                    const double t1 = ex * wy;
                    for (int bit = lo; bit <= hi; ++bit) {
                        const double px = (double)(bit - row * W) + 0.5;
                        if (pm_right_of(ed, t1, ey, px)) parity ^= 1u << (bit & 31);
                    }
                }
            }
            if (active && parity) atomicOr(mask + word, parity);
        }
    }
}

// ---- host: the ring records in a workspace ----------------------------------------------------------------------------------------------------------------
static inline PmRings pm_carve_set(int R, P3Carve& c) {
    PmRings w;
    w.state = c.take<int32_t>(R);
    w.n = c.take<int32_t>(R);
    w.first = c.take<int64_t>(R);
    w.box = c.take<double>(4 * (int64_t)R);
    return w;
}
