// p3hip — COCO AP / AR of a predicted ring set against a ground-truth ring set (gfx950), for instance masks (`segm`) and for their boundaries
// (`boundary`), from the packed rings to the 2 x 12 stats on the device.  include/p3hip.h (p3_coco_metrics) and DESIGN.md section 22 hold the definition.
//   cm_ring_kernel     one thread per ring of either set: validity, box (pm_rings.h); a prediction whose score is NaN is invalid
//   cm_raster_kernel   one workgroup per ring: its mask bit-packed into its slab of the workspace (bit c & 31 of word c >> 5, row stride ceil(W / 32)), only
//                      the rows and words of its box; area; the boundary by a separable erosion through a second slab; the size-bucket flags; for a prediction
//                      its stable rank among its image's valid predictions by counting, and its slot in the image's list of kept predictions
//   cm_pair_kernel     one wave per (gt ring, kept prediction slot): popcount(a & b) over the intersected rows and words, for the masks and for the boundaries
//   cm_match_kernel    one workgroup per image, one thread per (type, area range, threshold): COCO's greedy walk over the kept predictions
//   cm_order_kernel    one thread per prediction: its stable rank by descending score among the first 1, 10 and 100 kept predictions of all images, by counting
//   cm_series_kernel   one workgroup per (type, area range, maxDets, threshold): tp / fp flags in rank order, integer prefix sums, precision made non-increasing
//                      from the right, recall, the 101 lower-bound searches
//   cm_stats_kernel    one thread per stat: the mean over the entries > -1 in index order
// Integer counts everywhere a count is meant; the quotients are doubles of integers, each operation rounded on its own (contraction is off for the whole file).
#include "pm_rings.h"

#pragma clang fp contract(off)

constexpr int CM_KEEP = 100;               // maxDets[-1]: predictions of an image that take part
constexpr int CM_T = 10, CM_R = 101, CM_A = 4, CM_M = 3;
constexpr int CM_SERIES = 2 * CM_A * CM_M * CM_T;
constexpr int CM_MATCH_THREADS = 128;      // 2 x 4 x 10 = 80 live
constexpr int CM_IOU_LDS = 2048;           // pair IoUs of an image (both types) the match kernel stages in LDS; more are read where the pair kernel left them
constexpr uint8_t CM_SKIP = 0x80;          // flag byte of a ring that is not valid; bits 0..3: outside area range a

static const double cm_iou_thrs[CM_T] = {0.5, 0.55000000000000004, 0.59999999999999998, 0.65000000000000002, 0.69999999999999996,
                                         0.75, 0.80000000000000004, 0.84999999999999998, 0.89999999999999991, 0.94999999999999996};
static const double cm_rec_thrs[CM_R] = {
    0, 0.01, 0.02, 0.029999999999999999, 0.040000000000000001, 0.050000000000000003, 0.059999999999999998, 0.070000000000000007, 0.080000000000000002,
    0.089999999999999997, 0.10000000000000001, 0.11, 0.12, 0.13, 0.14000000000000001, 0.14999999999999999, 0.16, 0.17000000000000001, 0.17999999999999999, 0.19,
    0.20000000000000001, 0.20999999999999999, 0.22, 0.23000000000000001, 0.23999999999999999, 0.25, 0.26000000000000001, 0.27000000000000002,
    0.28000000000000003, 0.28999999999999998, 0.29999999999999999, 0.31, 0.32000000000000001, 0.33000000000000002, 0.34000000000000002, 0.35000000000000003,
    0.35999999999999999, 0.37, 0.38, 0.39000000000000001, 0.40000000000000002, 0.41000000000000003, 0.41999999999999998, 0.42999999999999999, 0.44,
    0.45000000000000001, 0.46000000000000002, 0.47000000000000003, 0.47999999999999998, 0.48999999999999999, 0.5, 0.51000000000000001, 0.52000000000000002,
    0.53000000000000003, 0.54000000000000004, 0.55000000000000004, 0.56000000000000005, 0.57000000000000006, 0.57999999999999996, 0.58999999999999997,
    0.59999999999999998, 0.60999999999999999, 0.62, 0.63, 0.64000000000000001, 0.65000000000000002, 0.66000000000000003, 0.67000000000000004,
    0.68000000000000005, 0.69000000000000006, 0.70000000000000007, 0.70999999999999996, 0.71999999999999997, 0.72999999999999998, 0.73999999999999999, 0.75,
    0.76000000000000001, 0.77000000000000002, 0.78000000000000003, 0.79000000000000004, 0.80000000000000004, 0.81000000000000005, 0.82000000000000006,
    0.83000000000000007, 0.83999999999999997, 0.84999999999999998, 0.85999999999999999, 0.87, 0.88, 0.89000000000000001, 0.90000000000000002,
    0.91000000000000003, 0.92000000000000004, 0.93000000000000005, 0.94000000000000006, 0.95000000000000007, 0.95999999999999996, 0.96999999999999997,
    0.97999999999999998, 0.98999999999999999, 1};
struct CmTables { double iou[CM_T], rec[CM_R]; };          // kernel arguments: no constant-memory upload, no copy to order against the launches

// per ring of one set (workspace), behind the PmRings record
struct CmRings {
    PmRings pm;
    int32_t* ibox;            // [R, 4] = (first row, last row, first word, last word) of the slab region that is written; last row < first row: none
    uint8_t* flags;           // CM_SKIP, or bit a set when the ring's area lies outside area range a
    uint32_t* mask;           // [R, H ceil(W / 32)]
    uint32_t* hmask;          // the horizontally eroded mask (boundary only)
    uint32_t* bmask;          // the boundary (boundary only)
    const float* extra;       // gt: area or null; predictions: score or null
    int32_t* area_px;
    int32_t* boundary_px;
};
struct CmWs {
    CmRings gt, dt;
    int32_t* kept;            // [B, 100]: the prediction at each rank of an image, -1 behind the last
    double* pair_iou;         // [2, 100 R_gt]: row 0 the mask IoU, row 1 min(mask IoU, boundary IoU); 0 where the boxes do not meet
    int32_t* order;           // [3, R_dt]: rank among the first 1 / 10 / 100 kept predictions of all images, -1 when not among them
    uint8_t* flag;            // [CM_SERIES, R_dt] in rank order: 1 tp, 2 fp, 0 ignored
    int32_t* tp;              // [CM_SERIES, R_dt]
    double* pr;               // [CM_SERIES, R_dt]
};
struct CmOut {
    double* stats;
    double* precision;
    double* recall;
    int32_t* dt_rank;
    int32_t* pair_inter;
    int32_t* dt_match;
    uint8_t* dt_ignore;
    int32_t* gt_match;
    int32_t* status;
};

__device__ __forceinline__ float cm_score(const float* score, int d) { return score ? score[d] : 1.0f; }
__device__ __forceinline__ uint8_t cm_area_flags(double area) {
    const double lo[CM_A] = {0.0, 0.0, 1024.0, 9216.0}, hi[CM_A] = {1e10, 1024.0, 9216.0, 1e10};
    uint8_t f = 0;
    for (int a = 0; a < CM_A; ++a) f |= (uint8_t)((area < lo[a] || area > hi[a]) << a);
    return f;
}

// ---- rings ----------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PM_THREADS) void cm_ring_kernel(PmSet gt, PmSet dt, CmRings wg, CmRings wd, int B, int32_t* status) {
    const int r = blockIdx.x * PM_THREADS + threadIdx.x;
    if (r < gt.R) {
        pm_ring(gt, wg.pm, r, B, status);
    } else if (r - gt.R < dt.R) {
        const int d = r - gt.R;
        pm_ring(dt, wd.pm, d, B, status);
        const float s = cm_score(wd.extra, d);
        if (wd.pm.state[d] == 1 && s != s) {          // a NaN score has no place in the order
            wd.pm.state[d] = 0;
            atomicOr(status, 1);
        }
    }
}

// ---- instance masks -------------------------------------------------------------------------------------------------------------------------------------
// word w of row `row` of a slab whose written region is words [w0, w1]: what lies outside it is not in the mask
__device__ __forceinline__ uint32_t cm_word(const uint32_t* slab, int Wd, int row, int w, int w0, int w1) {
    return (w < w0 || w > w1) ? 0u : slab[(int64_t)row * Wd + w];
}
// bit i of the result: pixel (row, 32 w + i + dx)
__device__ __forceinline__ uint32_t cm_shifted(const uint32_t* slab, int Wd, int row, int w, int dx, int w0, int w1) {
    const int q = dx >> 5, rb = dx & 31;          // dx = 32 q + rb with 0 <= rb < 32, also for dx < 0
    const uint32_t lo = cm_word(slab, Wd, row, w + q, w0, w1);
    if (rb == 0) return lo;
    return (lo >> rb) | (cm_word(slab, Wd, row, w + q + 1, w0, w1) << (32 - rb));
}

__global__ __launch_bounds__(PM_THREADS) void cm_raster_kernel(PmSet gt, PmSet dt, CmRings wg, CmRings wd, int H, int W, int dil, int boundary, int32_t* kept,
                                                               CmOut o) {
    __shared__ PmEdge edges[PM_EDGE_CHUNK];
    __shared__ int red[PM_THREADS / 64];
    const int tid = threadIdx.x;
    const bool is_dt = (int)blockIdx.x >= gt.R;
    const int r = is_dt ? blockIdx.x - gt.R : blockIdx.x;
    const PmSet& s = is_dt ? dt : gt;
    const CmRings& w = is_dt ? wd : wg;
    const int Wd = (W + 31) >> 5;
    int32_t* ibox = w.ibox + 4 * (int64_t)r;
    if (w.pm.state[r] != 1) {          // uniform over the workgroup
        if (tid == 0) {
            ibox[0] = 0; ibox[1] = -1; ibox[2] = 0; ibox[3] = -1;
            w.flags[r] = CM_SKIP;
            w.area_px[r] = 0;
            w.boundary_px[r] = 0;
            if (is_dt) o.dt_rank[r] = -1;
        }
        return;
    }
    int r0 = 0, r1 = -1, c0 = 0, c1 = -1;
    const bool any = pm_pixel_box(w.pm.box + 4 * (int64_t)r, H, W, r0, r1, c0, c1);
    if (!any) { r0 = 0; r1 = -1; c0 = 0; c1 = -1; }
    const int w0 = c0 >> 5, w1 = any ? c1 >> 5 : -1;
    const int nw = w1 - w0 + 1;
    const int units = any ? (r1 - r0 + 1) * nw : 0;
    uint32_t* mask = w.mask + (int64_t)r * H * Wd;
    const int n = w.pm.n[r];
    const int64_t first = w.pm.first[r];
    int area = 0;
    for (int base = 0; base < units; base += PM_THREADS) {
        const int u = base + tid;
        const bool active = u < units;
        const int row = r0 + u / nw, word = w0 + u % nw;
        const int lo = c0 > (word << 5) ? c0 : (word << 5), hi = c1 < (word << 5) + 31 ? c1 : (word << 5) + 31;
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
                if (!pm_crossed(ed, py)) continue;
                const double ex = ed.bx - ed.ax, ey = ed.by - ed.ay, wy = py - ed.ay;
                const double t1 = ex * wy;
                for (int c = lo; c <= hi; ++c) {
                    const double px = (double)c + 0.5;
                    if (pm_right_of(ed, t1, ey, px)) parity ^= 1u << (c & 31);
                }
            }
        }
        if (active) {
            mask[(int64_t)row * Wd + word] = parity;
            area += __popc(parity);
        }
    }
    int area_px;
    wg_scan<false, int>(area, red, area_px);          // its barriers also order the mask stores in front of the erosion's loads
    int boundary_px = 0;
    if (boundary && units > 0) {
        uint32_t* hmask = w.hmask + (int64_t)r * H * Wd;
        uint32_t* bmask = w.bmask + (int64_t)r * H * Wd;
        for (int u = tid; u < units; u += PM_THREADS) {          // horizontal: AND of the 2 dil + 1 shifted words, nearest first; 0 ends it
            const int row = r0 + u / nw, word = w0 + u % nw;
            uint32_t h = mask[(int64_t)row * Wd + word];
            for (int dx = 1; dx <= dil && h; ++dx) h &= cm_shifted(mask, Wd, row, word, dx, w0, w1) & cm_shifted(mask, Wd, row, word, -dx, w0, w1);
            hmask[(int64_t)row * Wd + word] = h;
        }
        __syncthreads();
        int cnt = 0;
        for (int u = tid; u < units; u += PM_THREADS) {          // vertical: AND of the 2 dil + 1 rows; a row outside the box holds nothing
            const int row = r0 + u / nw, word = w0 + u % nw;
            uint32_t e = hmask[(int64_t)row * Wd + word];
            for (int dy = 1; dy <= dil && e; ++dy)
                e &= (row - dy < r0 || row + dy > r1) ? 0u : hmask[(int64_t)(row - dy) * Wd + word] & hmask[(int64_t)(row + dy) * Wd + word];
            const uint32_t b = mask[(int64_t)row * Wd + word] & ~e;
            bmask[(int64_t)row * Wd + word] = b;
            cnt += __popc(b);
        }
        wg_scan<false, int>(cnt, red, boundary_px);
    }
    // a prediction's rank among its image's valid predictions: those with a higher score, and the earlier ones of the same score
    int rank = 0;
    if (is_dt) {
        const int b = dt.image[r];
        const int d0 = pm_lower(dt.image, dt.R, b), d1 = pm_lower(dt.image, dt.R, b + 1);
        const float si = cm_score(wd.extra, r);
        int before = 0;
        for (int j = d0 + tid; j < d1; j += PM_THREADS) {
            if (wd.pm.state[j] != 1) continue;
            const float sj = cm_score(wd.extra, j);
            before += sj > si || (sj == si && j < r);
        }
        wg_scan<false, int>(before, red, rank);
    }
    if (tid != 0) return;
    ibox[0] = r0; ibox[1] = r1; ibox[2] = w0; ibox[3] = w1;
    w.area_px[r] = area_px;
    w.boundary_px[r] = boundary_px;
    if (is_dt) {
        w.flags[r] = cm_area_flags((double)area_px);
        o.dt_rank[r] = rank < CM_KEEP ? rank : -1;
        if (rank < CM_KEEP) kept[(int64_t)dt.image[r] * CM_KEEP + rank] = r;
    } else {
        w.flags[r] = cm_area_flags(w.extra ? (double)w.extra[r] : (double)area_px);
    }
}

// ---- pairs ----------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int cm_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double cm_iou(int inter, int a, int b) {
    const int uni = a + b - inter;
    return uni == 0 ? 0.0 : (double)inter / (double)uni;
}

__global__ __launch_bounds__(PM_THREADS) void cm_pair_kernel(PmSet gt, CmRings wg, CmRings wd, int slots, int H, int W, int boundary, const int32_t* kept,
                                                             double* pair_iou, CmOut o) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (PM_THREADS / 64) + (threadIdx.x >> 6);
    if (wave >= (int64_t)gt.R * slots) return;
    const int g = (int)(wave / slots), k = (int)(wave % slots);
    if (wg.pm.state[g] != 1) return;
    const int d = kept[(int64_t)gt.image[g] * CM_KEEP + k];
    if (d < 0) return;
    const int32_t* gb = wg.ibox + 4 * (int64_t)g;
    const int32_t* db = wd.ibox + 4 * (int64_t)d;
    const int r0 = gb[0] > db[0] ? gb[0] : db[0], r1 = gb[1] < db[1] ? gb[1] : db[1];
    const int w0 = gb[2] > db[2] ? gb[2] : db[2], w1 = gb[3] < db[3] ? gb[3] : db[3];
    if (r1 < r0 || w1 < w0) return;          // the boxes do not meet: the 0 of the memsets stays
    const int Wd = (W + 31) >> 5, nw = w1 - w0 + 1, units = (r1 - r0 + 1) * nw;
    const int64_t slab = (int64_t)H * Wd;
    const uint32_t* ma = wg.mask + g * slab;
    const uint32_t* mb = wd.mask + d * slab;
    int im = 0, ib = 0;
    for (int u = lane; u < units; u += 64) {
        const int64_t at = (int64_t)(r0 + u / nw) * Wd + (w0 + u % nw);
        im += __popc(ma[at] & mb[at]);
    }
    im = cm_wave_sum(im);
    if (boundary) {
        const uint32_t* ba = wg.bmask + g * slab;
        const uint32_t* bb = wd.bmask + d * slab;
        for (int u = lane; u < units; u += 64) {
            const int64_t at = (int64_t)(r0 + u / nw) * Wd + (w0 + u % nw);
            ib += __popc(ba[at] & bb[at]);
        }
        ib = cm_wave_sum(ib);
    }
    if (lane != 0) return;
    const int64_t at = (int64_t)CM_KEEP * g + k, row = (int64_t)CM_KEEP * gt.R;
    const double vm = cm_iou(im, wg.area_px[g], wd.area_px[d]);
    o.pair_inter[at] = im;
    pair_iou[at] = vm;
    if (boundary) {
        const double vb = cm_iou(ib, wg.boundary_px[g], wd.boundary_px[d]);
        o.pair_inter[row + at] = ib;
        pair_iou[row + at] = vb < vm ? vb : vm;
    }
}

// ---- matching -------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CM_MATCH_THREADS) void cm_match_kernel(PmSet gt, PmSet dt, CmRings wg, CmRings wd, int types, const int32_t* kept,
                                                                    const double* pair_iou, CmTables tb, CmOut o) {
    __shared__ double staged[CM_IOU_LDS];
    __shared__ int red[CM_MATCH_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int g0 = pm_lower(gt.image, gt.R, b), G = pm_lower(gt.image, gt.R, b + 1) - g0;
    const int32_t* mine = kept + (int64_t)b * CM_KEEP;
    int D;
    wg_scan<false, int>(tid < CM_KEEP && mine[tid] >= 0, red, D);
    if (G == 0 || D == 0) {          // nothing to walk; a prediction without a gt ring is still ignored by its own area
        if (tid < 2 * CM_A * CM_T && (types >> (tid / (CM_A * CM_T)) & 1)) {
            const int a = tid / CM_T % CM_A;
            for (int k = 0; k < D; ++k) o.dt_ignore[(int64_t)tid * dt.R + mine[k]] = wd.flags[mine[k]] >> a & 1;
        }
        return;
    }
    // the IoUs of the image: [type][gt ring][slot], in LDS when they fit
    const double* iou = pair_iou + (int64_t)CM_KEEP * g0;
    int64_t type_stride = (int64_t)CM_KEEP * gt.R;
    int ring_stride = CM_KEEP;
    if ((int64_t)2 * G * D <= CM_IOU_LDS) {
        for (int i = tid; i < 2 * G * D; i += CM_MATCH_THREADS) {
            const int ty = i / (G * D), gl = i / D % G, k = i % D;
            staged[i] = iou[ty * type_stride + (int64_t)gl * CM_KEEP + k];
        }
        iou = staged;
        type_stride = G * D;
        ring_stride = D;
    }
    __syncthreads();
    if (tid >= 2 * CM_A * CM_T) return;
    const int ty = tid / (CM_A * CM_T), a = tid / CM_T % CM_A, t = tid % CM_T;
    if (!(types >> ty & 1)) return;
    int32_t* gtm = o.gt_match + (int64_t)tid * gt.R;          // tid = (type 4 + a) 10 + t: this thread's rows of the three outputs
    int32_t* dtm = o.dt_match + (int64_t)tid * dt.R;
    uint8_t* dti = o.dt_ignore + (int64_t)tid * dt.R;
    const double start = tb.iou[t] < 1.0 - 1e-10 ? tb.iou[t] : 1.0 - 1e-10;
    for (int k = 0; k < D; ++k) {
        const int d = mine[k];
        double best = start;
        int m = -1;
        for (int pass = 0; pass < 2 && m < 0; ++pass) {          // the gt rings that are not ignored, then, with no match held, the ignored ones
            for (int gl = 0; gl < G; ++gl) {
                const uint8_t f = wg.flags[g0 + gl];
                if ((f & CM_SKIP) || (f >> a & 1) != pass) continue;
                if (gtm[g0 + gl] >= 0) continue;
                const double v = iou[ty * type_stride + (int64_t)gl * ring_stride + k];
                if (v < best) continue;
                best = v;
                m = g0 + gl;
            }
        }
        if (m >= 0) {
            dtm[d] = m;
            gtm[m] = d;
            dti[d] = wg.flags[m] >> a & 1;
        } else {
            dti[d] = wd.flags[d] >> a & 1;
        }
    }
}

// ---- accumulation ---------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int cm_max_dets(int mi) { return mi == 0 ? 1 : (mi == 1 ? 10 : CM_KEEP); }

__global__ __launch_bounds__(PM_THREADS) void cm_order_kernel(PmSet dt, const float* score, const int32_t* dt_rank, int32_t* order) {
    const int i = blockIdx.x * PM_THREADS + threadIdx.x;
    if (i >= dt.R) return;
    const int ri = dt_rank[i];
    int c[CM_M] = {0, 0, 0};
    if (ri >= 0) {
        const float si = cm_score(score, i);
        const int bi = dt.image[i];
        for (int j = 0; j < dt.R; ++j) {
            const int rj = dt_rank[j];
            if (rj < 0) continue;
            const float sj = cm_score(score, j);
            const int bj = dt.image[j];
            const bool before = sj > si || (sj == si && (bj < bi || (bj == bi && rj < ri)));          // stable: image order, then the order in the image
            for (int mi = 0; mi < CM_M; ++mi) c[mi] += before && rj < cm_max_dets(mi);
        }
    }
    for (int mi = 0; mi < CM_M; ++mi) order[(int64_t)mi * dt.R + i] = ri >= 0 && ri < cm_max_dets(mi) ? c[mi] : -1;
}

__global__ __launch_bounds__(PM_THREADS) void cm_series_kernel(int R_gt, int R_dt, CmRings wg, int types, const int32_t* order, uint8_t* flag_ws, int32_t* tp_ws,
                                                               double* pr_ws, CmTables tb, CmOut o) {
    __shared__ unsigned long long red[PM_THREADS / 64];
    __shared__ double red_d[PM_THREADS / 64];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int ty = s / (CM_A * CM_M * CM_T), a = s / (CM_M * CM_T) % CM_A, mi = s / CM_T % CM_M, t = s % CM_T;
    double* prec = o.precision + ((((int64_t)ty * CM_T + t) * CM_R) * CM_A + a) * CM_M + mi;          // + r CM_A CM_M
    double* rec = o.recall + (((int64_t)ty * CM_T + t) * CM_A + a) * CM_M + mi;
    if (!(types >> ty & 1)) {
        if (tid < CM_R) prec[(int64_t)tid * CM_A * CM_M] = pm_nan();
        if (tid == 0) *rec = pm_nan();
        return;
    }
    const int32_t* ord = order + (int64_t)mi * R_dt;
    uint32_t npig = 0, nd = 0;
    for (int g = tid; g < R_gt; g += PM_THREADS) {
        const uint8_t f = wg.flags[g];
        npig += !(f & CM_SKIP) && !(f >> a & 1);
    }
    for (int d = tid; d < R_dt; d += PM_THREADS) nd += ord[d] >= 0;
    unsigned long long both;
    wg_scan<false, unsigned long long>(p3_pack2(npig, nd), red, both);
    npig = (uint32_t)p3_hi32(both);
    nd = (uint32_t)p3_lo32(both);
    if (npig == 0) {          // uniform
        if (tid < CM_R) prec[(int64_t)tid * CM_A * CM_M] = -1.0;
        if (tid == 0) *rec = -1.0;
        return;
    }
    uint8_t* flag = flag_ws + (int64_t)s * R_dt;
    int32_t* tp = tp_ws + (int64_t)s * R_dt;
    double* pr = pr_ws + (int64_t)s * R_dt;
    const int64_t row = ((int64_t)(ty * CM_A + a) * CM_T + t) * R_dt;
    for (int d = tid; d < R_dt; d += PM_THREADS) {
        const int p = ord[d];
        if (p >= 0) flag[p] = o.dt_ignore[row + d] ? 0 : (o.dt_match[row + d] >= 0 ? 1 : 2);
    }
    __syncthreads();
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < nd; base += PM_THREADS) {
        const uint32_t i = base + tid;
        const uint8_t f = i < nd ? flag[i] : 0;
        const unsigned long long v = p3_pack2(f == 1, f == 2);
        const unsigned long long incl = wg_excl<unsigned long long>(v, red, carry) + v;
        if (i < nd) {
            const double ntp = (double)(uint32_t)p3_hi32(incl), nfp = (double)(uint32_t)p3_lo32(incl);
            tp[i] = p3_hi32(incl);
            pr[i] = ntp / (nfp + ntp + 2.220446049250313e-16);
        }
    }
    __syncthreads();
    double right = 0.0;          // the maximum of everything to the right: precision is never negative
    for (uint32_t base = 0; base < nd; base += PM_THREADS) {
        const int64_t i = (int64_t)nd - 1 - base - tid;
        double total;
        double v = wg_scan<true, double>(i >= 0 ? pr[i] : 0.0, red_d, total);
        v = v > right ? v : right;
        if (i >= 0) pr[i] = v;
        right = total > right ? total : right;
    }
    __syncthreads();
    const double den = (double)npig;
    if (tid == 0) *rec = nd ? (double)tp[nd - 1] / den : 0.0;
    if (tid < CM_R) {
        const double want = tb.rec[tid];
        uint32_t lo = 0, hi = nd;          // the first i with tp[i] / npig >= want
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if ((double)tp[mid] / den < want) lo = mid + 1;
            else hi = mid;
        }
        prec[(int64_t)tid * CM_A * CM_M] = lo < nd ? pr[lo] : 0.0;
    }
}

// ---- stats ----------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void cm_stats_kernel(int types, CmOut o) {
    const int tid = threadIdx.x;
    if (tid >= 24) return;
    const int ty = tid / 12, k = tid % 12;
    if (!(types >> ty & 1)) { o.stats[tid] = pm_nan(); return; }
    // pycocotools' summarize: (ap, threshold index or -1 for all, area range, maxDets index)
    const int ap = k < 6, tsel = k == 1 ? 0 : (k == 2 ? 5 : -1);
    const int a = k < 3 ? 0 : (k < 6 ? k - 2 : (k < 9 ? 0 : k - 8));
    const int mi = k < 6 ? 2 : (k < 9 ? k - 6 : 2);
    double sum = 0.0;
    int cnt = 0;
    for (int t = 0; t < CM_T; ++t) {
        if (tsel >= 0 && t != tsel) continue;
        if (ap) {
            for (int r = 0; r < CM_R; ++r) {
                const double v = o.precision[((((int64_t)ty * CM_T + t) * CM_R + r) * CM_A + a) * CM_M + mi];
                if (v > -1.0) { sum += v; ++cnt; }
            }
        } else {
            const double v = o.recall[(((int64_t)ty * CM_T + t) * CM_A + a) * CM_M + mi];
            if (v > -1.0) { sum += v; ++cnt; }
        }
    }
    o.stats[tid] = cnt ? sum / (double)cnt : -1.0;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------------------
static CmRings cm_carve_set(int R, int64_t slab, bool boundary, P3Carve& c) {
    CmRings w;
    w.pm = pm_carve_set(R, c);
    w.ibox = c.take<int32_t>(4 * (int64_t)R);
    w.flags = c.take<uint8_t>(R);
    w.mask = c.take<uint32_t>(R * slab);
    w.hmask = boundary ? c.take<uint32_t>(R * slab) : nullptr;
    w.bmask = boundary ? c.take<uint32_t>(R * slab) : nullptr;
    w.extra = nullptr;
    w.area_px = w.boundary_px = nullptr;
    return w;
}
static CmWs cm_carve(int R_gt, int R_dt, int B, int H, int W, int types, P3Carve& c) {
    const int64_t slab = (int64_t)H * ((W + 31) >> 5);
    const bool boundary = (types & P3_COCO_BOUNDARY) != 0;
    CmWs l;
    l.gt = cm_carve_set(R_gt, slab, boundary, c);
    l.dt = cm_carve_set(R_dt, slab, boundary, c);
    l.kept = c.take<int32_t>((int64_t)B * CM_KEEP);
    l.pair_iou = c.take<double>((int64_t)2 * CM_KEEP * R_gt);
    l.order = c.take<int32_t>((int64_t)CM_M * R_dt);
    l.flag = c.take<uint8_t>((int64_t)CM_SERIES * R_dt);
    l.tp = c.take<int32_t>((int64_t)CM_SERIES * R_dt);
    l.pr = c.take<double>((int64_t)CM_SERIES * R_dt);
    return l;
}
static bool cm_sizes_ok(int R_gt, int R_dt, int B, int H, int W, int types) {
    return R_gt >= 0 && R_dt >= 0 && B >= 1 && H >= 1 && W >= 1 && (int64_t)H * W <= PM_MAX_HW && types > 0 &&
           (types & ~(P3_COCO_SEGM | P3_COCO_BOUNDARY)) == 0;
}

extern "C" void p3_coco_thresholds(double* iou10, double* rec101) {
    if (iou10) memcpy(iou10, cm_iou_thrs, sizeof cm_iou_thrs);
    if (rec101) memcpy(rec101, cm_rec_thrs, sizeof cm_rec_thrs);
}

extern "C" int64_t p3_coco_metrics_workspace_bytes(int R_gt, int R_dt, int B, int H, int W, int iou_types) {
    if (!cm_sizes_ok(R_gt, R_dt, B, H, W, iou_types)) return 0;
    P3Carve c = {nullptr, 0};
    cm_carve(R_gt, R_dt, B, H, W, iou_types, c);
    return c.at;
}

extern "C" int p3_coco_metrics(const float* gt_pos, int64_t V_gt, const int64_t* gt_slice, const int32_t* gt_image, const float* gt_area, int R_gt,
                               const float* dt_pos, int64_t V_dt, const int64_t* dt_slice, const int32_t* dt_image, const float* dt_score, int R_dt, int B, int H,
                               int W, int iou_types, double* stats, double* precision, double* recall, int32_t* gt_area_px, int32_t* dt_area_px,
                               int32_t* gt_boundary_px, int32_t* dt_boundary_px, int32_t* dt_rank, int32_t* pair_inter, int32_t* dt_match, uint8_t* dt_ignore,
                               int32_t* gt_match, int32_t* status, void* workspace, void* stream) {
    P3_CHECK(V_gt >= 0 && V_dt >= 0 && R_gt >= 0 && R_dt >= 0, P3_EINVAL, "p3_coco_metrics: a negative count (V_gt, V_dt, R_gt, R_dt >= 0)");
    P3_CHECK(B >= 1 && H >= 1 && W >= 1, P3_EINVAL, "p3_coco_metrics: bad sizes (B, H, W >= 1)");
    P3_CHECK((int64_t)H * W <= PM_MAX_HW, P3_EINVAL, "p3_coco_metrics: H W above 2^18 (the bound of p3_polygon_metrics)");
    P3_CHECK((int64_t)R_gt + R_dt < ((int64_t)1 << 31) - PM_THREADS && (int64_t)R_gt * CM_KEEP * 2 < ((int64_t)1 << 31) && (int64_t)B * CM_KEEP < ((int64_t)1 << 31),
             P3_EINVAL, "p3_coco_metrics: R_gt + R_dt must stay below 2^31 - 256, 200 R_gt and 100 B below 2^31");
    P3_CHECK(iou_types > 0 && (iou_types & ~(P3_COCO_SEGM | P3_COCO_BOUNDARY)) == 0, P3_EINVAL,
             "p3_coco_metrics: iou_types is a non-empty set of P3_COCO_SEGM | P3_COCO_BOUNDARY");
    P3_CHECK(stats && precision && recall && status, P3_EINVAL, "p3_coco_metrics: null pointer (stats, precision, recall, status)");
    P3_CHECK(R_gt == 0 || (gt_pos && gt_slice && gt_image && gt_area_px && gt_boundary_px && pair_inter && gt_match), P3_EINVAL,
             "p3_coco_metrics: null pointer (gt_pos, gt_slice, gt_image, gt_area_px, gt_boundary_px, pair_inter, gt_match)");
    P3_CHECK(R_dt == 0 || (dt_pos && dt_slice && dt_image && dt_area_px && dt_boundary_px && dt_rank && dt_match && dt_ignore), P3_EINVAL,
             "p3_coco_metrics: null pointer (dt_pos, dt_slice, dt_image, dt_area_px, dt_boundary_px, dt_rank, dt_match, dt_ignore)");
    P3_CHECK((R_gt == 0 || !(p3_host_array(gt_slice) || p3_host_array(gt_image))) && (R_dt == 0 || !(p3_host_array(dt_slice) || p3_host_array(dt_image))),
             P3_EINVAL, "p3_coco_metrics: ring_slice and ring_image must be device memory");
    P3_CHECK((R_gt == 0 || !gt_area || !p3_host_array(gt_area)) && (R_dt == 0 || !dt_score || !p3_host_array(dt_score)), P3_EINVAL,
             "p3_coco_metrics: score and area must be device memory");
    const int64_t need = p3_coco_metrics_workspace_bytes(R_gt, R_dt, B, H, W, iou_types);
    P3_CHECK(need == 0 || workspace, P3_EINVAL, "p3_coco_metrics: null workspace (p3_coco_metrics_workspace_bytes(R_gt, R_dt, B, H, W, iou_types))");
    hipStream_t s = (hipStream_t)stream;
    P3Carve carve = {(char*)workspace, 0};
    CmWs l = cm_carve(R_gt, R_dt, B, H, W, iou_types, carve);
    l.gt.extra = gt_area; l.gt.area_px = gt_area_px; l.gt.boundary_px = gt_boundary_px;
    l.dt.extra = dt_score; l.dt.area_px = dt_area_px; l.dt.boundary_px = dt_boundary_px;
    const PmSet gt = {(const float2*)gt_pos, gt_slice, gt_image, V_gt, R_gt}, dt = {(const float2*)dt_pos, dt_slice, dt_image, V_dt, R_dt};
    const CmOut o = {stats, precision, recall, dt_rank, pair_inter, dt_match, dt_ignore, gt_match, status};
    const int boundary = (iou_types & P3_COCO_BOUNDARY) != 0;
    const int rows = 2 * CM_A * CM_T;
    CmTables tb;
    memcpy(tb.iou, cm_iou_thrs, sizeof cm_iou_thrs);
    memcpy(tb.rec, cm_rec_thrs, sizeof cm_rec_thrs);
    const double diag = 0.02 * sqrt((double)H * (double)H + (double)W * (double)W);
    const int dil = (int)fmax(1.0, rint(diag));          // round-half-even
    P3_TRY(p3_memset(status, 0, sizeof(int32_t), s));
    P3_TRY(p3_memset(l.kept, 0xff, (int64_t)B * CM_KEEP * sizeof(int32_t), s));
    if (R_gt > 0) {
        P3_TRY(p3_memset(pair_inter, 0, (int64_t)2 * CM_KEEP * R_gt * sizeof(int32_t), s));
        P3_TRY(p3_memset(l.pair_iou, 0, (int64_t)2 * CM_KEEP * R_gt * sizeof(double), s));
        P3_TRY(p3_memset(gt_match, 0xff, (int64_t)rows * R_gt * sizeof(int32_t), s));
    }
    if (R_dt > 0) {
        P3_TRY(p3_memset(dt_match, 0xff, (int64_t)rows * R_dt * sizeof(int32_t), s));
        P3_TRY(p3_memset(dt_ignore, 0, (int64_t)rows * R_dt, s));
    }
    if (R_gt + R_dt > 0) {
        P3_TRY(p3_launch<cm_ring_kernel>(nullptr, p3_ceil_div((int64_t)R_gt + R_dt, PM_THREADS), PM_THREADS, 0, s, gt, dt, l.gt, l.dt, B, status));
        P3_TRY(p3_launch<cm_raster_kernel>("cm_raster_kernel", R_gt + R_dt, PM_THREADS, 0, s, gt, dt, l.gt, l.dt, H, W, dil, boundary, l.kept, o));
    }
    const int slots = R_dt < CM_KEEP ? R_dt : CM_KEEP;
    if (R_gt > 0 && slots > 0)
        P3_TRY(p3_launch<cm_pair_kernel>("cm_pair_kernel", p3_ceil_div((int64_t)R_gt * slots, PM_THREADS / 64), PM_THREADS, 0, s, gt, l.gt, l.dt, slots, H, W,
                                         boundary, l.kept, l.pair_iou, o));
    P3_TRY(p3_launch<cm_match_kernel>("cm_match_kernel", B, CM_MATCH_THREADS, 0, s, gt, dt, l.gt, l.dt, iou_types, l.kept, l.pair_iou, tb, o));
    if (R_dt > 0) P3_TRY(p3_launch<cm_order_kernel>(nullptr, p3_ceil_div(R_dt, PM_THREADS), PM_THREADS, 0, s, dt, dt_score, dt_rank, l.order));
    P3_TRY(p3_launch<cm_series_kernel>("cm_series_kernel", CM_SERIES, PM_THREADS, 0, s, R_gt, R_dt, l.gt, iou_types, l.order, l.flag, l.tp, l.pr, tb, o));
    P3_TRY(p3_launch<cm_stats_kernel>(nullptr, 1, 64, 0, s, iou_types, o));
    return P3_OK;
}
