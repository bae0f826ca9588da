// p3hip — mask and topology metrics, subset IoU and annotation counts of a predicted ring set against a ground-truth ring set (gfx950): the modes `topdig`,
// `subset_iou` and `stats` of the reference's Evaluator.evaluate, from the packed rings to the nine means and seven counts on the device.  include/p3hip.h
// (p3_mask_metrics) and DESIGN.md section 24 hold the definition.
//   mm_ring_kernel     one thread per ring of either set: validity, vertex count, box (pm_rings.h)
//   mm_mask_kernel     one workgroup per image, two bit-packed masks in LDS (2 x H W / 8 bytes, at most 64 KB, and 1 KB of staged edges): the filled pair
//                      (pm_raster_set) and its TP / FP / FN, then in the same LDS the stroked pair: integer end points of 32 edges staged at a time, units of
//                      (edge, position along the edge's longer axis), the few candidates across it tested exactly, a word's bits ORed with one atomicOr
//   mm_finish_kernel   one workgroup: a thread per image makes its figures, NR, subset flag, invalid_rings and counts; thread 0 sums them in image order
// The filled masks are doubles as in poly_metrics.hip (contraction off); everything about the stroke is integer arithmetic.
#include "pm_rings.h"          // the ring set, ring validity, pm_raster_set

#pragma clang fp contract(off)

constexpr int MM_MAX_THICKNESS = 64;
constexpr int MM_MASK_BITS = P3_MM_TOPDIG | P3_MM_SUBSET;          // the modes that need the mask kernel

struct MmOut {
    double* metrics;
    int64_t* stats;
    int32_t* image_conf;            // [B, 2, 4] = (filled, stroked) x (TP, FP, FN, TN)
    double* image_scores;           // [B, 6]
    double* image_nr;
    int32_t* image_subset;
    int32_t* invalid_rings;         // [B, 2] = (gt, prediction)
    int32_t* status;
};

// ---- rings ----------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PM_THREADS) void mm_ring_kernel(PmSet gt, PmSet dt, PmRings wg, PmRings wd, int B, MmOut o) {
    const int r = blockIdx.x * PM_THREADS + threadIdx.x;
    if (r < gt.R) pm_ring(gt, wg, r, B, o.status);
    else if (r - gt.R < dt.R) pm_ring(dt, wd, r - gt.R, B, o.status);
}

// ---- the stroked mask -----------------------------------------------------------------------------------------------------------------------------------
// one chunk of a ring's edges in LDS: the integer end points, the first position along the longer axis whose line can hold a pixel of the band, and the
// exclusive prefix of the number of such positions
struct MmChunk {
    int ax[PM_EDGE_CHUNK], ay[PM_EDGE_CHUNK], bx[PM_EDGE_CHUNK], by[PM_EDGE_CHUNK], lo[PM_EDGE_CHUNK], pre[PM_EDGE_CHUNK + 1];
};
static_assert(sizeof(MmChunk) <= PM_EDGE_CHUNK * sizeof(PmEdge), "the staged end points of the stroke lie where the filled pass stages its edges");

__device__ __forceinline__ int64_t mm_floor_div(int64_t a, int64_t b) {          // b > 0
    const int64_t q = a / b;
    return q * b > a ? q - 1 : q;
}
__device__ __forceinline__ int64_t mm_ceil_div(int64_t a, int64_t b) { return -mm_floor_div(-a, b); }          // b > 0

// pixel p = (px, py) lies within T / 2 of the segment (a, b): include/p3hip.h p3_mask_metrics step 2, TT = T T.  |coordinates| <= 2^15, 0 <= p < 2^18: u and d
// stay below 2^19 and 2^17, u.d and the cross product below 2^37; a cross product above 2^23 fails whatever L2 is (4 x 2^46 > 2^12 x 2^34 > TT L2), so its
// square is only taken where it is at most 2^46
__device__ __forceinline__ bool mm_in_band(int64_t px, int64_t py, int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t TT) {
    const int64_t dx = bx - ax, dy = by - ay, ux = px - ax, uy = py - ay;
    const int64_t L2 = dx * dx + dy * dy, t = ux * dx + uy * dy;
    if (L2 == 0 || t <= 0) return 4 * (ux * ux + uy * uy) <= TT;
    if (t >= L2) {
        const int64_t vx = px - bx, vy = py - by;
        return 4 * (vx * vx + vy * vy) <= TT;
    }
    const int64_t cr = ux * dy - uy * dx;
    if (cr > ((int64_t)1 << 23) || cr < -((int64_t)1 << 23)) return false;
    return 4 * cr * cr <= TT * L2;
}

// the outlines of the valid rings of one set of image b into `mask`, T pixels thick.  Every thread of the workgroup calls it.  An edge is walked along its
// longer axis (the major one: y unless |dx| > |dy|): a unit is one position m on that axis within h = ceil(T / 2) of the edge's extent; its candidates are
// the positions k across it that the part of the segment within h of m reaches, widened by h: at most 4 h + 3 of them, since the segment's slope across is
// at most 1.  A pixel within T / 2 of the segment has its nearest point within h on either axis, so no pixel of the band is missed; each candidate is tested
// exactly.
__device__ void mm_stroke_set(const PmSet& s, const PmRings& w, int b, int H, int W, int T, uint32_t* mask, MmChunk& c, int* red) {
    const int tid = threadIdx.x;
    const int h = (T + 1) >> 1;
    const int64_t TT = (int64_t)T * T;
    const int r_lo = pm_lower(s.image, s.R, b), r_hi = pm_lower(s.image, s.R, b + 1);
    for (int r = r_lo; r < r_hi; ++r) {
        if (w.state[r] != 1) continue;          // uniform over the workgroup
        const int n = w.n[r];
        const float2* v = s.pos + w.first[r];
        for (int e0 = 0; e0 < n; e0 += PM_EDGE_CHUNK) {
            const int cnt = n - e0 < PM_EDGE_CHUNK ? n - e0 : PM_EDGE_CHUNK;
            __syncthreads();          // the last chunk has been read
            int units = 0;
            if (tid < cnt) {
                const int i = e0 + tid, j = i + 1 == n ? 0 : i + 1;
                const float2 pa = v[i], pb = v[j];
                const int ax = (int)rint((double)pa.x), ay = (int)rint((double)pa.y), bx = (int)rint((double)pb.x), by = (int)rint((double)pb.y);
                const bool swap = abs(bx - ax) > abs(by - ay);          // x is the major axis
                const int am = swap ? ax : ay, bm = swap ? bx : by, M = swap ? W : H;
                const int lo = max(min(am, bm) - h, 0), hi = min(max(am, bm) + h, M - 1);
                units = hi >= lo ? hi - lo + 1 : 0;          // <= M <= 2^18, 32 of them: far inside int32
                c.ax[tid] = ax; c.ay[tid] = ay; c.bx[tid] = bx; c.by[tid] = by; c.lo[tid] = lo;
            }
            int total;
            const int incl = wg_scan<false, int>(units, red, total);
            if (tid < cnt) c.pre[tid] = incl - units;
            if (tid == 0) c.pre[cnt] = total;
            __syncthreads();
            for (int u = tid; u < total; u += PM_THREADS) {
                int e = 0, top = cnt - 1;          // the last edge whose prefix is <= u
                while (e < top) {
                    const int mid = (e + top + 1) >> 1;
                    if (c.pre[mid] <= u) e = mid;
                    else top = mid - 1;
                }
                const int ax = c.ax[e], ay = c.ay[e], bx = c.bx[e], by = c.by[e];
                const bool swap = abs(bx - ax) > abs(by - ay);
                const int m = c.lo[e] + (u - c.pre[e]);
                const int am = swap ? ax : ay, bm = swap ? bx : by, ak = swap ? ay : ax, bk = swap ? by : bx, K = swap ? H : W;
                int k0, k1;          // the candidates across
                if (am == bm) {          // |dk| <= |dm| = 0: a point
                    k0 = k1 = ak;
                } else {
                    const int m_lo = max(m - h, min(am, bm)), m_hi = min(m + h, max(am, bm));          // not empty: m lies within h of the extent
                    const int64_t dm = bm - am, dk = bk - ak, sg = dm > 0 ? 1 : -1;          // k(m) = ak + dk (m - am) / dm, monotone in m
                    const int64_t n0 = sg * dk * (m_lo - am), n1 = sg * dk * (m_hi - am), den = sg * dm;
                    const int64_t f0 = mm_floor_div(n0, den), f1 = mm_floor_div(n1, den), c0 = mm_ceil_div(n0, den), c1 = mm_ceil_div(n1, den);
                    k0 = ak + (int)(f0 < f1 ? f0 : f1);
                    k1 = ak + (int)(c0 > c1 ? c0 : c1);
                }
                k0 = max(k0 - h, 0);
                k1 = min(k1 + h, K - 1);
                int word = -1;
                uint32_t bits = 0;
                for (int k = k0; k <= k1; ++k) {
                    const int px = swap ? m : k, py = swap ? k : m;
                    if (!mm_in_band(px, py, ax, ay, bx, by, TT)) continue;
                    const int bit = py * W + px;          // H W <= 2^18: no overflow
                    if ((bit >> 5) != word) {
                        if (bits) atomicOr(mask + word, bits);
                        word = bit >> 5;
                        bits = 0;
                    }
                    bits |= 1u << (bit & 31);
                }
                if (bits) atomicOr(mask + word, bits);
            }
        }
    }
}

// TP, FP, FN of the two masks in LDS, then TN: one row of image_conf.  Every thread of the workgroup calls it, behind a barrier.
__device__ void mm_confusion(const uint32_t* mg, const uint32_t* md, int words, int HW, int* red, int32_t* conf) {
    int tp = 0, fp = 0, fn = 0;
    for (int i = threadIdx.x; i < words; i += PM_THREADS) {
        const uint32_t g = mg[i], p = md[i];
        tp += __popc(p & g); fp += __popc(p & ~g); fn += __popc(~p & g);
    }
    int ttp, tfp, tfn;
    wg_scan<false, int>(tp, red, ttp);
    wg_scan<false, int>(fp, red, tfp);
    wg_scan<false, int>(fn, red, tfn);
    if (threadIdx.x == 0) {
        conf[0] = ttp; conf[1] = tfp; conf[2] = tfn; conf[3] = HW - ttp - tfp - tfn;
    }
}

__global__ __launch_bounds__(PM_THREADS) void mm_mask_kernel(PmSet gt, PmSet dt, PmRings wg, PmRings wd, int H, int W, int T, int modes, MmOut o) {
    extern __shared__ __attribute__((aligned(16))) uint32_t mm_lds[];
    __shared__ int red[PM_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int words = (H * W + 31) >> 5;
    uint32_t* mg = mm_lds;
    uint32_t* md = mm_lds + words;
    PmEdge* edges = (PmEdge*)(mm_lds + 2 * words);          // an even number of 4-byte words behind a 16-byte aligned base: the doubles are 8-byte aligned
    int32_t* conf = o.image_conf + 8 * (int64_t)b;
    for (int i = tid; i < 2 * words; i += PM_THREADS) mm_lds[i] = 0;
    __syncthreads();
    pm_raster_set(gt, wg, b, H, W, mg, edges);
    pm_raster_set(dt, wd, b, H, W, md, edges);
    __syncthreads();
    mm_confusion(mg, md, words, H * W, red, conf);          // ends on wg_scan's barrier: the masks have been read
    if (!(modes & P3_MM_TOPDIG)) {
        if (tid < 4) conf[4 + tid] = 0;
        return;
    }
    for (int i = tid; i < 2 * words; i += PM_THREADS) mm_lds[i] = 0;
    MmChunk& chunk = *(MmChunk*)edges;          // mm_stroke_set starts on a barrier: the masks are clear and the filled pass has read its last edges
    mm_stroke_set(gt, wg, b, H, W, T, mg, chunk, red);
    mm_stroke_set(dt, wd, b, H, W, T, md, chunk, red);
    __syncthreads();
    mm_confusion(mg, md, words, H * W, red, conf + 4);
}

// ---- per image, per set ---------------------------------------------------------------------------------------------------------------------------------
// (iou, acc, f1) of one row of image_conf: step 3
__device__ __forceinline__ void mm_scores(const int32_t* conf, int HW, double* out) {
    const int tp = conf[0], fp = conf[1], fn = conf[2], tn = conf[3];
    if (tp + fp + fn == 0) {
        out[0] = out[1] = out[2] = 1.0;
        return;
    }
    out[0] = (double)tp / ((double)(tp + fp + fn) + 1e-9);
    out[1] = (double)(tp + tn) / (double)HW;
    out[2] = (double)(2 * tp) / (double)(2 * tp + fp + fn);
}

// the rings of image b in one set: invalid ones, the vertices of the valid ones, the counted ones (not left out) and their slice lengths
__device__ __forceinline__ void mm_count_set(const PmSet& s, const PmRings& w, int r0, int r1, int& bad, int64_t& valid_vertices, int64_t& rings, int64_t& vertices) {
    bad = 0;
    valid_vertices = rings = vertices = 0;
    for (int r = r0; r < r1; ++r) {
        const int st = w.state[r];
        if (st < 0) continue;          // left out: its slice may not be one
        bad += st == 0;
        valid_vertices += w.n[r];          // 0 for an invalid ring
        ++rings;
        vertices += s.slice[2 * r + 1] - s.slice[2 * r];
    }
}

__global__ __launch_bounds__(PM_THREADS) void mm_finish_kernel(PmSet gt, PmSet dt, PmRings wg, PmRings wd, int64_t* counts, int B, int HW, int modes, MmOut o) {
    const double nan = pm_nan();
    for (int b = threadIdx.x; b < B; b += PM_THREADS) {
        const int g0 = pm_lower(gt.image, gt.R, b), g1 = pm_lower(gt.image, gt.R, b + 1);
        const int d0 = pm_lower(dt.image, dt.R, b), d1 = pm_lower(dt.image, dt.R, b + 1);
        int bad_g, bad_d;
        int64_t nv_g, nv_d;
        int64_t* cnt = counts + 4 * (int64_t)b;          // (gt rings, prediction rings, gt vertices, prediction vertices) of the image
        mm_count_set(gt, wg, g0, g1, bad_g, nv_g, cnt[0], cnt[2]);
        mm_count_set(dt, wd, d0, d1, bad_d, nv_d, cnt[1], cnt[3]);
        o.invalid_rings[2 * b] = bad_g;
        o.invalid_rings[2 * b + 1] = bad_d;
        int32_t* conf = o.image_conf + 8 * (int64_t)b;
        double* sc = o.image_scores + 6 * (int64_t)b;
        if (!(modes & MM_MASK_BITS)) {
            for (int k = 0; k < 8; ++k) conf[k] = 0;
        }
        if (modes & P3_MM_TOPDIG) {
            mm_scores(conf, HW, sc);
            mm_scores(conf + 4, HW, sc + 3);
        } else {
            for (int k = 0; k < 6; ++k) sc[k] = nan;
        }
        if (modes & P3_MM_SUBSET) {
            const double ng = (double)nv_g, nd = (double)nv_d;
            o.image_nr[b] = 1.0 - fabs(nd - ng) / (nd + ng + 1e-9);
            o.image_subset[b] = d1 > d0;
        } else {
            o.image_nr[b] = nan;
            o.image_subset[b] = 0;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, s_iou = 0.0, s_ciou = 0.0, s_nr = 0.0;
    int64_t st[7] = {B, 0, 0, 0, 0, 0, 0};
    int in_subset = 0;
    for (int b = 0; b < B; ++b) {          // image order
        if (modes & P3_MM_TOPDIG) {
            for (int k = 0; k < 6; ++k) sum[k] += o.image_scores[6 * (int64_t)b + k];
        }
        if ((modes & P3_MM_SUBSET) && o.image_subset[b]) {
            double f[3];
            mm_scores(o.image_conf + 8 * (int64_t)b, HW, f);
            const double nr = o.image_nr[b];
            ++in_subset;
            s_iou += f[0];
            s_ciou += f[0] * nr;
            s_nr += nr;
        }
        const int64_t* cnt = counts + 4 * (int64_t)b;
        st[1] += cnt[0] > 0; st[2] += cnt[1] > 0;
        st[3] += cnt[0]; st[4] += cnt[1]; st[5] += cnt[2]; st[6] += cnt[3];
    }
    for (int k = 0; k < 6; ++k) o.metrics[k] = (modes & P3_MM_TOPDIG) ? sum[k] / (double)B : nan;
    o.metrics[6] = in_subset ? s_iou / (double)in_subset : nan;
    o.metrics[7] = in_subset ? s_ciou / (double)in_subset : nan;
    o.metrics[8] = in_subset ? s_nr / (double)in_subset : nan;
    for (int k = 0; k < 7; ++k) o.stats[k] = (modes & P3_MM_STATS) ? st[k] : 0;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------------------
struct MmWs {
    PmRings gt, dt;
    int64_t* counts;          // [B, 4]
};
static MmWs mm_carve(int R_gt, int R_dt, int B, P3Carve& c) {
    MmWs l;
    l.gt = pm_carve_set(R_gt, c);
    l.dt = pm_carve_set(R_dt, c);
    l.counts = c.take<int64_t>(4 * (int64_t)B);
    return l;
}

extern "C" int64_t p3_mask_metrics_workspace_bytes(int R_gt, int R_dt, int B) {
    if (R_gt < 0 || R_dt < 0 || B < 1) return 0;
    P3Carve c = {nullptr, 0};
    mm_carve(R_gt, R_dt, B, c);
    return c.at;
}

extern "C" int p3_mask_metrics(const float* gt_pos, int64_t V_gt, const int64_t* gt_slice, const int32_t* gt_image, int R_gt, const float* dt_pos, int64_t V_dt,
                               const int64_t* dt_slice, const int32_t* dt_image, int R_dt, int B, int H, int W, int buffer_thickness, int modes,
                               double* metrics, int64_t* stats, int32_t* image_conf, double* image_scores, double* image_nr, int32_t* image_subset,
                               int32_t* invalid_rings, int32_t* status, void* workspace, void* stream) {
    P3_CHECK(V_gt >= 0 && V_dt >= 0 && R_gt >= 0 && R_dt >= 0, P3_EINVAL, "p3_mask_metrics: a negative count (V_gt, V_dt, R_gt, R_dt >= 0)");
    P3_CHECK(B >= 1 && H >= 1 && W >= 1, P3_EINVAL, "p3_mask_metrics: bad sizes (B, H, W >= 1)");
    P3_CHECK((int64_t)H * W <= PM_MAX_HW, P3_EINVAL, "p3_mask_metrics: H W above 2^18 (the bound of p3_polygon_metrics: two masks of an image are held in LDS)");
    P3_CHECK((int64_t)R_gt + R_dt < ((int64_t)1 << 31) - PM_THREADS, P3_EINVAL, "p3_mask_metrics: R_gt + R_dt must stay below 2^31 - 256");
    P3_CHECK(buffer_thickness >= 1 && buffer_thickness <= MM_MAX_THICKNESS, P3_EINVAL, "p3_mask_metrics: buffer_thickness must lie in [1, 64]");
    P3_CHECK(modes > 0 && (modes & ~(P3_MM_TOPDIG | P3_MM_SUBSET | P3_MM_STATS)) == 0, P3_EINVAL, "p3_mask_metrics: modes is a non-empty set of P3_MM_* bits");
    P3_CHECK(metrics && stats && image_conf && image_scores && image_nr && image_subset && invalid_rings && status, P3_EINVAL,
             "p3_mask_metrics: null pointer (metrics, stats, image_conf, image_scores, image_nr, image_subset, invalid_rings, status)");
    P3_CHECK(R_gt == 0 || (gt_pos && gt_slice && gt_image), P3_EINVAL, "p3_mask_metrics: null pointer (gt_pos, gt_slice, gt_image)");
    P3_CHECK(R_dt == 0 || (dt_pos && dt_slice && dt_image), P3_EINVAL, "p3_mask_metrics: null pointer (dt_pos, dt_slice, dt_image)");
    P3_CHECK((R_gt == 0 || !(p3_host_array(gt_slice) || p3_host_array(gt_image))) && (R_dt == 0 || !(p3_host_array(dt_slice) || p3_host_array(dt_image))),
             P3_EINVAL, "p3_mask_metrics: ring_slice and ring_image must be device memory");
    P3_CHECK(workspace, P3_EINVAL, "p3_mask_metrics: null workspace (p3_mask_metrics_workspace_bytes(R_gt, R_dt, B))");
    hipStream_t s = (hipStream_t)stream;
    P3Carve carve = {(char*)workspace, 0};
    const MmWs l = mm_carve(R_gt, R_dt, B, carve);
    const PmSet gt = {(const float2*)gt_pos, gt_slice, gt_image, V_gt, R_gt}, dt = {(const float2*)dt_pos, dt_slice, dt_image, V_dt, R_dt};
    const MmOut o = {metrics, stats, image_conf, image_scores, image_nr, image_subset, invalid_rings, status};
    P3_TRY(p3_memset(status, 0, sizeof(int32_t), s));
    if (R_gt + R_dt > 0) P3_TRY(p3_launch<mm_ring_kernel>(nullptr, p3_ceil_div((int64_t)R_gt + R_dt, PM_THREADS), PM_THREADS, 0, s, gt, dt, l.gt, l.dt, B, o));
    if (modes & MM_MASK_BITS) {
        const int words = (H * W + 31) >> 5;
        const size_t lds = (size_t)(2 * words) * sizeof(uint32_t) + PM_EDGE_CHUNK * sizeof(PmEdge);
        P3_TRY(p3_launch<mm_mask_kernel>("mm_mask_kernel", B, PM_THREADS, lds, s, gt, dt, l.gt, l.dt, H, W, buffer_thickness, modes, o));
    }
    P3_TRY(p3_launch<mm_finish_kernel>(nullptr, 1, PM_THREADS, 0, s, gt, dt, l.gt, l.dt, l.counts, B, H * W, modes, o));
    return P3_OK;
}
