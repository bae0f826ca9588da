// p3hip — polygon metrics (gfx950): IoU / C-IoU / NR, POLIS, chamfer and Hausdorff of a predicted ring set against a ground-truth ring set, per image and
// over the batch, from the packed rings to the six means on the device.  include/p3hip.h (p3_polygon_metrics) and DESIGN.md section 21 hold the definition.
//   pm_ring_kernel     one thread per ring of either set: valid / invalid / left out, vertex count, box; match = -1 and pair_* = NaN for every gt ring
//   pm_raster_kernel   one workgroup per image: both masks bit-packed in LDS (even-odd at pixel centres, union over the rings), I = |gt & dt|, U = |gt | dt|
//   pm_match_kernel    one workgroup per image: per gt ring the first argmax of the box IoU over the image's predictions, counted when > 0.5; NR; invalid_rings
//   pm_pair_kernel     one workgroup per gt ring: POLIS over vertices x edges, chamfer and Hausdorff over the 0.1 px samples, which are made on the fly
//   pm_finish_kernel   one workgroup: per-image figures, then the six means in image order
// Every floating-point value is a double made of the fp32 coordinates; contraction is off for the whole file, so that a product and the sum behind it round as
// the float64 restatement (tests/poly_metrics_ref.py) rounds them: sample counts, crossings and the argmax are then the restatement's.
#include "pm_rings.h"          // the ring set, ring validity, the crossing rule and pm_raster_set, shared with the other scoring stages

#pragma clang fp contract(off)

constexpr int PM_OWN = 4;                  // samples a thread owns in registers
constexpr int PM_TILE = PM_THREADS * PM_OWN;          // samples of the other ring in LDS at a time, and the samples the workgroup owns at a time
constexpr double PM_STEP = 0.1;            // segmentize(0.1)

struct PmOut {
    double* metrics;
    double* image_iou;
    double* image_nr;
    double* image_polis;
    double* image_chamfer;
    double* image_hausdorff;
    int32_t* image_valid;
    int32_t* image_counts;          // [B, 2] = (I, U)
    int32_t* match;
    double* pair_polis;
    double* pair_chamfer;
    double* pair_hausdorff;
    int32_t* invalid_rings;         // [B, 2] = (gt, prediction)
    int32_t* status;
};

// ---- rings ----------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PM_THREADS) void pm_ring_kernel(PmSet gt, PmSet dt, PmRings wg, PmRings wd, int B, PmOut o) {
    const int r = blockIdx.x * PM_THREADS + threadIdx.x;
    if (r < gt.R) {
        pm_ring(gt, wg, r, B, o.status);
        o.match[r] = -1;
        o.pair_polis[r] = o.pair_chamfer[r] = o.pair_hausdorff[r] = pm_nan();
    } else if (r - gt.R < dt.R) {
        pm_ring(dt, wd, r - gt.R, B, o.status);
    }
}

// ---- masks, I and U -------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PM_THREADS) void pm_raster_kernel(PmSet gt, PmSet dt, PmRings wg, PmRings wd, int H, int W, PmOut o) {
    extern __shared__ __attribute__((aligned(16))) uint32_t pm_lds[];
    __shared__ int red[PM_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int words = (H * W + 31) >> 5;
    uint32_t* mg = pm_lds;
    uint32_t* md = pm_lds + words;
    PmEdge* edges = (PmEdge*)(pm_lds + 2 * words);          // an even number of 4-byte words behind a 16-byte aligned base: the doubles are 8-byte aligned
    for (int i = tid; i < 2 * words; i += PM_THREADS) pm_lds[i] = 0;
    __syncthreads();
    pm_raster_set(gt, wg, b, H, W, mg, edges);
    pm_raster_set(dt, wd, b, H, W, md, edges);
    __syncthreads();
    int ni = 0, nu = 0;
    for (int i = tid; i < words; i += PM_THREADS) {
        ni += __popc(mg[i] & md[i]);
        nu += __popc(mg[i] | md[i]);
    }
    int ti, tu;
    wg_scan<false, int>(ni, red, ti);
    wg_scan<false, int>(nu, red, tu);
    if (tid == 0) {
        o.image_counts[2 * b] = ti;
        o.image_counts[2 * b + 1] = tu;
    }
}

// ---- matching -------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double pm_box_iou(const double* g, const double* d) {
    const double gx1 = g[0] + g[2], dx1 = d[0] + d[2], gy1 = g[1] + g[3], dy1 = d[1] + d[3];
    const double iw = (gx1 < dx1 ? gx1 : dx1) - (g[0] > d[0] ? g[0] : d[0]);
    const double ih = (gy1 < dy1 ? gy1 : dy1) - (g[1] > d[1] ? g[1] : d[1]);
    if (iw <= 0.0 || ih <= 0.0) return 0.0;
    const double i = iw * ih;
    const double ag = g[2] * g[3], ad = d[2] * d[3];
    return i / (ag + ad - i);
}

__global__ __launch_bounds__(PM_THREADS) void pm_match_kernel(PmSet gt, PmSet dt, PmRings wg, PmRings wd, PmOut o) {
    __shared__ unsigned long long red[PM_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int g0 = pm_lower(gt.image, gt.R, b), g1 = pm_lower(gt.image, gt.R, b + 1);
    const int d0 = pm_lower(dt.image, dt.R, b), d1 = pm_lower(dt.image, dt.R, b + 1);
    uint32_t nv_g = 0, nv_d = 0, bad_g = 0, bad_d = 0;
    for (int g = g0 + tid; g < g1; g += PM_THREADS) {
        const int st = wg.state[g];
        bad_g += st == 0;
        if (st != 1) continue;
        nv_g += wg.n[g];
        const double* gb = wg.box + 4 * (int64_t)g;
        int best = -1;
        double best_iou = -1.0;
        for (int d = d0; d < d1; ++d) {
            if (wd.state[d] != 1) continue;
            const double v = pm_box_iou(gb, wd.box + 4 * (int64_t)d);
            if (v > best_iou) { best_iou = v; best = d; }          // the first argmax
        }
        if (best >= 0 && best_iou > 0.5) o.match[g] = best;
    }
    for (int d = d0 + tid; d < d1; d += PM_THREADS) {
        const int st = wd.state[d];
        bad_d += st == 0;
        if (st == 1) nv_d += wd.n[d];
    }
    unsigned long long tv, tb;
    wg_scan<false, unsigned long long>(p3_pack2(nv_g, nv_d), red, tv);          // a ring has fewer than 2^30 vertices; an image of more than 2^32 is not met
    wg_scan<false, unsigned long long>(p3_pack2(bad_g, bad_d), red, tb);
    if (tid == 0) {
        const double ng = (double)(uint32_t)p3_hi32(tv), nd = (double)(uint32_t)p3_lo32(tv);
        o.image_nr[b] = 1.0 - fabs(nd - ng) / (nd + ng + 1e-9);
        o.invalid_rings[2 * b] = p3_hi32(tb);
        o.invalid_rings[2 * b + 1] = p3_lo32(tb);
    }
}

// ---- pairs ----------------------------------------------------------------------------------------------------------------------------------------------
struct PmRingRef { const float2* v; int n; };
// one chunk of a ring's edges in LDS: end points, length, sample count and the exclusive prefix of the counts; `total` includes the closing sample behind the last edge
struct PmChunk {
    double x[PM_EDGE_CHUNK + 1], y[PM_EDGE_CHUNK + 1], L[PM_EDGE_CHUNK];
    int m[PM_EDGE_CHUNK], pre[PM_EDGE_CHUNK + 1];
    double x_first, y_first;
    int cnt, total, closes;
};

__device__ __forceinline__ double pm_vx(const PmRingRef& r, int i) { return (double)r.v[i].x; }
__device__ __forceinline__ double pm_vy(const PmRingRef& r, int i) { return (double)r.v[i].y; }

// every thread of the workgroup calls it; ends on a barrier
__device__ void pm_chunk_build(const PmRingRef& r, int e0, PmChunk& c, int* red) {
    const int tid = threadIdx.x;
    const int cnt = r.n - e0 < PM_EDGE_CHUNK ? r.n - e0 : PM_EDGE_CHUNK;
    __syncthreads();          // the chunk's last readers are done
    int m = 0;
    if (tid < cnt) {
        const int i = e0 + tid, j = i + 1 == r.n ? 0 : i + 1;
        const double px = pm_vx(r, i), py = pm_vy(r, i), qx = pm_vx(r, j), qy = pm_vy(r, j);
        const double dx = qx - px, dy = qy - py;
        const double L = __dsqrt_rn(dx * dx + dy * dy);
        const double k = ceil(L / PM_STEP);          // <= 2^16 sqrt(2) / 0.1: far inside int32
        m = k > 1.0 ? (int)k : 1;
        c.x[tid] = px; c.y[tid] = py; c.L[tid] = L; c.m[tid] = m;
        if (tid == cnt - 1) { c.x[cnt] = qx; c.y[cnt] = qy; }
    }
    int tot;
    const int incl = wg_scan<false, int>(m, red, tot);
    if (tid < cnt) c.pre[tid] = incl - m;
    if (tid == 0) {
        const int closes = e0 + cnt == r.n;
        c.cnt = cnt;
        c.closes = closes;
        c.total = tot + closes;
        c.pre[cnt] = tot;
        c.x_first = pm_vx(r, 0);
        c.y_first = pm_vy(r, 0);
    }
    __syncthreads();
}

// sample i < c.total of the chunk
__device__ __forceinline__ void pm_sample(const PmChunk& c, int i, double& sx, double& sy) {
    if (i >= c.pre[c.cnt]) { sx = c.x_first; sy = c.y_first; return; }          // the closing sample: the first vertex once more
    int lo = 0, hi = c.cnt - 1;          // the last edge whose prefix is <= i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (c.pre[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    const double px = c.x[lo], py = c.y[lo], L = c.L[lo];
    if (!(L > 0.0)) { sx = px; sy = py; return; }
    const double t = ((double)(i - c.pre[lo]) * (L / (double)c.m[lo])) / L;
    sx = px + t * (c.x[lo + 1] - px);
    sy = py + t * (c.y[lo + 1] - py);
}

// sum and maximum over the samples of ring a of their least distance to the samples of ring b; `count`: the samples of a
__device__ void pm_directed(const PmRingRef& a, const PmRingRef& b, PmChunk& ca, PmChunk& cb, double2* tile, int* red_i, double* red_d, double& sum, double& mx,
                            double& count) {
    const int tid = threadIdx.x;
    double s = 0.0, m = 0.0;
    int64_t total = 0;
    for (int ea = 0; ea < a.n; ea += PM_EDGE_CHUNK) {
        pm_chunk_build(a, ea, ca, red_i);
        const int na = ca.total;
        total += na;
        for (int oa = 0; oa < na; oa += PM_TILE) {
            double ox[PM_OWN], oy[PM_OWN], best[PM_OWN];
#pragma unroll
            for (int k = 0; k < PM_OWN; ++k) {
                const int i = oa + k * PM_THREADS + tid;
                ox[k] = oy[k] = 0.0;
                best[k] = __longlong_as_double(0x7ff0000000000000ll);
                if (i < na) pm_sample(ca, i, ox[k], oy[k]);
            }
            const int live = (na - oa + PM_THREADS - 1) / PM_THREADS;          // owned slots any thread uses: uniform
            for (int eb = 0; eb < b.n; eb += PM_EDGE_CHUNK) {
                pm_chunk_build(b, eb, cb, red_i);
                const int nb = cb.total;
                for (int tb = 0; tb < nb; tb += PM_TILE) {
                    const int cnt = nb - tb < PM_TILE ? nb - tb : PM_TILE;
                    __syncthreads();          // the last tile has been read
                    for (int j = tid; j < cnt; j += PM_THREADS) {
                        double x, y;
                        pm_sample(cb, tb + j, x, y);
                        tile[j] = make_double2(x, y);
                    }
                    __syncthreads();
                    for (int j = 0; j < cnt; ++j) {
                        const double2 q = tile[j];
#pragma unroll
                        for (int k = 0; k < PM_OWN; ++k) {
                            if (k < live) {
                                const double dx = ox[k] - q.x, dy = oy[k] - q.y;
                                const double d2 = dx * dx + dy * dy;
                                best[k] = d2 < best[k] ? d2 : best[k];
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < PM_OWN; ++k) {
                if (oa + k * PM_THREADS + tid < na) {
                    const double d = __dsqrt_rn(best[k]);
                    s += d;
                    m = d > m ? d : m;
                }
            }
        }
    }
    double ts;
    wg_scan<false, double>(s, red_d, ts);
    sum = ts;
    mx = wg_max<double>(m, red_d);
    count = (double)total;
}

// sum over the vertices of a of the least distance to the edges of b (the closing one included; a zero-length edge is a point)
__device__ double pm_polis_side(const PmRingRef& a, const PmRingRef& b, double* red_d) {
    double s = 0.0;
    for (int i = threadIdx.x; i < a.n; i += PM_THREADS) {
        const double ax = pm_vx(a, i), ay = pm_vy(a, i);
        double best = __longlong_as_double(0x7ff0000000000000ll);
        double px = pm_vx(b, 0), py = pm_vy(b, 0);
        for (int e = 0; e < b.n; ++e) {
            const int j = e + 1 == b.n ? 0 : e + 1;
            const double qx = pm_vx(b, j), qy = pm_vy(b, j);
            const double vx = qx - px, vy = qy - py, wx = ax - px, wy = ay - py;
            const double den = vx * vx + vy * vy;
            double t = den > 0.0 ? (wx * vx + wy * vy) / den : 0.0;
            t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
            const double dx = ax - (px + t * vx), dy = ay - (py + t * vy);
            const double d2 = dx * dx + dy * dy;
            best = d2 < best ? d2 : best;
            px = qx; py = qy;
        }
        s += __dsqrt_rn(best);
    }
    double ts;
    wg_scan<false, double>(s, red_d, ts);
    return ts;
}

__global__ __launch_bounds__(PM_THREADS) void pm_pair_kernel(PmSet gt, PmSet dt, PmRings wg, PmRings wd, int modes, PmOut o) {
    __shared__ PmChunk ca, cb;
    __shared__ double2 tile[PM_TILE];
    __shared__ int red_i[PM_THREADS / 64];
    __shared__ double red_d[PM_THREADS / 64];
    const int g = blockIdx.x;
    const int d = o.match[g];
    if (d < 0) return;          // not counted: match -1 and the NaN of pm_ring_kernel stay
    const PmRingRef A = {gt.pos + wg.first[g], wg.n[g]}, Bp = {dt.pos + wd.first[d], wd.n[d]};
    if (modes & P3_PM_POLIS) {
        const double sa = pm_polis_side(A, Bp, red_d), sb = pm_polis_side(Bp, A, red_d);
        if (threadIdx.x == 0) o.pair_polis[g] = sa / (double)(2 * ((int64_t)A.n + 1)) + sb / (double)(2 * ((int64_t)Bp.n + 1));
    }
    if (modes & P3_PM_SAMPLES) {
        double s1, m1, n1, s2, m2, n2;
        pm_directed(A, Bp, ca, cb, tile, red_i, red_d, s1, m1, n1);
        pm_directed(Bp, A, ca, cb, tile, red_i, red_d, s2, m2, n2);
        if (threadIdx.x == 0) {
            o.pair_chamfer[g] = (s1 / n1 + s2 / n2) / 2.0;
            o.pair_hausdorff[g] = m1 > m2 ? m1 : m2;
        }
    }
}

// ---- per image, per set ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PM_THREADS) void pm_finish_kernel(PmSet gt, int B, int modes, PmOut o) {
    const double nan = pm_nan();
    for (int b = threadIdx.x; b < B; b += PM_THREADS) {
        const int g0 = pm_lower(gt.image, gt.R, b), g1 = pm_lower(gt.image, gt.R, b + 1);
        double sp = 0.0, sc = 0.0, sh = 0.0;
        int pairs = 0;
        for (int g = g0; g < g1; ++g) {          // the counted pairs in gt order
            if (o.match[g] < 0) continue;
            ++pairs;
            sp += o.pair_polis[g]; sc += o.pair_chamfer[g]; sh += o.pair_hausdorff[g];
        }
        o.image_valid[b] = pairs > 0;
        o.image_polis[b] = pairs > 0 ? sp / (double)pairs : nan;
        o.image_chamfer[b] = pairs > 0 ? sc / (double)pairs : nan;
        o.image_hausdorff[b] = pairs > 0 ? sh / (double)pairs : nan;
        if (modes & P3_PM_IOU) {
            const int I = o.image_counts[2 * b], U = o.image_counts[2 * b + 1];
            o.image_iou[b] = U == 0 ? 1.0 : (double)I / ((double)U + 1e-9);
        } else {
            o.image_iou[b] = o.image_nr[b] = nan;          // NR belongs to the IoU mode (compute_IoU_cIoU)
            o.image_counts[2 * b] = o.image_counts[2 * b + 1] = 0;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double iou = 0.0, ciou = 0.0, nr = 0.0, sp = 0.0, sc = 0.0, sh = 0.0;
    int valid = 0;
    for (int b = 0; b < B; ++b) {          // image order
        iou += o.image_iou[b];
        ciou += o.image_iou[b] * o.image_nr[b];
        nr += o.image_nr[b];
        if (!o.image_valid[b]) continue;
        ++valid;
        sp += o.image_polis[b]; sc += o.image_chamfer[b]; sh += o.image_hausdorff[b];
    }
    o.metrics[0] = iou / (double)B;
    o.metrics[1] = ciou / (double)B;
    o.metrics[2] = (modes & P3_PM_IOU) ? nr / (double)B : nan;
    o.metrics[3] = valid ? sp / (double)valid : nan;
    o.metrics[4] = valid ? sc / (double)valid : nan;
    o.metrics[5] = valid ? sh / (double)valid : nan;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------------------
struct PmWs { PmRings gt, dt; };
static PmWs pm_carve(int R_gt, int R_dt, P3Carve& c) {
    PmWs l;
    l.gt = pm_carve_set(R_gt, c);
    l.dt = pm_carve_set(R_dt, c);
    return l;
}

extern "C" int64_t p3_polygon_metrics_workspace_bytes(int R_gt, int R_dt, int B) {
    if (R_gt < 0 || R_dt < 0 || B < 1) return 0;
    P3Carve c = {nullptr, 0};
    pm_carve(R_gt, R_dt, c);
    return c.at;
}

extern "C" int p3_polygon_metrics(const float* gt_pos, int64_t V_gt, const int64_t* gt_slice, const int32_t* gt_image, int R_gt, const float* dt_pos, int64_t V_dt,
                                  const int64_t* dt_slice, const int32_t* dt_image, int R_dt, int B, int H, int W, int modes, double* metrics, double* image_iou,
                                  double* image_nr, double* image_polis, double* image_chamfer, double* image_hausdorff, int32_t* image_valid,
                                  int32_t* image_counts, int32_t* match, double* pair_polis, double* pair_chamfer, double* pair_hausdorff,
                                  int32_t* invalid_rings, int32_t* status, void* workspace, void* stream) {
    P3_CHECK(V_gt >= 0 && V_dt >= 0 && R_gt >= 0 && R_dt >= 0, P3_EINVAL, "p3_polygon_metrics: a negative count (V_gt, V_dt, R_gt, R_dt >= 0)");
    P3_CHECK(B >= 1 && H >= 1 && W >= 1, P3_EINVAL, "p3_polygon_metrics: bad sizes (B, H, W >= 1)");
    P3_CHECK((int64_t)H * W <= PM_MAX_HW, P3_EINVAL, "p3_polygon_metrics: H W above 2^18 (both masks of an image are held in LDS)");
    P3_CHECK((int64_t)R_gt + R_dt < ((int64_t)1 << 31) - PM_THREADS, P3_EINVAL, "p3_polygon_metrics: R_gt + R_dt must stay below 2^31 - 256");
    P3_CHECK(modes > 0 && (modes & ~(P3_PM_IOU | P3_PM_POLIS | P3_PM_SAMPLES)) == 0, P3_EINVAL, "p3_polygon_metrics: modes is a non-empty set of P3_PM_* bits");
    P3_CHECK(metrics && image_iou && image_nr && image_polis && image_chamfer && image_hausdorff && image_valid && image_counts && invalid_rings && status,
             P3_EINVAL, "p3_polygon_metrics: null pointer (metrics, image_*, invalid_rings, status)");
    P3_CHECK(R_gt == 0 || (gt_pos && gt_slice && gt_image && match && pair_polis && pair_chamfer && pair_hausdorff), P3_EINVAL,
             "p3_polygon_metrics: null pointer (gt_pos, gt_slice, gt_image, match, pair_*)");
    P3_CHECK(R_dt == 0 || (dt_pos && dt_slice && dt_image), P3_EINVAL, "p3_polygon_metrics: null pointer (dt_pos, dt_slice, dt_image)");
    P3_CHECK((R_gt == 0 || !(p3_host_array(gt_slice) || p3_host_array(gt_image))) && (R_dt == 0 || !(p3_host_array(dt_slice) || p3_host_array(dt_image))),
             P3_EINVAL, "p3_polygon_metrics: ring_slice and ring_image must be device memory");
    const int64_t need = p3_polygon_metrics_workspace_bytes(R_gt, R_dt, B);
    P3_CHECK(need == 0 || workspace, P3_EINVAL, "p3_polygon_metrics: null workspace (p3_polygon_metrics_workspace_bytes(R_gt, R_dt, B))");
    hipStream_t s = (hipStream_t)stream;
    P3Carve carve = {(char*)workspace, 0};
    const PmWs l = pm_carve(R_gt, R_dt, carve);
    const PmSet gt = {(const float2*)gt_pos, gt_slice, gt_image, V_gt, R_gt}, dt = {(const float2*)dt_pos, dt_slice, dt_image, V_dt, R_dt};
    const PmOut o = {metrics, image_iou, image_nr, image_polis, image_chamfer, image_hausdorff, image_valid, image_counts, match, pair_polis, pair_chamfer,
                     pair_hausdorff, invalid_rings, status};
    P3_TRY(p3_memset(status, 0, sizeof(int32_t), s));
    if (R_gt + R_dt > 0) P3_TRY(p3_launch<pm_ring_kernel>(nullptr, p3_ceil_div((int64_t)R_gt + R_dt, PM_THREADS), PM_THREADS, 0, s, gt, dt, l.gt, l.dt, B, o));
    if (modes & P3_PM_IOU) {
        const int words = (H * W + 31) >> 5;
        const size_t lds = (size_t)(2 * words) * sizeof(uint32_t) + PM_EDGE_CHUNK * sizeof(PmEdge);
        P3_TRY(p3_launch<pm_raster_kernel>("pm_raster_kernel", B, PM_THREADS, lds, s, gt, dt, l.gt, l.dt, H, W, o));
    }
    P3_TRY(p3_launch<pm_match_kernel>(nullptr, B, PM_THREADS, 0, s, gt, dt, l.gt, l.dt, o));
    if (R_gt > 0 && R_dt > 0 && (modes & (P3_PM_POLIS | P3_PM_SAMPLES)))
        P3_TRY(p3_launch<pm_pair_kernel>("pm_pair_kernel", R_gt, PM_THREADS, 0, s, gt, dt, l.gt, l.dt, modes, o));
    P3_TRY(p3_launch<pm_finish_kernel>(nullptr, 1, PM_THREADS, 0, s, gt, B, modes, o));
    return P3_OK;
}
