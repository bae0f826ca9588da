// p3hip — max tangent angle error (MTA) of a predicted ring set against a ground-truth ring set (gfx950): the contour measure of the reference's
// eval/angle_eval.py, from the packed rings to the mean angle on the device.  include/p3hip.h (p3_max_tangent_angle) and DESIGN.md section 23 hold the definition.
//   mta_ring_kernel      one thread per ring of either set: validity, box (pm_rings.h); every prediction starts as state 1 with NaN figures and (0, 0) pixels
//   mta_mask_kernel      one workgroup of 16 waves per image: the gt union mask and the union of the prediction masks bit-packed in LDS (2 x H W / 8 bytes, at
//                        most 64 KB, and 128 bytes for the sums); a wave per ring: first the gt rings into their mask, then per valid prediction its own parity inside its pixel box
//                        against the gt mask for (A, I) and its state (empty, below precision, kept); the overlap report; invalid_rings
//   mta_project_kernel   one workgroup per prediction ring, the kept ones work: samples from per-edge counts prefix-summed in LDS 32 edges at a time, tiles
//                        of PM_THREADS samples that overlap by one, the image's gt edges streamed through LDS 32 at a time across ring boundaries, the
//                        projected points in LDS, thread k folds the edge (k, k + 1); the least cosine per workgroup
//   mta_finish_kernel    one workgroup: the counted angles in degrees summed in ring order, the mean
// Every floating-point value is a double made of the fp32 coordinates; contraction is off for the whole file, so that a product and the sum behind it round as
// the float64 restatement (tests/mta_ref.py) rounds them: sample counts, crossings and the nearest edge are then the restatement's.
// MtaChunk / mta_chunk_build follow the shape of poly_metrics.hip's PmChunk / pm_chunk_build (stage 32 edges, scan their counts, two barriers) but share no
// code with them: the count rule (rint of L / spacing against ceil of L / 0.1), the 64-bit prefix with a carry across chunks, the missing closing sample and
// the interpolation (j ((q - p) / m), the end point exact) all differ, so a shared routine would have meant changing the existing kernel.
#include "pm_rings.h"          // the ring set, ring validity and the crossing rule

#pragma clang fp contract(off)

constexpr int MTA_EDGES = PM_THREADS - 1;          // edges a tile of PM_THREADS samples forms: the tiles overlap by one sample
constexpr int MTA_MASK_THREADS = 1024;             // sixteen waves of an image's workgroup raster sixteen rings at a time
constexpr double MTA_MIN_SPACING = 0.015625;       // 1 / 64: with coordinates within 2^15 an edge has fewer than 2^23 samples, and a kernel cannot be made to walk for minutes

struct MtaOut {
    double* mta;
    int32_t* counted;
    double* ring_angle;
    double* ring_cos;
    int32_t* ring_state;
    int32_t* ring_px;               // [R_dt, 2] = (A, I)
    int32_t* image_overlap_px;
    int32_t* invalid_rings;         // [B, 2] = (gt, prediction)
    int32_t* status;
};

// ---- rings ----------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PM_THREADS) void mta_ring_kernel(PmSet gt, PmSet dt, PmRings wg, PmRings wd, int B, MtaOut o) {
    const int r = blockIdx.x * PM_THREADS + threadIdx.x;
    if (r < gt.R) {
        pm_ring(gt, wg, r, B, o.status);
    } else if (r - gt.R < dt.R) {
        const int d = r - gt.R;
        pm_ring(dt, wd, d, B, o.status);
        o.ring_angle[d] = o.ring_cos[d] = pm_nan();
        o.ring_state[d] = P3_MTA_INVALID;
        o.ring_px[2 * d] = o.ring_px[2 * d + 1] = 0;
    }
}

// ---- masks, precision, overlap --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mta_wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the parity of valid ring r inside its pixel box, by one wave: a lane per (row, word) unit, the edges read where they lie (every lane reads the same vertex);
// f(word, parity) for every unit with a pixel inside.  The bits of a word that two rows share are disjoint.  No barrier: the waves of a workgroup take
// different rings.
template <class F>
__device__ __forceinline__ void mta_wave_raster(const PmSet& s, const PmRings& w, int r, int H, int W, F&& f) {
    const int lane = threadIdx.x & 63;
    const int n = w.n[r];
    const float2* v = s.pos + w.first[r];
    int r0, r1, c0, c1;          // rows and columns whose centres can lie inside
    if (!pm_pixel_box(w.box + 4 * (int64_t)r, H, W, r0, r1, c0, c1)) return;
    const int per_row = ((c1 - c0) >> 5) + 2;          // words a row's [c0, c1] can touch
    const int units = (r1 - r0 + 1) * per_row;
    for (int u = lane; u < units; u += 64) {
        const int row = r0 + u / per_row;
        const int bit0 = row * W + c0, bit1 = row * W + c1;          // H W <= 2^18: no overflow
        const int word = (bit0 >> 5) + u % per_row;
        if (word > (bit1 >> 5)) continue;
        const int lo = bit0 > (word << 5) ? bit0 : (word << 5), hi = bit1 < (word << 5) + 31 ? bit1 : (word << 5) + 31;
        const double py = (double)row + 0.5;
        uint32_t parity = 0;
        float2 pa = v[0];
        for (int e = 0; e < n; ++e) {
            const float2 pb = v[e + 1 == n ? 0 : e + 1];
            const PmEdge ed = {(double)pa.x, (double)pa.y, (double)pb.x, (double)pb.y};
            pa = pb;
            if (!pm_crossed(ed, py)) continue;          // not crossed by this row's centres
            const double ex = ed.bx - ed.ax, ey = ed.by - ed.ay, wy = py - ed.ay;
            const double t1 = ex * wy;
            for (int bit = lo; bit <= hi; ++bit) {
                const double px = (double)(bit - row * W) + 0.5;
                if (pm_right_of(ed, t1, ey, px)) parity ^= 1u << (bit & 31);
            }
        }
        if (parity) f(word, parity);
    }
}

__global__ __launch_bounds__(MTA_MASK_THREADS) void mta_mask_kernel(PmSet gt, PmSet dt, PmRings wg, PmRings wd, int H, int W, double min_precision, MtaOut o) {
    extern __shared__ __attribute__((aligned(16))) uint32_t mta_lds[];          // all of the kernel's LDS, so that the launch states the whole of it: 128 bytes more than 64 KB at the largest image
    unsigned long long* red = (unsigned long long*)mta_lds;          // one per wave, for wg_scan
    uint32_t* masks = mta_lds + 2 * (MTA_MASK_THREADS / 64);
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int words = (H * W + 31) >> 5;
    uint32_t* mg = masks;                     // the union of the valid gt rings
    uint32_t* md = masks + words;             // the union of the valid predictions
    for (int i = tid; i < 2 * words; i += MTA_MASK_THREADS) masks[i] = 0;
    __syncthreads();
    const int g_lo = pm_lower(gt.image, gt.R, b), g_hi = pm_lower(gt.image, gt.R, b + 1);
    const int d_lo = pm_lower(dt.image, dt.R, b), d_hi = pm_lower(dt.image, dt.R, b + 1);
    for (int g = g_lo + wave; g < g_hi; g += MTA_MASK_THREADS / 64)          // a wave per ring
        if (wg.state[g] == 1) mta_wave_raster(gt, wg, g, H, W, [&](int word, uint32_t parity) { atomicOr(mg + word, parity); });
    __syncthreads();          // the gt mask is complete
    unsigned long long sum_a = 0;          // over this wave's predictions
    for (int d = d_lo + wave; d < d_hi; d += MTA_MASK_THREADS / 64) {
        if (wd.state[d] != 1) continue;          // uniform over the wave
        uint32_t a = 0, in = 0;
        mta_wave_raster(dt, wd, d, H, W, [&](int word, uint32_t parity) {
            a += __popc(parity);
            in += __popc(parity & mg[word]);
            atomicOr(md + word, parity);
        });
        const int A = (int)mta_wave_sum(a), I = (int)mta_wave_sum(in);
        sum_a += (unsigned long long)A;
        if (lane == 0) {
            o.ring_px[2 * d] = A;
            o.ring_px[2 * d + 1] = I;
            o.ring_state[d] = A == 0 ? P3_MTA_EMPTY : ((double)I / (double)A > min_precision ? P3_MTA_COUNTED : P3_MTA_BELOW_PRECISION);
        }
    }
    __syncthreads();          // the union of the predictions is complete
    uint32_t nu = 0, bad_g = 0, bad_d = 0;
    for (int i = tid; i < words; i += MTA_MASK_THREADS) nu += __popc(md[i]);
    for (int g = g_lo + tid; g < g_hi; g += MTA_MASK_THREADS) bad_g += wg.state[g] == 0;
    for (int d = d_lo + tid; d < d_hi; d += MTA_MASK_THREADS) bad_d += wd.state[d] == 0;
    unsigned long long ta, tu, tb;
    wg_scan<false, unsigned long long>(lane == 0 ? sum_a : 0ull, red, ta);
    wg_scan<false, unsigned long long>((unsigned long long)nu, red, tu);
    wg_scan<false, unsigned long long>(p3_pack2(bad_g, bad_d), red, tb);
    if (tid == 0) {
        const int32_t overlap = p3_sat31((int64_t)(ta - tu));
        o.image_overlap_px[b] = overlap;
        if (overlap != 0) atomicOr(o.status, 4);
        o.invalid_rings[2 * b] = p3_hi32(tb);
        o.invalid_rings[2 * b + 1] = p3_lo32(tb);
    }
}

// ---- samples, projection, the least cosine --------------------------------------------------------------------------------------------------------------
// one chunk of the prediction's edges in LDS: end points, sample counts and their exclusive prefix inside the chunk
struct MtaChunk {
    double x[PM_EDGE_CHUNK + 1], y[PM_EDGE_CHUNK + 1];
    unsigned long long pre[PM_EDGE_CHUNK + 1];
    int m[PM_EDGE_CHUNK];
    int cnt;
};

// every thread of the workgroup calls it; ends on a barrier
__device__ void mta_chunk_build(const float2* v, int n, int e0, double spacing, MtaChunk& c, unsigned long long* red) {
    const int tid = threadIdx.x;
    const int cnt = n - e0 < PM_EDGE_CHUNK ? n - e0 : PM_EDGE_CHUNK;
    __syncthreads();          // the chunk's last readers are done
    unsigned long long m = 0;
    if (tid < cnt) {
        const int i = e0 + tid, j = i + 1 == n ? 0 : i + 1;
        const double px = (double)v[i].x, py = (double)v[i].y, qx = (double)v[j].x, qy = (double)v[j].y;
        const double dx = qx - px, dy = qy - py;
        const double L = __dsqrt_rn(dx * dx + dy * dy);
        const double k = rint(L / spacing);          // half to even
        m = k > 1.0 ? (unsigned long long)k : 1;          // L / spacing <= 2^16 sqrt(2) 64: far inside int32
        c.x[tid] = px; c.y[tid] = py; c.m[tid] = (int)m;
        if (tid == cnt - 1) { c.x[cnt] = qx; c.y[cnt] = qy; }
    }
    unsigned long long tot;
    const unsigned long long incl = wg_scan<false, unsigned long long>(m, red, tot);
    if (tid < cnt) c.pre[tid] = incl - m;
    if (tid == 0) {
        c.cnt = cnt;
        c.pre[cnt] = tot;
    }
    __syncthreads();
}

// sample li of the chunk, 1 <= li <= c.pre[c.cnt]: point j = li - pre[e] of the edge e with pre[e] < li <= pre[e + 1]; point m is the end point itself
__device__ __forceinline__ void mta_sample(const MtaChunk& c, unsigned long long li, double& sx, double& sy) {
    int lo = 0, hi = c.cnt - 1;          // the last edge whose prefix is < li
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (c.pre[mid] < li) lo = mid;
        else hi = mid - 1;
    }
    const int j = (int)(li - c.pre[lo]), m = c.m[lo];
    const double px = c.x[lo], py = c.y[lo], qx = c.x[lo + 1], qy = c.y[lo + 1];
    if (j == m) { sx = qx; sy = qy; return; }
    sx = px + (double)j * ((qx - px) / (double)m);
    sy = py + (double)j * ((qy - py) / (double)m);
}

// a position in the valid gt edges of an image, rings in set order: edge `e` of ring `g`; g == g_hi: behind the last edge
struct MtaCursor { int g, e; };
// k edges further; `passed`: the edges there were, when fewer than k
__device__ __forceinline__ MtaCursor mta_advance(const PmRings& wg, int g_hi, MtaCursor c, int k, int& passed) {
    int left = k;
    while (c.g < g_hi) {
        const int avail = (wg.state[c.g] == 1 ? wg.n[c.g] : 0) - c.e;
        if (left < avail) { c.e += left; passed = k; return c; }
        left -= avail;
        ++c.g;
        c.e = 0;
    }
    passed = k - left;
    return c;
}

__global__ __launch_bounds__(PM_THREADS) void mta_project_kernel(PmSet gt, PmSet dt, PmRings wg, PmRings wd, double spacing, double max_stretch, MtaOut o) {
    __shared__ MtaChunk chunk;
    __shared__ PmEdge edges[PM_EDGE_CHUNK];
    __shared__ double2 samp[PM_THREADS], proj[PM_THREADS];
    __shared__ unsigned long long red_u[PM_THREADS / 64];
    __shared__ double red_d[PM_THREADS / 64];
    const int d = blockIdx.x, tid = threadIdx.x;
    if (o.ring_state[d] != P3_MTA_COUNTED) return;          // uniform; only mta_mask_kernel's kept rings go on
    const int n = wd.n[d];
    const float2* v = dt.pos + wd.first[d];
    const int b = dt.image[d];
    const int g_lo = pm_lower(gt.image, gt.R, b), g_hi = pm_lower(gt.image, gt.R, b + 1);
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    const double lo_stretch = 1.0 / max_stretch;
    double neg_cos = -inf;          // the greatest -c of this thread's valid edges
    int e_first = 0;                // the chunk that holds the tile's first sample, and the samples on the edges in front of it
    unsigned long long carry_first = 0;
    for (unsigned long long base = 0;; base += MTA_EDGES) {          // the tile: samples base .. base + 255 of the line; sample 0 is vertex 0
        const unsigned long long i = base + tid, next = base + MTA_EDGES;
        double sx = 0.0, sy = 0.0;
        bool have = false;
        int e0 = e_first, e_next = -1;
        unsigned long long carry = carry_first, end = 0, carry_next = 0;
        bool more;          // the ring has edges behind the chunks this tile has seen
        for (;;) {
            mta_chunk_build(v, n, e0, spacing, chunk, red_u);
            end = carry + chunk.pre[chunk.cnt];
            if (!have) {
                if (i == 0) { sx = chunk.x[0]; sy = chunk.y[0]; have = true; }          // base == 0: the chunk starts at edge 0
                else if (i > carry && i <= end) { mta_sample(chunk, i - carry, sx, sy); have = true; }
            }
            if (next > carry && next <= end) { e_next = e0; carry_next = carry; }
            more = e0 + chunk.cnt < n;
            if (end >= next || !more) break;
            carry = end;
            e0 += chunk.cnt;
        }
        // the nearest point on the gt edges of the image, the first edge with the strictly smallest squared distance
        double best = inf, bx = 0.0, by = 0.0;
        MtaCursor cur = {g_lo, 0};
        for (;;) {
            int cnt, mine;
            const MtaCursor at = mta_advance(wg, g_hi, cur, tid < PM_EDGE_CHUNK ? tid : 0, mine);
            cur = mta_advance(wg, g_hi, cur, PM_EDGE_CHUNK, cnt);          // uniform
            if (cnt == 0) break;
            __syncthreads();          // the last chunk has been read
            if (tid < cnt) {
                const int ng = wg.n[at.g], j = at.e + 1 == ng ? 0 : at.e + 1;
                const float2 pa = gt.pos[wg.first[at.g] + at.e], pb = gt.pos[wg.first[at.g] + j];
                edges[tid] = {(double)pa.x, (double)pa.y, (double)pb.x, (double)pb.y};
            }
            __syncthreads();
            if (!have) continue;
            for (int k = 0; k < cnt; ++k) {
                const PmEdge ed = edges[k];
                const double ex = ed.bx - ed.ax, ey = ed.by - ed.ay, wx = sx - ed.ax, wy = sy - ed.ay;
                const double den = ex * ex + ey * ey;
                const double t = (wx * ex + wy * ey) / den;
                double cx = ed.ax + t * ex, cy = ed.ay + t * ey;
                if (!(den > 0.0) || t <= 0.0) { cx = ed.ax; cy = ed.ay; }
                else if (t >= 1.0) { cx = ed.bx; cy = ed.by; }
                const double dx = sx - cx, dy = sy - cy;
                const double e = dx * dx + dy * dy;
                if (e < best) { best = e; bx = cx; by = cy; }
            }
        }
        __syncthreads();          // the last tile's samples and points have been read
        samp[tid] = make_double2(sx, sy);
        proj[tid] = make_double2(bx, by);
        __syncthreads();
        if (tid < MTA_EDGES && i + 1 <= end) {          // samples up to `end` exist, so sample i + 1 is in this tile
            const double2 s0 = samp[tid], s1 = samp[tid + 1], p0 = proj[tid], p1 = proj[tid + 1];
            const double ux = s1.x - s0.x, uy = s1.y - s0.y, vx = p1.x - p0.x, vy = p1.y - p0.y;
            const double nu = __dsqrt_rn(ux * ux + uy * uy), nv = __dsqrt_rn(vx * vx + vy * vy);
            const double nn = nu * nv;
            if (nn > 0.0) {
                const double stretch = nu / nv;
                if (lo_stretch < stretch && stretch < max_stretch) {
                    const double c = fabs((ux * vx + uy * vy) / nn);
                    neg_cos = -c > neg_cos ? -c : neg_cos;
                }
            }
        }
        if (!(end > next || more)) break;          // no sample behind `next`, the last one this tile has seen
        e_first = e_next;
        carry_first = carry_next;
    }
    const double top = wg_max<double>(neg_cos, red_d);
    if (tid != 0) return;
    if (!(top > -inf)) {
        o.ring_state[d] = P3_MTA_NO_EDGE;
        return;
    }
    const double c = -top;
    o.ring_cos[d] = c;
    o.ring_angle[d] = acos(c < 1.0 ? c : 1.0);
}

// ---- the mean -------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PM_THREADS) void mta_finish_kernel(int R_dt, MtaOut o) {
    __shared__ double deg[PM_THREADS];
    __shared__ int red[PM_THREADS / 64];
    const int tid = threadIdx.x;
    double sum = 0.0;          // thread 0's
    int mine = 0;
    for (int base = 0; base < R_dt; base += PM_THREADS) {
        const int r = base + tid;
        const bool counted = r < R_dt && o.ring_state[r] == P3_MTA_COUNTED;
        deg[tid] = counted ? o.ring_angle[r] * 180.0 / 3.141592653589793 : 0.0;          // + 0.0 leaves a sum that is never -0.0 as it is
        mine += counted;
        __syncthreads();
        if (tid == 0) {
            const int cnt = R_dt - base < PM_THREADS ? R_dt - base : PM_THREADS;
            for (int k = 0; k < cnt; ++k) sum += deg[k];          // ring order
        }
        __syncthreads();
    }
    int counted;
    wg_scan<false, int>(mine, red, counted);
    if (tid == 0) {
        *o.counted = counted;
        *o.mta = counted ? sum / (double)counted : pm_nan();
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------------------
struct MtaWs { PmRings gt, dt; };
static MtaWs mta_carve(int R_gt, int R_dt, P3Carve& c) {
    MtaWs l;
    l.gt = pm_carve_set(R_gt, c);
    l.dt = pm_carve_set(R_dt, c);
    return l;
}

extern "C" int64_t p3_max_tangent_angle_workspace_bytes(int R_gt, int R_dt, int B) {
    if (R_gt < 0 || R_dt < 0 || B < 1) return 0;
    P3Carve c = {nullptr, 0};
    mta_carve(R_gt, R_dt, c);
    return c.at;
}

extern "C" int p3_max_tangent_angle(const float* gt_pos, int64_t V_gt, const int64_t* gt_slice, const int32_t* gt_image, int R_gt, const float* dt_pos,
                                    int64_t V_dt, const int64_t* dt_slice, const int32_t* dt_image, int R_dt, int B, int H, int W, double sampling_spacing,
                                    double min_precision, double max_stretch, double* mta, int32_t* counted, double* ring_angle, double* ring_cos,
                                    int32_t* ring_state, int32_t* ring_px, int32_t* image_overlap_px, int32_t* invalid_rings, int32_t* status, void* workspace,
                                    void* stream) {
    P3_CHECK(V_gt >= 0 && V_dt >= 0 && R_gt >= 0 && R_dt >= 0, P3_EINVAL, "p3_max_tangent_angle: a negative count (V_gt, V_dt, R_gt, R_dt >= 0)");
    P3_CHECK(B >= 1 && H >= 1 && W >= 1, P3_EINVAL, "p3_max_tangent_angle: bad sizes (B, H, W >= 1)");
    P3_CHECK((int64_t)H * W <= PM_MAX_HW, P3_EINVAL, "p3_max_tangent_angle: H W above 2^18 (the bound of p3_polygon_metrics: two masks of an image are held in LDS)");
    P3_CHECK((int64_t)R_gt + R_dt < ((int64_t)1 << 31) - PM_THREADS, P3_EINVAL, "p3_max_tangent_angle: R_gt + R_dt must stay below 2^31 - 256");
    P3_CHECK(sampling_spacing > 0.0 && sampling_spacing <= 1.7976931348623157e308, P3_EINVAL,
             "p3_max_tangent_angle: sampling_spacing must be finite and > 0");
    P3_CHECK(sampling_spacing >= MTA_MIN_SPACING, P3_EINVAL, "p3_max_tangent_angle: sampling_spacing below 1 / 64 (the samples of a ring are bounded)");
    P3_CHECK(min_precision >= 0.0 && min_precision < 1.0, P3_EINVAL, "p3_max_tangent_angle: min_precision must lie in [0, 1)");
    P3_CHECK(max_stretch > 1.0 && max_stretch <= 1.7976931348623157e308, P3_EINVAL, "p3_max_tangent_angle: max_stretch must be finite and > 1");
    P3_CHECK(mta && counted && image_overlap_px && invalid_rings && status, P3_EINVAL,
             "p3_max_tangent_angle: null pointer (mta, counted, image_overlap_px, invalid_rings, status)");
    P3_CHECK(R_gt == 0 || (gt_pos && gt_slice && gt_image), P3_EINVAL, "p3_max_tangent_angle: null pointer (gt_pos, gt_slice, gt_image)");
    P3_CHECK(R_dt == 0 || (dt_pos && dt_slice && dt_image && ring_angle && ring_cos && ring_state && ring_px), P3_EINVAL,
             "p3_max_tangent_angle: null pointer (dt_pos, dt_slice, dt_image, ring_angle, ring_cos, ring_state, ring_px)");
    P3_CHECK((R_gt == 0 || !(p3_host_array(gt_slice) || p3_host_array(gt_image))) && (R_dt == 0 || !(p3_host_array(dt_slice) || p3_host_array(dt_image))),
             P3_EINVAL, "p3_max_tangent_angle: ring_slice and ring_image must be device memory");
    const int64_t need = p3_max_tangent_angle_workspace_bytes(R_gt, R_dt, B);
    P3_CHECK(need == 0 || workspace, P3_EINVAL, "p3_max_tangent_angle: null workspace (p3_max_tangent_angle_workspace_bytes(R_gt, R_dt, B))");
    hipStream_t s = (hipStream_t)stream;
    P3Carve carve = {(char*)workspace, 0};
    const MtaWs l = mta_carve(R_gt, R_dt, carve);
    const PmSet gt = {(const float2*)gt_pos, gt_slice, gt_image, V_gt, R_gt}, dt = {(const float2*)dt_pos, dt_slice, dt_image, V_dt, R_dt};
    const MtaOut o = {mta, counted, ring_angle, ring_cos, ring_state, ring_px, image_overlap_px, invalid_rings, status};
    P3_TRY(p3_memset(status, 0, sizeof(int32_t), s));
    if (R_gt + R_dt > 0) P3_TRY(p3_launch<mta_ring_kernel>(nullptr, p3_ceil_div((int64_t)R_gt + R_dt, PM_THREADS), PM_THREADS, 0, s, gt, dt, l.gt, l.dt, B, o));
    const size_t lds = (size_t)(2 * ((H * W + 31) >> 5)) * sizeof(uint32_t) + (MTA_MASK_THREADS / 64) * sizeof(unsigned long long);
    P3_TRY(p3_launch<mta_mask_kernel>("mta_mask_kernel", B, MTA_MASK_THREADS, lds, s, gt, dt, l.gt, l.dt, H, W, min_precision, o));
    if (R_dt > 0) P3_TRY(p3_launch<mta_project_kernel>("mta_project_kernel", R_dt, PM_THREADS, 0, s, gt, dt, l.gt, l.dt, sampling_spacing, max_stretch, o));
    P3_TRY(p3_launch<mta_finish_kernel>(nullptr, 1, PM_THREADS, 0, s, R_dt, o));
    return P3_OK;
}
