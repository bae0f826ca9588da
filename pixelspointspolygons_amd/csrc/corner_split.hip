// p3hip - FFL corner-aware contour simplification, the array half of `post_process` (predict/ffl/polygonize_acm.py:277-284, polygonize_asm.py:498-504:
// skimage approximate_polygon, frame_field_utils.detect_corners :71-114 on math_utils.compute_crossfield_uv, polygonize_utils.split_polylines_corner :47-61,
// LineString.simplify per piece) on the device.
//   p3_corner_split   optimised contours / skeleton paths + frame field -> the few-vertex polylines that go into shapely's unary_union.
//
// Polylines never interact: one workgroup per polyline, its explicit points (the first one appended again when `closed`) and all working arrays in LDS.
//   A  DP(explicit points, tol_pre)                                      Douglas-Peucker, level-synchronous (cs_dp)
//   B  corner mask of the survivors, u and v of the frame field computed at the survivors' pixels only
//   C  the pieces are the runs between consecutive corners.  The merged piece polyline[last corner:] + polyline[:first corner + 1] makes the sequence
//      wrap, so the survivors are read ROTATED to start at the first corner (v -> survivor (v + rot) mod m, V = m + 1 entries, the first corner twice):
//      every piece, the merged one last, is then a run between two boundaries of one linear sequence, in the order split_polylines_corner emits them
//   D  DP over that sequence with the boundaries kept from the start: all pieces of the polyline are simplified together
// cs_dp: every live point knows its section (s, e), the kept points around it.  A round is
//   1  d = distance to the section; atomicMax of d's bits (non-negative doubles order like their bits) on the section's key
//   2  a point whose d is the section's maximum and > tol: atomicMin of its index - the lowest index among equal maxima whatever the thread order
//   3  the winner becomes kept and the others move one of their ends onto it; a section without a winner dies (its points are dropped)
// until no section split: the recursion depth of Douglas-Peucker in rounds (up to n for a staircase), all inside the kernel.
// The same device function runs polylines over CS_LDS_CAP points (or all, when forced) with the arrays in the global workspace, one workgroup each.
// Distances and the frame field are evaluated in double with contraction off; every decision is a comparison, every output an index or a bit copy of an
// input position: two runs, either form, alone or inside a batch give the same bits.
// Launches: cs_offsets (scan of the explicit lengths), cs_lds / cs_global (A - D into a per-polyline staging area), cs_scan (scan of the polylines' vertex and
// piece counts, totals, status), cs_emit (compaction into the outputs, nothing past the capacities).  No host synchronisation.
#include "p3_common.h"

#pragma clang fp contract(off)

#define CS_THREADS 256
#define CS_SCAN_THREADS 1024
#define CS_LDS_CAP 4096           // explicit points of a polyline that run in LDS: the cap of ACM_LDS_CAP / ASM_LDS_CAP, so that what the optimisers ran in one
                                  // launch is post-processed in one launch.  31 B per point = 124 KiB of the CU's 160 KiB: one workgroup per CU, and a batch has
                                  // about as many polylines as the device has CUs
#define CS_PAD 8                  // the rotated sequence of stage D has one entry more than the polyline has survivors
#define CS_NONE 0xffffffffu
enum { CS_KEPT = 1, CS_DEAD = 2, CS_BND = 4 };          // state of a sequence entry; 0 = live (undecided)

struct CsIn {
    const float2* pos; const int64_t* index; const int64_t* slice; const uint8_t* closed; const int32_t* poly_batch; const float* c0c2;
    int64_t N, K, E;          // positions, index entries (0 without index), capacity of explicit points
    int P, B, H, W;
    double tol_pre, tol;
};
struct CsWork {               // per polyline, LDS or workspace
    float2* pt;               // [n] explicit points
    uint32_t* idx;            // [n] survivor of stage A -> explicit point
    uint32_t* se;             // [n + 1][2] live entry: its section's kept ends (s, e); kept entry: [0] = the winner of the section that starts there
    unsigned long long* key;  // [n + 1] kept entry: bits of the largest distance in the section that starts there
    uint8_t* state;           // [n + 1]
    uint8_t* mask;            // [n] corner mask of the survivors
    uint8_t* fl;              // [n] stage flags of the explicit points
};

// the clamped source range of polyline i: explicit point k is source entry s0 + (k < len ? k : k - len)
__device__ __forceinline__ void cs_range(const CsIn& in, int i, int64_t& s0, int& len, int& n) {
    const int64_t L = in.index ? in.K : in.N;
    int64_t a = in.slice[2 * (int64_t)i], b = in.slice[2 * (int64_t)i + 1];
    a = a < 0 ? 0 : (a > L ? L : a);
    b = b < a ? a : (b > L ? L : b);
    const int64_t l = b - a > 0x3fffffff ? 0x3fffffff : b - a;
    s0 = a; len = (int)l;
    n = len + ((in.closed[i] && len > 0) ? 1 : 0);
}
__device__ __forceinline__ float2 cs_point(const CsIn& in, int64_t s0, int len, int k) {
    int64_t a = s0 + (k < len ? k : k - len);
    if (in.index) { a = in.index[a]; a = a < 0 ? 0 : (a > in.N - 1 ? in.N - 1 : a); }
    return in.pos[a];
}

// point-to-segment distance of k to (s, e): perpendicular where k projects inside the segment, else to the nearer end (covers s == e)
__device__ __forceinline__ double cs_dist(float2 k, float2 s, float2 e) {
    const double dr = (double)e.x - (double)s.x, dc = (double)e.y - (double)s.y;
    const double ar = (double)k.x - (double)s.x, ac = (double)k.y - (double)s.y;
    const double br = (double)e.x - (double)k.x, bc = (double)e.y - (double)k.y;
    if (ar * dr + ac * dc > 0.0 && br * dr + bc * dc > 0.0) return fabs(ar * dc - ac * dr) / sqrt(dr * dr + dc * dc);
    const double da = sqrt(ar * ar + ac * ac), db = sqrt(br * br + bc * bc);
    return da < db ? da : db;
}

// principal square root of x + i y
__device__ __forceinline__ void cs_csqrt(double x, double y, double& re, double& im) {
    if (x == 0.0 && y == 0.0) { re = 0.0; im = y; return; }
    const double t = sqrt((fabs(x) + sqrt(x * x + y * y)) * 0.5);
    if (x >= 0.0) { re = t; im = y / (2.0 * t); }
    else { re = fabs(y) / (2.0 * t); im = copysign(t, y); }
}

// detect_corners' compute_is_corner for one vertex p with its left and right edges
__device__ __forceinline__ bool cs_corner(const CsIn& in, const float* cf, float2 p, double lr, double lc, double rr, double rc) {
    const double pr = fmin(fmax(rint((double)p.x), 0.0), (double)(in.H - 1)), pc = fmin(fmax(rint((double)p.y), 0.0), (double)(in.W - 1));          // NaN lands on 0
    const int64_t hw = (int64_t)in.H * in.W;
    const float* q = cf + (int64_t)pr * in.W + (int64_t)pc;
    const double c0r = q[0], c0i = q[hw], c2r = q[2 * hw], c2i = q[3 * hw];
    double sr, si, ur, ui, vr, vi;
    cs_csqrt(c2r * c2r - c2i * c2i - 4.0 * c0r, 2.0 * c2r * c2i - 4.0 * c0i, sr, si);
    cs_csqrt((c2r + sr) / 2.0, (c2i + si) / 2.0, ur, ui);
    cs_csqrt((c2r - sr) / 2.0, (c2i - si) / 2.0, vr, vi);
    const bool left_is_u = fabs(lr * vr + lc * vi) < fabs(lr * ur + lc * ui);
    const bool right_is_u = fabs(rr * vr + rc * vi) < fabs(rr * ur + rc * ui);
    return left_is_u != right_is_u;
}

// Douglas-Peucker over the sequence entry v -> pt[idx[(v + rot) mod m]], v < V.  The caller set state[] (kept, dead or live) and the section of every live entry.
__device__ __forceinline__ void cs_dp(const CsWork& w, int V, int m, int rot, double tol) {
#define CS_PT(v) w.pt[w.idx[(v) + rot >= m ? (v) + rot - m : (v) + rot]]
    for (int round = 0; round < V; ++round) {          // every round but the last keeps a point
        for (int v = threadIdx.x; v < V; v += CS_THREADS)
            if (w.state[v] & CS_KEPT) { w.key[v] = 0ull; w.se[2 * v] = CS_NONE; }
        __syncthreads();
        for (int v = threadIdx.x; v < V; v += CS_THREADS) {
            if (w.state[v]) continue;
            const uint32_t s = w.se[2 * v], e = w.se[2 * v + 1];
            const double d = cs_dist(CS_PT(v), CS_PT(s), CS_PT(e));
            atomicMax(&w.key[s], (unsigned long long)__double_as_longlong(d));
        }
        __syncthreads();
        for (int v = threadIdx.x; v < V; v += CS_THREADS) {
            if (w.state[v]) continue;
            const uint32_t s = w.se[2 * v], e = w.se[2 * v + 1];
            const double d = cs_dist(CS_PT(v), CS_PT(s), CS_PT(e));          // the same operations: the same bits
            if (d > tol && (unsigned long long)__double_as_longlong(d) == w.key[s]) atomicMin(&w.se[2 * s], (uint32_t)v);
        }
        __syncthreads();
        int changed = 0;
        for (int v = threadIdx.x; v < V; v += CS_THREADS) {
            if (w.state[v]) continue;
            const uint32_t win = w.se[2 * w.se[2 * v]];
            if (win == CS_NONE) { w.state[v] = CS_DEAD; continue; }
            changed = 1;
            if ((uint32_t)v == win) w.state[v] = CS_KEPT;
            else if ((uint32_t)v < win) w.se[2 * v + 1] = win;
            else w.se[2 * v] = win;
        }
        if (!__syncthreads_or(changed)) break;
    }
#undef CS_PT
}

// stages A - D of polyline i (n >= 2 explicit points, already in w.pt).  stage_src [2 n]: the explicit point of every output vertex, piece after piece;
// stage_piece [n]: (first, one past the last) of every piece inside stage_src; pcount[0 .. 3) = vertices, pieces, longest piece.
__device__ __forceinline__ void cs_polyline(const CsIn& in, const CsWork& w, int n, const float* cf, int32_t* stage_src, int2* stage_piece, int32_t* pcount) {
    __shared__ int red[CS_THREADS / 64];
    __shared__ int sh[4];          // corners: count, first, last; longest piece
    const int tid = threadIdx.x;

    // ---- A
    for (int k = tid; k < n; k += CS_THREADS) {
        const bool end = k == 0 || k == n - 1;
        w.idx[k] = k;
        w.state[k] = (end || !(in.tol_pre > 0.0)) ? CS_KEPT : 0;
        w.se[2 * k] = 0; w.se[2 * k + 1] = n - 1;
    }
    if (tid == 0) { sh[0] = 0; sh[1] = 0x7fffffff; sh[2] = -1; sh[3] = 0; }
    __syncthreads();
    if (in.tol_pre > 0.0) cs_dp(w, n, n, 0, in.tol_pre);
    __syncthreads();
    int m = 0;
    for (int at = 0; at < n; at += CS_THREADS) {          // survivors, in order
        const int k = at + tid;
        const int f = (k < n && (w.state[k] & CS_KEPT)) ? 1 : 0;
        int total;
        const int incl = wg_scan<false, int>(f, red, total);
        if (k < n) w.fl[k] = f;
        if (f) w.idx[m + incl - 1] = k;          // slot <= k, and nothing reads idx here
        m += total;
    }
    __syncthreads();

    // ---- B
    const float2 q0 = w.pt[w.idx[0]], ql = w.pt[w.idx[m - 1]];
    const double gr = fabs((double)q0.x - (double)ql.x), gc = fabs((double)q0.y - (double)ql.y);
    const bool ring = (gr > gc ? gr : gc) < 1e-6;
    for (int j = tid; j < m; j += CS_THREADS) {
        bool corner;
        if (ring) {
            if (j == m - 1) continue;          // written with vertex 0
            const float2 p = w.pt[w.idx[j]], a = w.pt[w.idx[j == 0 ? m - 2 : j - 1]], b = w.pt[w.idx[j + 1]];
            corner = cs_corner(in, cf, p, (double)a.x - (double)p.x, (double)a.y - (double)p.y, (double)b.x - (double)p.x, (double)b.y - (double)p.y);
            if (j == 0) w.mask[m - 1] = corner;
        } else if (j == 0 || j == m - 1) corner = true;
        else {
            const float2 p = w.pt[w.idx[j]], a = w.pt[w.idx[j - 1]], b = w.pt[w.idx[j + 1]];
            corner = cs_corner(in, cf, p, (double)a.x - (double)p.x, (double)a.y - (double)p.y, (double)b.x - (double)p.x, (double)b.y - (double)p.y);
        }
        w.mask[j] = corner;
    }
    __syncthreads();
    for (int j = tid; j < m; j += CS_THREADS)
        if (w.mask[j]) { w.fl[w.idx[j]] |= 2; atomicAdd(&sh[0], 1); atomicMin(&sh[1], j); atomicMax(&sh[2], j); }
    __syncthreads();

    // ---- C: the rotated sequence and its boundaries
    const int nc = sh[0];
    const bool merged = nc > 0 && !w.mask[0] && !w.mask[m - 1];
    const int rot = merged ? sh[1] : 0, V = merged ? m + 1 : m;
    const int nb = nc == 0 ? 2 : (merged ? nc + 1 : nc);          // boundaries; nb - 1 pieces
    for (int v = tid; v < V; v += CS_THREADS) {
        const int j = v + rot >= m ? v + rot - m : v + rot;
        const bool bnd = nc == 0 ? (v == 0 || v == V - 1) : w.mask[j] != 0;
        w.state[v] = bnd ? (CS_KEPT | CS_BND) : 0;
    }
    __syncthreads();
    int carry = -1;
    for (int at = 0; at < V; at += CS_THREADS) {          // s: the last boundary at or before v
        const int v = at + tid;
        int total;
        const int s = max(carry, wg_scan<true, int>((v < V && w.state[v]) ? v : -1, red, total));
        if (v < V && !w.state[v]) w.se[2 * v] = (uint32_t)s;
        carry = max(carry, total);
    }
    carry = 0;
    for (int at = 0; at < V; at += CS_THREADS) {          // e: the first boundary at or after v, from the far end (V - e, 0 = none)
        const int v = V - 1 - (at + tid);
        int total;
        const int e = max(carry, wg_scan<true, int>((v >= 0 && w.state[v]) ? V - v : 0, red, total));
        if (v >= 0 && !w.state[v]) {
            if (e == 0 || w.se[2 * v] == CS_NONE) w.state[v] = CS_DEAD;          // outside every piece
            else { w.se[2 * v + 1] = (uint32_t)(V - e); if (!(in.tol > 0.0)) w.state[v] = CS_KEPT; }
        }
        carry = max(carry, total);
    }
    __syncthreads();

    // ---- D
    if (in.tol > 0.0) cs_dp(w, V, m, rot, in.tol);
    __syncthreads();

    // ---- the polyline's output: kept entries in order, a boundary between two pieces twice
    int kept_before = 0, bnd_before = 0;
    for (int at = 0; at < V; at += CS_THREADS) {
        const int v = at + tid;
        const int st = v < V ? w.state[v] : 0;
        const int fk = (st & CS_KEPT) ? 1 : 0, fb = (st & CS_BND) ? 1 : 0;
        int tk, tb;
        const int ik = wg_scan<false, int>(fk, red, tk), ib = wg_scan<false, int>(fb, red, tb);
        if (fk) {
            const int kb = kept_before + ik - 1, b = bnd_before + ib - 1;          // kept entries before v; index of the last boundary at or before v
            const int j = v + rot >= m ? v + rot - m : v + rot;
            const int32_t src = (int32_t)w.idx[j];
            if (v < m) w.fl[src] |= 4;
            if (!fb) stage_src[kb + b] = src;
            else {
                if (b < nb - 1) { stage_src[kb + b] = src; stage_piece[b].x = kb + b; }
                if (b >= 1) { stage_src[kb + b - 1] = src; stage_piece[b - 1].y = kb + b; }
            }
        }
        kept_before += tk; bnd_before += tb;
    }
    __syncthreads();          // stage_piece of this workgroup is visible to it
    for (int p = tid; p < nb - 1; p += CS_THREADS) atomicMax(&sh[3], stage_piece[p].y - stage_piece[p].x);
    __syncthreads();
    if (tid == 0 && nb >= 2) { pcount[0] = kept_before + nb - 2; pcount[1] = nb - 1; pcount[2] = sh[3]; }
}

// exoff [P + 1]: first explicit point of every polyline.  A polyline whose points would pass the capacity E (overlapping slices) gets none and sets status bit 1.
__global__ __launch_bounds__(CS_SCAN_THREADS) void cs_offsets_kernel(CsIn in, int64_t* exoff, int32_t* flag) {
    __shared__ int64_t red[CS_SCAN_THREADS / 64];
    int64_t carry = 0;
    int over = 0;
    for (int at = 0; at < in.P; at += CS_SCAN_THREADS) {
        const int i = at + threadIdx.x;
        int64_t s0; int len = 0, n = 0;
        if (i < in.P) cs_range(in, i, s0, len, n);
        const int64_t ex = wg_excl((int64_t)n, red, carry);
        if (i < in.P) {
            const bool fits = ex + n <= in.E;
            exoff[i] = fits ? ex : -1;
            over |= fits ? 0 : 1;
        }
    }
    if (__syncthreads_or(over) && threadIdx.x == 0) *flag = 2;
    if (threadIdx.x == 0) exoff[in.P] = carry < in.E ? carry : in.E;
}

struct CsStage { const int64_t* exoff; int32_t* src; int2* piece; int32_t* pcount; uint8_t* flags; };

__global__ __launch_bounds__(CS_THREADS) void cs_lds_kernel(CsIn in, CsStage st) {
    __shared__ float2 pt[CS_LDS_CAP];
    __shared__ uint32_t idx[CS_LDS_CAP];
    __shared__ uint32_t se[2 * (CS_LDS_CAP + CS_PAD)];
    __shared__ unsigned long long key[CS_LDS_CAP + CS_PAD];
    __shared__ uint8_t state[CS_LDS_CAP + CS_PAD], mask[CS_LDS_CAP], fl[CS_LDS_CAP];
    const int i = blockIdx.x;
    int64_t s0; int len, n;
    cs_range(in, i, s0, len, n);
    const int64_t off = st.exoff[i];
    if (n < 2 || n > CS_LDS_CAP || off < 0) return;          // uniform over the workgroup
    for (int k = threadIdx.x; k < n; k += CS_THREADS) pt[k] = cs_point(in, s0, len, k);
    const int b = min(max(in.poly_batch[i], 0), in.B - 1);
    CsWork w = {pt, idx, se, key, state, mask, fl};
    cs_polyline(in, w, n, in.c0c2 + (int64_t)b * 4 * in.H * in.W, st.src + 2 * off, st.piece + off, st.pcount + 4 * (int64_t)i);
    for (int k = threadIdx.x; k < n; k += CS_THREADS) st.flags[off + k] = fl[k];
}

struct CsGlobal { float2* pt; uint32_t* idx; uint32_t* se; unsigned long long* key; uint8_t* state; uint8_t* mask; };

__global__ __launch_bounds__(CS_THREADS) void cs_global_kernel(CsIn in, CsStage st, CsGlobal g, int all) {
    const int i = blockIdx.x;
    int64_t s0; int len, n;
    cs_range(in, i, s0, len, n);
    const int64_t off = st.exoff[i];
    if (n < 2 || (!all && n <= CS_LDS_CAP) || off < 0) return;
    const int64_t o1 = off + (int64_t)CS_PAD * i;          // the arrays with one entry more per polyline
    for (int k = threadIdx.x; k < n; k += CS_THREADS) g.pt[off + k] = cs_point(in, s0, len, k);
    const int b = min(max(in.poly_batch[i], 0), in.B - 1);
    CsWork w = {g.pt + off, g.idx + off, g.se + 2 * o1, g.key + o1, g.state + o1, g.mask + off, st.flags + off};
    cs_polyline(in, w, n, in.c0c2 + (int64_t)b * 4 * in.H * in.W, st.src + 2 * off, st.piece + off, st.pcount + 4 * (int64_t)i);
}

// pcount [P][4] -> out offsets of every polyline (vertices << 32 | pieces), the totals, the longest piece and the status
__global__ __launch_bounds__(CS_SCAN_THREADS) void cs_scan_kernel(int P, const int32_t* pcount, unsigned long long* ooff, int max_vertices, int max_pieces,
                                                                  const int32_t* flag, int32_t* counts, int32_t* status) {
    __shared__ unsigned long long red[CS_SCAN_THREADS / 64];
    __shared__ int lmax[CS_SCAN_THREADS / 64];
    unsigned long long carry = 0;
    int longest = 0;
    for (int at = 0; at < P; at += CS_SCAN_THREADS) {
        const int i = at + threadIdx.x;
        unsigned long long v = 0;
        if (i < P) { v = p3_pack2(pcount[4 * (int64_t)i], pcount[4 * (int64_t)i + 1]); longest = max(longest, pcount[4 * (int64_t)i + 2]); }
        const unsigned long long ex = wg_excl(v, red, carry);
        if (i < P) ooff[i] = ex;
    }
    const int mx = wg_max(longest, lmax);
    if (threadIdx.x == 0) {
        const int nv = p3_hi32(carry), np = p3_lo32(carry);          // at most 2 E and E, and the entry point keeps E below 2^30
        counts[0] = nv; counts[1] = np; counts[2] = mx;
        status[0] = ((nv > max_vertices || np > max_pieces) ? 1 : 0) | *flag;
    }
}

__global__ __launch_bounds__(CS_THREADS) void cs_emit_kernel(CsIn in, CsStage st, const unsigned long long* ooff, int max_vertices, int max_pieces, float2* out_pos,
                                                             int32_t* out_src, int64_t* piece_slice, int32_t* piece_poly, int32_t* piece_batch) {
    const int i = blockIdx.x;
    const int nv = st.pcount[4 * (int64_t)i], np = st.pcount[4 * (int64_t)i + 1];
    const int64_t off = st.exoff[i];
    if (nv <= 0 || off < 0) return;
    int64_t s0; int len, n;
    cs_range(in, i, s0, len, n);
    const unsigned long long o = ooff[i];
    const int64_t vo = (int64_t)(o >> 32), po = (int64_t)(o & 0xffffffffull);
    for (int t = threadIdx.x; t < nv; t += CS_THREADS) {
        const int64_t g = vo + t;
        if (g >= max_vertices) break;
        const int k = min(max(st.src[2 * off + t], 0), n - 1);
        out_src[g] = k;
        out_pos[g] = cs_point(in, s0, len, k);
    }
    const int b = min(max(in.poly_batch[i], 0), in.B - 1);
    for (int p = threadIdx.x; p < np; p += CS_THREADS) {
        const int64_t g = po + p;
        if (g >= max_pieces) break;
        const int2 r = st.piece[off + p];
        piece_slice[2 * g] = vo + r.x; piece_slice[2 * g + 1] = vo + r.y;
        piece_poly[g] = i; piece_batch[g] = b;
    }
}

// ---------------------------------------------------------------------------------------------------------------- workspace
struct CsWs {
    int64_t* exoff;
    int32_t *flag, *pcount;          // cleared together before every run: [flag, ooff)
    unsigned long long* ooff;
    int32_t* src; int2* piece; uint8_t* flags;
    CsGlobal g;
};
static CsWs cs_carve(int64_t E, int P, P3Carve& c) {
    CsWs l;
    memset(&l, 0, sizeof l);
    if (E < 1 || P < 1) return l;
    const int64_t E1 = E + (int64_t)CS_PAD * P;
    l.exoff = c.take<int64_t>((int64_t)P + 1);
    l.flag = c.take<int32_t>(1);
    l.pcount = c.take<int32_t>(4 * (int64_t)P);
    l.ooff = c.take<unsigned long long>(P);
    l.src = c.take<int32_t>(2 * E);
    l.piece = c.take<int2>(E);
    l.flags = c.take<uint8_t>(E);
    l.g.pt = c.take<float2>(E);
    l.g.idx = c.take<uint32_t>(E);
    l.g.se = c.take<uint32_t>(2 * E1);
    l.g.key = c.take<unsigned long long>(E1);
    l.g.state = c.take<uint8_t>(E1);
    l.g.mask = c.take<uint8_t>(E);
    return l;
}

extern "C" int64_t p3_corner_split_workspace_bytes(int64_t E, int P) {
    P3Carve c = {nullptr, 0};
    cs_carve(E, P, c);
    return c.at;
}

extern "C" int p3_corner_split(const float* pos, int64_t N, const int64_t* index, int64_t K, const int64_t* slice, const uint8_t* closed, const int32_t* poly_batch,
                               int P, const float* c0c2, int B, int H, int W, double tol_pre, double tol, int max_len, int force_fallback, int max_vertices,
                               int max_pieces, float* out_pos, int32_t* out_src, int64_t* piece_slice, int32_t* piece_poly, int32_t* piece_batch,
                               uint8_t* stage_flags, int32_t* counts, int32_t* status, void* workspace, void* stream) {
    P3_CHECK(P >= 0 && N >= 0 && K >= 0 && max_vertices >= 0 && max_pieces >= 0, P3_ESHAPE, "p3_corner_split: bad sizes (N, K, P, capacities >= 0)");
    P3_CHECK(B >= 1 && H >= 1 && W >= 1, P3_ESHAPE, "p3_corner_split: bad map sizes (B, H, W >= 1)");
    const int64_t E = (index ? K : N) + P;
    P3_CHECK(E < ((int64_t)1 << 30), P3_ESHAPE, "p3_corner_split: (index ? K : N) + P must stay below 2^30");
    P3_CHECK(counts && status, P3_EINVAL, "p3_corner_split: null pointer (counts, status)");
    P3_CHECK(tol_pre == tol_pre && tol == tol, P3_EINVAL, "p3_corner_split: a tolerance is NaN");
    P3_CHECK(index || K == 0, P3_EINVAL, "p3_corner_split: K > 0 without index");
    hipStream_t s = (hipStream_t)stream;
    if (P == 0 || N == 0 || (index && K == 0)) {          // no explicit point
        P3_TRY(p3_memset(counts, 0, 3 * sizeof(int32_t), s));
        return p3_memset(status, 0, sizeof(int32_t), s);
    }
    P3_CHECK(pos && slice && closed && poly_batch && c0c2, P3_EINVAL, "p3_corner_split: null pointer");
    P3_CHECK((max_vertices == 0 || (out_pos && out_src)) && (max_pieces == 0 || (piece_slice && piece_poly && piece_batch)), P3_EINVAL,
             "p3_corner_split: null output with a capacity above 0");
    P3_CHECK(workspace, P3_EINVAL, "p3_corner_split: null workspace (p3_corner_split_workspace_bytes((index ? K : N) + P, P))");
    P3Carve carve = {(char*)workspace, 0};
    const CsWs l = cs_carve(E, P, carve);
    CsIn in;
    in.pos = (const float2*)pos; in.index = index; in.slice = slice; in.closed = closed; in.poly_batch = poly_batch; in.c0c2 = c0c2;
    in.N = N; in.K = index ? K : 0; in.E = E; in.P = P; in.B = B; in.H = H; in.W = W; in.tol_pre = tol_pre; in.tol = tol;
    CsStage st = {l.exoff, l.src, l.piece, l.pcount, stage_flags ? stage_flags : l.flags};
    // a polyline nobody runs (under 2 points, over a wrong max_len, past the capacity E) has no piece and flags 0
    P3_TRY(p3_memset(l.flag, 0, (char*)l.ooff - (char*)l.flag, s));
    P3_TRY(p3_memset(st.flags, 0, E, s));
    const bool fast = !force_fallback;
    const bool slow = force_fallback || max_len <= 0 || (int64_t)max_len + 1 > CS_LDS_CAP;          // + 1: the closing point
    P3_TRY(p3_launch<cs_offsets_kernel>(nullptr, 1, CS_SCAN_THREADS, 0, s, in, l.exoff, l.flag));
    if (fast) P3_TRY(p3_launch<cs_lds_kernel>("cs_lds_kernel", P, CS_THREADS, 0, s, in, st));
    if (slow) P3_TRY(p3_launch<cs_global_kernel>(fast ? nullptr : "cs_global_kernel", P, CS_THREADS, 0, s, in, st, l.g, force_fallback ? 1 : 0));
    P3_TRY(p3_launch<cs_scan_kernel>(nullptr, 1, CS_SCAN_THREADS, 0, s, P, st.pcount, l.ooff, max_vertices, max_pieces, l.flag, counts, status));
    return p3_launch<cs_emit_kernel>(nullptr, P, CS_THREADS, 0, s, in, st, l.ooff, max_vertices, max_pieces, (float2*)out_pos, out_src, piece_slice, piece_poly,
                                     piece_batch);
}
