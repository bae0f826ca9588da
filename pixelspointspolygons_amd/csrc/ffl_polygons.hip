// p3hip - FFL polygons on the device: the planar-graph half of `shapely_postprocess` (predict/ffl/polygonize_acm.py:281-324, polygonize_asm.py:438-494:
// LineString per piece + the border ring, shapely.ops.unary_union, polygonize_full / polygonize, the min_area filter and polygonize_utils.compute_geom_prob
// :64-101 with the seg_threshold filter) behind p3_corner_split.
//   p3_ffl_polygons   pieces + indicator map -> polygons (a shell and its holes), their areas, probabilities and filter flags.
// DESIGN.md section 19 holds the definition; include/p3hip.h repeats it at the prototype.
//
// Images never interact: one workgroup per image (ffp_image), every working array in LDS.
//   1  segments of the image's pieces, zero-length pairs dropped, in piece order (a scan over the pieces)
//   2  nodes = the distinct end points + the four border corners, sorted by (x, y): a rank sort, every point counts the smaller ones
//   3  edges = segments as node pairs + the border sides, each side cut at the nodes that lie on it (a node's edge goes to the next node of its side);
//      duplicates die, every pair of edges is tested for a shared point (orientation signs in double): the image is flagged and gives nothing
//   4  dangles: edges with an end of degree 1 die, round after round
//   5  trace: outgoing half-edges per node (CSR by degree), ranked by angle inside the node; next(u->v) = the half-edge before v->u in counter-clockwise
//      order at v; a half-edge is its ring's start when no half-edge of the ring has a smaller (origin, destination) key - it walks until it meets one;
//      the start walks the ring once more: ring mark, shoelace sum in ring order, length
//   6  cuts: an edge with both half-edges on one ring dies; trace again (once: what is left is 2-edge-connected)
//   7  a ring with a negative sum looks for the smallest shell that contains its start node (crossing number, orientation signs; a shell that visits
//      the node is of the same component and never contains it) and becomes its hole; without one it is the unbounded face
//   8  shells ranked by key, holes ranked by key inside their shell; rings, polygons and areas go to the image's staging area
// ffp_lds_kernel runs the images of up to FFP_LDS_CAP edge slots, ffp_global_kernel the same function over the workspace for larger ones (or all, forced).
// ffp_prob_kernel: one workgroup of 1024 threads per polygon over the pixels of its window, the rounded rings and their boxes in LDS (the workspace for a
// polygon past FFP_PROB_VERTS / FFP_PROB_RINGS), exact integer edge tests, the indicator summed in double by thread-strided partial sums and a fixed tree.  No floating-point atomics; every decision is a comparison: two runs, either form, give the same bits.
// Launches: ffp_count (edge slots per image, input checks), ffp_offsets, ffp_lds / ffp_global, ffp_scan (offsets of the images' outputs, totals, status),
// ffp_emit (compaction, nothing past the capacities), ffp_prob.  No host synchronisation.
#include "p3_common.h"

#pragma clang fp contract(off)

#define FFP_THREADS 256
#define FFP_SCAN_THREADS 1024
#define FFP_LDS_CAP 1024          // edge slots of an image that run in LDS: 123 B per slot = 123 KiB of the CU's 160 KiB, one workgroup per CU
#define FFP_PAD 8                 // the node-indexed arrays hold one entry more than there are nodes
#define FFP_FOR(i, n) for (int i = threadIdx.x; i < (n); i += FFP_THREADS)

struct FfpPt { float x, y; };          // x = col, y = row

struct FfpIn {
    const float2* pos; const int64_t* slice; const int32_t* pbatch;
    int64_t V;
    int Q, B, H, W;
    double min_area;
};
struct FfpWork {                  // per image, LDS or workspace; C = edge slots
    double* rS;                   // [2 C] shoelace sum of the ring that starts at a half-edge.  The raw segments (FfpPt [2 C][2]) lie in the same bytes
    FfpPt* node;                  // [2 C + PAD]
    int32_t *eu, *ev;             // [C] edge = (node, node), eu < ev
    uint8_t* elive;               // [C] 1 live, 2 dying, 0 dead
    uint8_t* fl;                  // [2 C] first occurrence of a raw point; later: the half-edge starts a ring
    int32_t *deg, *start, *adj, *srt, *rank, *nxt, *ringof, *rlen, *rpar, *rtab;          // [2 C + PAD]
};
struct FfpStage { float2* pos; int2* ipos; int2* ring; int2* poly; float* area; int32_t* aflag; int4* rbox; };          // pos / ipos [3 S], the others [S], S = all edge slots

__device__ __forceinline__ bool ffp_eq(FfpPt a, FfpPt b) { return a.x == b.x && a.y == b.y; }
__device__ __forceinline__ bool ffp_less(FfpPt a, FfpPt b) { return a.x < b.x || (a.x == b.x && a.y < b.y); }
__device__ __forceinline__ FfpPt ffp_load(const FfpIn& in, int64_t k) {
    const float2 p = in.pos[k];
    FfpPt r; r.x = p.y + 0.0f; r.y = p.x + 0.0f;          // -0 becomes +0: equal coordinates have equal bits
    return r;
}
// piece q is well formed; s, e its slice
__device__ __forceinline__ bool ffp_piece_ok(const FfpIn& in, int q, int64_t& s, int64_t& e, int& pb) {
    s = in.slice[2 * (int64_t)q]; e = in.slice[2 * (int64_t)q + 1]; pb = in.pbatch[q];
    return s >= 0 && e >= s && e <= in.V && pb >= 0 && pb < in.B;
}
// p lies on border side k (0: x = 0, 1: y = H - 1, 2: x = W - 1, 3: y = 0); c: its coordinate along the side
__device__ __forceinline__ bool ffp_side(FfpPt p, int k, float xm, float ym, float& c) {
    if (k == 0 || k == 2) {
        if (p.x != (k == 0 ? 0.0f : xm) || !(p.y >= 0.0f && p.y <= ym)) return false;
        c = p.y;
    } else {
        if (p.y != (k == 3 ? 0.0f : ym) || !(p.x >= 0.0f && p.x <= xm)) return false;
        c = p.x;
    }
    return true;
}
__device__ __forceinline__ bool ffp_on_border(FfpPt p, float xm, float ym) {
    float c;
    return ffp_side(p, 0, xm, ym, c) || ffp_side(p, 1, xm, ym, c) || ffp_side(p, 2, xm, ym, c) || ffp_side(p, 3, xm, ym, c);
}
__device__ __forceinline__ double ffp_orient(FfpPt a, FfpPt b, FfpPt c) {
    return ((double)b.x - (double)a.x) * ((double)c.y - (double)a.y) - ((double)b.y - (double)a.y) * ((double)c.x - (double)a.x);
}
__device__ __forceinline__ bool ffp_in_box(FfpPt a, FfpPt b, FfpPt c) {
    return c.x >= fminf(a.x, b.x) && c.x <= fmaxf(a.x, b.x) && c.y >= fminf(a.y, b.y) && c.y <= fmaxf(a.y, b.y);
}
// two different edges (a, b), (c, d) given by node ids share a point that is no common end node
__device__ __forceinline__ bool ffp_not_planar(const FfpPt* node, int a, int b, int c, int d) {
    if (a == c || a == d || b == c || b == d) {
        const int o = (a == c || a == d) ? a : b, p = o == a ? b : a, q = (o == c) ? d : c;
        const FfpPt O = node[o], Pp = node[p], Qq = node[q];
        if (ffp_orient(O, Pp, Qq) != 0.0) return false;
        const double dot = ((double)Pp.x - (double)O.x) * ((double)Qq.x - (double)O.x) + ((double)Pp.y - (double)O.y) * ((double)Qq.y - (double)O.y);
        return dot > 0.0;
    }
    const FfpPt A = node[a], Bb = node[b], Cc = node[c], D = node[d];
    const double o1 = ffp_orient(A, Bb, Cc), o2 = ffp_orient(A, Bb, D), o3 = ffp_orient(Cc, D, A), o4 = ffp_orient(Cc, D, Bb);
    if (((o1 > 0.0 && o2 < 0.0) || (o1 < 0.0 && o2 > 0.0)) && ((o3 > 0.0 && o4 < 0.0) || (o3 < 0.0 && o4 > 0.0))) return true;
    return (o1 == 0.0 && ffp_in_box(A, Bb, Cc)) || (o2 == 0.0 && ffp_in_box(A, Bb, D)) || (o3 == 0.0 && ffp_in_box(Cc, D, A)) || (o4 == 0.0 && ffp_in_box(Cc, D, Bb));
}
__device__ __forceinline__ int ffp_origin(const FfpWork& w, int h) { return (h & 1) ? w.ev[h >> 1] : w.eu[h >> 1]; }
__device__ __forceinline__ unsigned long long ffp_key(const FfpWork& w, int h) {
    return p3_pack2(ffp_origin(w, h), ffp_origin(w, h ^ 1));
}
// direction g comes before direction h counter-clockwise from the positive x axis (both leave node o)
__device__ __forceinline__ bool ffp_angle_less(const FfpWork& w, int o, int g, int h) {
    const FfpPt O = w.node[o], G = w.node[ffp_origin(w, g ^ 1)], Hh = w.node[ffp_origin(w, h ^ 1)];
    const double gx = (double)G.x - (double)O.x, gy = (double)G.y - (double)O.y, hx = (double)Hh.x - (double)O.x, hy = (double)Hh.y - (double)O.y;
    const int hg = (gy > 0.0 || (gy == 0.0 && gx > 0.0)) ? 0 : 1, hh = (hy > 0.0 || (hy == 0.0 && hx > 0.0)) ? 0 : 1;
    if (hg != hh) return hg < hh;
    return gx * hy - gy * hx > 0.0;
}

// the rings of the live edges: nxt, fl (ring start), ringof, rS, rlen.  Every thread of the workgroup calls it.
__device__ __forceinline__ void ffp_trace(const FfpWork& w, int N, int ne, int* red) {
    const int tid = threadIdx.x;
    FFP_FOR(n, N) { w.deg[n] = 0; w.rlen[n] = 0; }
    __syncthreads();
    FFP_FOR(e, ne) if (w.elive[e] == 1) { atomicAdd(&w.deg[w.eu[e]], 1); atomicAdd(&w.deg[w.ev[e]], 1); }
    __syncthreads();
    int carry = 0;
    for (int at = 0; at < N; at += FFP_THREADS) {
        const int n = at + tid, v = n < N ? w.deg[n] : 0;
        const int ex = wg_excl(v, red, carry);
        if (n < N) w.start[n] = ex;
    }
    if (tid == 0) w.start[N] = carry;
    __syncthreads();
    FFP_FOR(h, 2 * ne) {
        w.fl[h] = 0;
        if (w.elive[h >> 1] != 1) continue;
        const int u = ffp_origin(w, h);
        w.adj[w.start[u] + atomicAdd(&w.rlen[u], 1)] = h;          // any order: the rank below does not depend on it
    }
    __syncthreads();
    FFP_FOR(h, 2 * ne) {
        if (w.elive[h >> 1] != 1) continue;
        const int u = ffp_origin(w, h);
        int r = 0;
        for (int i = w.start[u]; i < w.start[u + 1]; ++i) { const int g = w.adj[i]; if (g != h && ffp_angle_less(w, u, g, h)) ++r; }
        w.rank[h] = r;
        w.srt[w.start[u] + r] = h;
    }
    __syncthreads();
    FFP_FOR(h, 2 * ne) {
        if (w.elive[h >> 1] != 1) continue;
        const int t = h ^ 1, v = ffp_origin(w, t), d = w.start[v + 1] - w.start[v], p = w.rank[t];
        w.nxt[h] = w.srt[w.start[v] + (p == 0 ? d - 1 : p - 1)];
    }
    __syncthreads();
    FFP_FOR(h, 2 * ne) {
        if (w.elive[h >> 1] != 1) continue;
        const unsigned long long kh = ffp_key(w, h);
        int g = w.nxt[h], is = 1;
        for (int it = 0; it < 2 * ne && g != h; ++it) {
            if (ffp_key(w, g) < kh) { is = 0; break; }
            g = w.nxt[g];
        }
        w.fl[h] = (uint8_t)is;
    }
    __syncthreads();
    FFP_FOR(h, 2 * ne) {
        if (!w.fl[h]) continue;
        double S = 0.0;
        int L = 0, g = h;
        do {
            w.ringof[g] = h;
            const FfpPt a = w.node[ffp_origin(w, g)], c = w.node[ffp_origin(w, g ^ 1)];
            S += (double)a.x * (double)c.y - (double)c.x * (double)a.y;
            ++L;
            g = w.nxt[g];
        } while (g != h && L < 2 * ne);
        w.rS[h] = S; w.rlen[h] = L;
    }
    __syncthreads();
}

// node p lies strictly inside the ring that starts at half-edge g (a ring that visits p does not contain it)
__device__ __forceinline__ bool ffp_contains(const FfpWork& w, int g, int p, int ne) {
    const FfpPt Pp = w.node[p];
    int par = 0, x = g, it = 0;
    do {
        const int a = ffp_origin(w, x), c = ffp_origin(w, x ^ 1);
        if (a == p) return false;
        const FfpPt A = w.node[a], Cc = w.node[c];
        if ((A.y <= Pp.y) != (Cc.y <= Pp.y)) {
            const double o = ffp_orient(A, Cc, Pp);
            if (Cc.y > A.y ? o > 0.0 : o < 0.0) par ^= 1;
        }
        x = w.nxt[x];
    } while (x != g && ++it < 2 * ne);
    return par != 0;
}

// steps 1 - 8 for image b.  -> the image's status bits; pcount[0 .. 3) = polygons, rings, vertices (left as they are, zero, when a bit is set)
__device__ __forceinline__ int ffp_image(const FfpIn& in, const FfpWork& w, int C, int b, const FfpStage& st, int32_t* pcount) {
    __shared__ int red[FFP_THREADS / 64];
    __shared__ int sh[8];          // 0 status bits, 1 nodes, 2 edges, 3 shells, 4 rings, 5 vertices
    const int tid = threadIdx.x;
    const float xm = (float)(in.W - 1), ym = (float)(in.H - 1);
    FfpPt* seg = (FfpPt*)w.rS;
    if (tid < 8) sh[tid] = 0;
    __syncthreads();

    // ---- 1 segments, in piece order
    int nseg = 0;
    for (int at = 0; at < in.Q; at += FFP_THREADS) {
        const int q = at + tid;
        int64_t s = 0, e = 0;
        int pb = -1;
        const bool mine = q < in.Q && ffp_piece_ok(in, q, s, e, pb) && pb == b;
        int cnt = 0;
        if (mine)
            for (int64_t k = s; k + 1 < e; ++k) {
                const FfpPt a = ffp_load(in, k), c = ffp_load(in, k + 1);
                if (!isfinite(a.x) || !isfinite(a.y) || !isfinite(c.x) || !isfinite(c.y)) atomicOr(&sh[0], 2);
                if (!ffp_eq(a, c)) ++cnt;
            }
        int o = wg_excl(cnt, red, nseg);
        if (mine && cnt) {
            for (int64_t k = s; k + 1 < e; ++k) {
                const FfpPt a = ffp_load(in, k), c = ffp_load(in, k + 1);
                if (ffp_eq(a, c)) continue;
                if (o < C - 4) { seg[2 * o] = a; seg[2 * o + 1] = c; }
                ++o;
            }
        }
    }
    if (nseg > C - 4) { nseg = C - 4; if (tid == 0) atomicOr(&sh[0], 8); }          // cannot happen: ffp_count gave the image nseg + 4 slots at least
    __syncthreads();
    if (sh[0]) return sh[0];

    // ---- 2 nodes
    const int P = 2 * nseg + 4;
    auto raw = [&](int i) -> FfpPt {
        if (i < 2 * nseg) return seg[i];
        const int k = i - 2 * nseg;
        FfpPt c; c.x = (k == 2 || k == 3) ? xm : 0.0f; c.y = (k == 1 || k == 2) ? ym : 0.0f;
        return c;
    };
    FFP_FOR(i, P) {
        const FfpPt p = raw(i);
        int f = 1;
        for (int j = 0; j < i; ++j) if (ffp_eq(raw(j), p)) { f = 0; break; }
        w.fl[i] = (uint8_t)f;
        if (f) atomicAdd(&sh[1], 1);
    }
    __syncthreads();
    const int N = sh[1];
    FFP_FOR(i, P) {
        if (!w.fl[i]) continue;
        const FfpPt p = raw(i);
        int id = 0;
        for (int j = 0; j < P; ++j) if (w.fl[j] && ffp_less(raw(j), p)) ++id;
        w.node[id] = p;
    }
    if (tid == 0) sh[2] = nseg;
    __syncthreads();

    // ---- 3 edges
    auto find = [&](FfpPt p) -> int {
        int lo = 0, hi = N;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (ffp_less(w.node[mid], p)) lo = mid + 1; else hi = mid; }
        return lo < N ? lo : N - 1;
    };
    FFP_FOR(s, nseg) {
        const int u = find(seg[2 * s]), v = find(seg[2 * s + 1]);
        w.eu[s] = min(u, v); w.ev[s] = max(u, v); w.elive[s] = 1;
    }
    FFP_FOR(n, N) {
        const FfpPt p = w.node[n];
        for (int k = 0; k < 4; ++k) {
            float c, cm, cbest = 0.0f;
            if (!ffp_side(p, k, xm, ym, c)) continue;
            int best = -1;
            for (int m = 0; m < N; ++m)
                if (ffp_side(w.node[m], k, xm, ym, cm) && cm > c && (best < 0 || cm < cbest)) { best = m; cbest = cm; }
            if (best < 0) continue;
            const int slot = atomicAdd(&sh[2], 1);          // any order: no output depends on an edge's slot
            if (slot < C) { w.eu[slot] = min(n, best); w.ev[slot] = max(n, best); w.elive[slot] = 1; }
        }
    }
    __syncthreads();
    if (sh[2] > C && tid == 0) atomicOr(&sh[0], 8);          // cannot happen either
    const int ne = min(sh[2], C);
    __syncthreads();          // the raw segments are dead from here on: rS may be written
    FFP_FOR(e, ne) {
        const int a = w.eu[e], c = w.ev[e];
        int flag = 0;
        for (int f = 0; f < e; ++f) {
            const int a2 = w.eu[f], c2 = w.ev[f];
            if (a == a2 && c == c2) { w.elive[e] = 0; continue; }          // a duplicate: the first one stays
            if (ffp_not_planar(w.node, a, c, a2, c2)) { flag = 1; break; }
        }
        if (flag) atomicOr(&sh[0], 1);
    }
    __syncthreads();
    if (sh[0]) return sh[0];

    // ---- 4 dangles
    FFP_FOR(n, N) w.deg[n] = 0;
    __syncthreads();
    FFP_FOR(e, ne) if (w.elive[e]) { atomicAdd(&w.deg[w.eu[e]], 1); atomicAdd(&w.deg[w.ev[e]], 1); }
    __syncthreads();
    for (int round = 0; round <= ne; ++round) {
        int changed = 0;
        FFP_FOR(e, ne) if (w.elive[e] == 1 && (w.deg[w.eu[e]] == 1 || w.deg[w.ev[e]] == 1)) { w.elive[e] = 2; changed = 1; }
        if (!__syncthreads_or(changed)) break;
        FFP_FOR(e, ne) if (w.elive[e] == 2) { w.elive[e] = 0; atomicSub(&w.deg[w.eu[e]], 1); atomicSub(&w.deg[w.ev[e]], 1); }
        __syncthreads();
    }

    // ---- 5, 6 rings; cuts; rings again
    ffp_trace(w, N, ne, red);
    int cut = 0;
    FFP_FOR(e, ne) if (w.elive[e] == 1 && w.ringof[2 * e] == w.ringof[2 * e + 1]) { w.elive[e] = 0; cut = 1; }
    if (__syncthreads_or(cut)) ffp_trace(w, N, ne, red);

    // ---- 7 shells and holes
    const int H2 = 2 * ne;
    FFP_FOR(h, H2) {
        if (!w.fl[h]) continue;
        const double S = w.rS[h];
        if (!(S > 0.0) && !(S < 0.0)) atomicOr(&sh[0], 4);
    }
    __syncthreads();
    if (sh[0]) return sh[0];
    FFP_FOR(h, H2) {
        if (!w.fl[h]) continue;
        w.rpar[h] = -1;
        if (w.rS[h] > 0.0) continue;
        const int p = ffp_origin(w, h);
        int best = -1;
        double bestS = 0.0;
        for (int g = 0; g < H2; ++g) {
            if (!w.fl[g] || !(w.rS[g] > 0.0)) continue;
            const double S = w.rS[g];
            if (best >= 0 && (S > bestS || (S == bestS && ffp_key(w, g) > ffp_key(w, best)))) continue;
            if (ffp_contains(w, g, p, ne)) { best = g; bestS = S; }
        }
        w.rpar[h] = best;
    }
    __syncthreads();

    // ---- 8 order: shells by key (adj[rank] = shell), per shell its rings (rank[h]) and vertices (srt[h])
    FFP_FOR(h, H2) {
        if (!w.fl[h] || !(w.rS[h] > 0.0)) continue;
        const unsigned long long kh = ffp_key(w, h);
        int r = 0, nr = 1, nv = w.rlen[h] + 1;
        for (int g = 0; g < H2; ++g) {
            if (!w.fl[g]) continue;
            if (w.rS[g] > 0.0) { if (ffp_key(w, g) < kh) ++r; }
            else if (w.rpar[g] == h) { ++nr; nv += w.rlen[g] + 1; }
        }
        w.adj[r] = h; w.rank[h] = nr; w.srt[h] = nv;
        atomicAdd(&sh[3], 1);
    }
    __syncthreads();
    const int ns = sh[3];
    int cr = 0, cv = 0;
    for (int at = 0; at < ns; at += FFP_THREADS) {          // deg[rank] = first ring, start[rank] = first vertex of the polygon
        const int r = at + tid, h = r < ns ? w.adj[r] : 0, nr = r < ns ? w.rank[h] : 0, nv = r < ns ? w.srt[h] : 0;
        const int er = wg_excl(nr, red, cr), ev = wg_excl(nv, red, cv);
        if (r < ns) { w.deg[r] = er; w.start[r] = ev; w.ringof[h] = r; }          // ringof[shell] = its rank from here on
    }
    __syncthreads();
    FFP_FOR(h, H2) {          // every ring that is put out: its index, its vertices
        if (!w.fl[h]) continue;
        int ri, vo;
        if (w.rS[h] > 0.0) { const int r = w.ringof[h]; ri = w.deg[r]; vo = w.start[r]; }
        else {
            const int par = w.rpar[h];
            if (par < 0) continue;          // the unbounded face
            const unsigned long long kh = ffp_key(w, h);
            const int r = w.ringof[par];
            ri = w.deg[r] + 1; vo = w.start[r] + w.rlen[par] + 1;
            for (int g = 0; g < H2; ++g)
                if (g != h && w.fl[g] && !(w.rS[g] > 0.0) && w.rpar[g] == par && ffp_key(w, g) < kh) { ++ri; vo += w.rlen[g] + 1; }
        }
        w.rtab[ri] = h;
        const int L = w.rlen[h];
        st.ring[ri] = make_int2(vo, vo + L + 1);
        int g = h;
        for (int i = 0; i <= L; ++i) {          // closed: the start vertex once more
            const FfpPt p = w.node[ffp_origin(w, g)];
            st.pos[vo + i] = make_float2(p.y, p.x);
            g = w.nxt[g];
        }
    }
    __syncthreads();
    FFP_FOR(r, ns) {
        const int h = w.adj[r], r0 = w.deg[r], nr = w.rank[h];
        double area = w.rS[h] * 0.5;
        for (int i = 1; i < nr; ++i) area -= fabs(w.rS[w.rtab[r0 + i]] * 0.5);
        st.poly[r] = make_int2(r0, r0 + nr);
        st.area[r] = (float)area;
        st.aflag[r] = in.min_area < area ? 0 : 1;
    }
    if (tid == 0) { pcount[0] = ns; pcount[1] = cr; pcount[2] = cv; }
    return 0;
}

// slots [B]: the edge slots image b needs = its segments + its segment ends on the border + 4.  flag: bit 1 when a piece is malformed (it is left out).
__global__ __launch_bounds__(FFP_THREADS) void ffp_count_kernel(FfpIn in, int32_t* slots, int32_t* flag) {
    __shared__ int sh[2];
    const int b = blockIdx.x;
    const float xm = (float)(in.W - 1), ym = (float)(in.H - 1);
    if (threadIdx.x < 2) sh[threadIdx.x] = 0;
    __syncthreads();
    int cnt = 0, bad = 0;
    FFP_FOR(q, in.Q) {
        int64_t s, e;
        int pb;
        if (!ffp_piece_ok(in, q, s, e, pb)) { bad = 1; continue; }
        if (pb != b) continue;
        for (int64_t k = s; k + 1 < e; ++k) {
            const FfpPt a = ffp_load(in, k), c = ffp_load(in, k + 1);
            if (!ffp_eq(a, c)) cnt += 1 + (ffp_on_border(a, xm, ym) ? 1 : 0) + (ffp_on_border(c, xm, ym) ? 1 : 0);
        }
    }
    if (cnt) atomicAdd(&sh[0], cnt);
    if (bad) atomicOr(&sh[1], 1);
    __syncthreads();
    if (threadIdx.x == 0) { slots[b] = sh[0] + 4; if (sh[1] && b == 0) *flag = 2; }
}

// soff [B + 1]: first edge slot of every image in the workspace
__global__ __launch_bounds__(FFP_SCAN_THREADS) void ffp_offsets_kernel(int B, const int32_t* slots, int64_t* soff) {
    __shared__ int64_t red[FFP_SCAN_THREADS / 64];
    int64_t carry = 0;
    for (int at = 0; at < B; at += FFP_SCAN_THREADS) {
        const int i = at + threadIdx.x;
        const int64_t ex = wg_excl((int64_t)(i < B ? slots[i] : 0), red, carry);
        if (i < B) soff[i] = ex;
    }
    if (threadIdx.x == 0) soff[B] = carry;
}

struct FfpImages { const int32_t* slots; const int64_t* soff; int64_t S; int32_t* pcount; int32_t* image_status; };

__device__ __forceinline__ FfpStage ffp_stage_of(const FfpStage& st, int64_t off) {
    FfpStage s = {st.pos + 3 * off, st.ipos + 3 * off, st.ring + off, st.poly + off, st.area + off, st.aflag + off, st.rbox + off};
    return s;
}

__global__ __launch_bounds__(FFP_THREADS) void ffp_lds_kernel(FfpIn in, FfpImages im, FfpStage st, int all_global) {
    constexpr int C = FFP_LDS_CAP, C2 = 2 * C + FFP_PAD;
    __shared__ double rS[2 * C];
    __shared__ FfpPt node[C2];
    __shared__ int32_t eu[C], ev[C], deg[C2], start[C2], adj[C2], srt[C2], rank[C2], nxt[C2], ringof[C2], rlen[C2], rpar[C2], rtab[C2];
    __shared__ uint8_t elive[C], fl[2 * C];
    const int b = blockIdx.x;
    const int64_t off = im.soff[b];
    if (all_global || im.slots[b] > C || off + im.slots[b] > im.S) return;          // uniform over the workgroup
    FfpWork w = {rS, node, eu, ev, elive, fl, deg, start, adj, srt, rank, nxt, ringof, rlen, rpar, rtab};
    const int bits = ffp_image(in, w, im.slots[b], b, ffp_stage_of(st, off), im.pcount + 4 * (int64_t)b);          // the image's own slots: its staging area has no more
    if (threadIdx.x == 0) im.image_status[b] = bits;
}

struct FfpGlobal { double* rS; FfpPt* node; int32_t *eu, *ev; uint8_t *elive, *fl; int32_t* ints; int64_t I; };          // ints: 10 arrays of I = 2 S + PAD B entries

__global__ __launch_bounds__(FFP_THREADS) void ffp_global_kernel(FfpIn in, FfpImages im, FfpStage st, FfpGlobal g, int all_global) {
    const int b = blockIdx.x;
    const int64_t off = im.soff[b];
    const int C = im.slots[b];
    if (off + C > im.S) { if (threadIdx.x == 0) im.image_status[b] = 8; return; }          // cannot happen: the workspace holds 3 V + 4 B slots
    if (!all_global && C <= FFP_LDS_CAP) return;
    const int64_t o2 = 2 * off + (int64_t)FFP_PAD * b;
    int32_t* a = g.ints + o2;
    FfpWork w = {g.rS + 2 * off, g.node + o2, g.eu + off, g.ev + off, g.elive + off, g.fl + 2 * off,
                 a, a + g.I, a + 2 * g.I, a + 3 * g.I, a + 4 * g.I, a + 5 * g.I, a + 6 * g.I, a + 7 * g.I, a + 8 * g.I, a + 9 * g.I};
    const int bits = ffp_image(in, w, C, b, ffp_stage_of(st, off), im.pcount + 4 * (int64_t)b);
    if (threadIdx.x == 0) im.image_status[b] = bits;
}

// pcount [B][4] -> ioff [B + 1][3]: first polygon, ring and vertex of every image in the outputs; totals; status
__global__ __launch_bounds__(FFP_SCAN_THREADS) void ffp_scan_kernel(int B, const int32_t* pcount, int64_t* ioff, int max_polygons, int max_rings, int max_vertices,
                                                                    const int32_t* flag, int32_t* counts, int32_t* status) {
    __shared__ int64_t red[FFP_SCAN_THREADS / 64];
    int64_t carry[3] = {0, 0, 0};
    for (int at = 0; at < B; at += FFP_SCAN_THREADS) {
        const int i = at + threadIdx.x;
        for (int k = 0; k < 3; ++k) {
            const int64_t ex = wg_excl((int64_t)(i < B ? pcount[4 * (int64_t)i + k] : 0), red, carry[k]);
            if (i < B) ioff[3 * (int64_t)i + k] = ex;
        }
    }
    if (threadIdx.x == 0) {
        for (int k = 0; k < 3; ++k) { ioff[3 * (int64_t)B + k] = carry[k]; counts[k] = p3_sat31(carry[k]); }
        status[0] = ((carry[0] > max_polygons || carry[1] > max_rings || carry[2] > max_vertices) ? 1 : 0) | *flag;
    }
}

__global__ __launch_bounds__(FFP_THREADS) void ffp_emit_kernel(int B, FfpImages im, FfpStage all, const int64_t* ioff, int max_polygons, int max_rings, int max_vertices,
                                                               float2* ring_pos, int64_t* ring_slice, int64_t* poly_rings, int32_t* poly_batch, float* poly_area) {
    const int b = blockIdx.x;
    const int32_t* pc = im.pcount + 4 * (int64_t)b;
    const int np = pc[0], nr = pc[1], nv = pc[2];
    if (np <= 0) return;
    const FfpStage st = ffp_stage_of(all, im.soff[b]);
    const int64_t po = ioff[3 * (int64_t)b], ro = ioff[3 * (int64_t)b + 1], vo = ioff[3 * (int64_t)b + 2];
    FFP_FOR(i, nv) { const int64_t g = vo + i; if (g < max_vertices) ring_pos[g] = st.pos[i]; }
    FFP_FOR(r, nr) { const int64_t g = ro + r; if (g < max_rings) { ring_slice[2 * g] = vo + st.ring[r].x; ring_slice[2 * g + 1] = vo + st.ring[r].y; } }
    FFP_FOR(p, np) {
        const int64_t g = po + p;
        if (g >= max_polygons) continue;
        poly_rings[2 * g] = ro + st.poly[p].x; poly_rings[2 * g + 1] = ro + st.poly[p].y;
        poly_batch[g] = b; poly_area[g] = st.area[p];
    }
}

// pixel (px, py) lies on an edge of the rounded rings [0, nr) of `ring`, or inside them by the even-odd rule over all of them.  ip[i - voff] is vertex i.
// A ring whose box (min x, min y, max x, max y) does not hold the pixel is skipped: the pixel is on none of its edges, and a ray from outside a closed ring
// crosses it an even number of times
__device__ __forceinline__ bool ffp_covered(const int2* ip, int voff, const int2* ring, const int4* rbox, int nr, int px, int py) {
    int par = 0;
    for (int r = 0; r < nr; ++r) {
        const int4 bx = rbox[r];
        if (px < bx.x || px > bx.z || py < bx.y || py > bx.w) continue;
        const int i0 = ring[r].x - voff, i1 = ring[r].y - voff;
        int2 a = ip[i0];
        for (int i = i0 + 1; i < i1; ++i) {
            const int2 c = ip[i];
            if (py >= min(a.y, c.y) && py <= max(a.y, c.y)) {          // an edge that does not reach the pixel's row neither holds the pixel nor crosses its ray
                const int64_t cr = (int64_t)(c.x - a.x) * (py - a.y) - (int64_t)(c.y - a.y) * (px - a.x);
                if (cr == 0 && px >= min(a.x, c.x) && px <= max(a.x, c.x)) return true;
                if ((a.y <= py) != (c.y <= py) && (c.y > a.y ? cr > 0 : cr < 0)) par ^= 1;
            }
            a = c;
        }
    }
    return par != 0;
}

#define FFP_PROB_VERTS 4096          // rounded vertices and rings of a polygon that are kept in LDS (48 KiB); a larger polygon reads them from the workspace
#define FFP_PROB_RINGS 512
#define FFP_PROB_THREADS 1024       // 16 waves on the polygon's window: the background polygon of an image is most of the image

__global__ __launch_bounds__(FFP_PROB_THREADS) void ffp_prob_kernel(int B, int H, int W, const float* indicator, FfpImages im, FfpStage all, const int64_t* ioff,
                                                               int max_polygons, double seg_thr, float* poly_prob, int32_t* poly_flags) {
    __shared__ double sacc[FFP_PROB_THREADS];
    __shared__ int scnt[FFP_PROB_THREADS];
    __shared__ float sbox[4][FFP_PROB_THREADS];
    __shared__ int2 sip[FFP_PROB_VERTS], sring[FFP_PROB_RINGS];
    __shared__ int4 srbox[FFP_PROB_RINGS];
    const int tid = threadIdx.x;
    const int64_t total = ioff[3 * (int64_t)B];
    for (int64_t g = blockIdx.x; g < total && g < max_polygons; g += gridDim.x) {
        int lo = 0, hi = B;          // the image of polygon g: the last b with ioff[b] <= g
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (ioff[3 * (int64_t)mid] <= g) lo = mid; else hi = mid; }
        const int b = lo, j = (int)(g - ioff[3 * (int64_t)b]);
        const FfpStage st = ffp_stage_of(all, im.soff[b]);
        const int r0 = st.poly[j].x, nr = st.poly[j].y - r0;
        const int v0 = st.ring[r0].x, v1 = st.ring[r0].y, vend = st.ring[r0 + nr - 1].y;
        float bx0 = INFINITY, by0 = INFINITY, bx1 = -INFINITY, by1 = -INFINITY;
        for (int i = v0 + tid; i < v1; i += FFP_PROB_THREADS) {
            const float2 p = st.pos[i];          // (row, col)
            bx0 = fminf(bx0, p.y); bx1 = fmaxf(bx1, p.y); by0 = fminf(by0, p.x); by1 = fmaxf(by1, p.x);
        }
        sbox[0][tid] = bx0; sbox[1][tid] = by0; sbox[2][tid] = bx1; sbox[3][tid] = by1;
        __syncthreads();
        for (int s = FFP_PROB_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s) {
                sbox[0][tid] = fminf(sbox[0][tid], sbox[0][tid + s]); sbox[1][tid] = fminf(sbox[1][tid], sbox[1][tid + s]);
                sbox[2][tid] = fmaxf(sbox[2][tid], sbox[2][tid + s]); sbox[3][tid] = fmaxf(sbox[3][tid], sbox[3][tid + s]);
            }
            __syncthreads();
        }
        bx0 = sbox[0][0]; by0 = sbox[1][0]; bx1 = sbox[2][0]; by1 = sbox[3][0];
        double acc = 0.0;
        int cnt = 0;
        // int(minx) < 0 or int(maxx) + 1 > W with int() truncating towards zero
        const bool outside = !(bx0 > -1.0f) || !(by0 > -1.0f) || !(bx1 < (float)W) || !(by1 < (float)H);
        if (!outside) {          // uniform
            const int minx = (int)bx0, miny = (int)by0, maxx = (int)bx1 + 1, maxy = (int)by1 + 1;
            const bool lds = vend - v0 <= FFP_PROB_VERTS && nr <= FFP_PROB_RINGS;          // uniform
            int2* ip = lds ? sip : st.ipos;
            int2* ring = lds ? sring : st.ring + r0;
            int4* rbox = lds ? srbox : st.rbox + r0;
            const int voff = lds ? v0 : 0;
            for (int i = v0 + tid; i < vend; i += FFP_PROB_THREADS) {          // np.round(coords - (minx, miny)) in the cropped window, moved back
                const float2 p = st.pos[i];
                ip[i - voff] = make_int2((int)rint((double)p.y - (double)minx) + minx, (int)rint((double)p.x - (double)miny) + miny);
            }
            __syncthreads();          // the workgroup's own writes, LDS or global, are visible to it
            for (int r = tid; r < nr; r += FFP_PROB_THREADS) {
                const int2 rg = st.ring[r0 + r];
                int4 bx = make_int4(0x7fffffff, 0x7fffffff, -0x7fffffff, -0x7fffffff);
                for (int i = rg.x; i < rg.y; ++i) {
                    const int2 p = ip[i - voff];
                    bx.x = min(bx.x, p.x); bx.y = min(bx.y, p.y); bx.z = max(bx.z, p.x); bx.w = max(bx.w, p.y);
                }
                rbox[r] = bx;
                if (lds) sring[r] = rg;
            }
            __syncthreads();
            const int ww = maxx - minx, wh = maxy - miny;
            const float* ind = indicator + (int64_t)b * H * W;
            for (int idx = tid; idx < ww * wh; idx += FFP_PROB_THREADS) {
                const int px = minx + idx % ww, py = miny + idx / ww;
                if (!ffp_covered(ip, voff, ring, rbox, 1, px, py)) continue;
                if (nr > 1 && ffp_covered(ip, voff, ring + 1, rbox + 1, nr - 1, px, py)) continue;
                acc += (double)ind[(int64_t)py * W + px];
                ++cnt;
            }
        }
        sacc[tid] = acc; scnt[tid] = cnt;
        __syncthreads();
        for (int s = FFP_PROB_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s) { sacc[tid] += sacc[tid + s]; scnt[tid] += scnt[tid + s]; }
            __syncthreads();
        }
        if (tid == 0) {
            const double prob = scnt[0] > 0 ? sacc[0] / (double)scnt[0] : 0.0;
            poly_prob[g] = (float)prob;
            poly_flags[g] = st.aflag[j] | (seg_thr < prob ? 0 : 2);
        }
        __syncthreads();          // the shared arrays are free again
    }
}

// ---------------------------------------------------------------------------------------------------------------- workspace
struct FfpWs {
    int64_t S;
    int32_t* slots;
    int32_t *flag, *pcount;          // cleared together before every run: [flag, soff)
    int64_t *soff, *ioff;
    FfpStage st;
    FfpGlobal g;
};
static FfpWs ffp_carve(int64_t V, int B, P3Carve& c) {
    FfpWs l;
    memset(&l, 0, sizeof l);
    if (V < 0 || B < 1) return l;
    const int64_t S = 3 * V + 4 * (int64_t)B, I = 2 * S + (int64_t)FFP_PAD * B;          // an image's slots: segments + 2 ends each + 4
    l.S = S; l.g.I = I;
    l.slots = c.take<int32_t>(B);
    l.flag = c.take<int32_t>(1);
    l.pcount = c.take<int32_t>(4 * (int64_t)B);
    l.soff = c.take<int64_t>((int64_t)B + 1);
    l.ioff = c.take<int64_t>(3 * ((int64_t)B + 1));
    l.st.pos = c.take<float2>(3 * S);
    l.st.ipos = c.take<int2>(3 * S);
    l.st.ring = c.take<int2>(S);
    l.st.poly = c.take<int2>(S);
    l.st.area = c.take<float>(S);
    l.st.aflag = c.take<int32_t>(S);
    l.st.rbox = c.take<int4>(S);
    l.g.rS = c.take<double>(2 * S);
    l.g.node = c.take<FfpPt>(I);
    l.g.eu = c.take<int32_t>(S);
    l.g.ev = c.take<int32_t>(S);
    l.g.elive = c.take<uint8_t>(S);
    l.g.fl = c.take<uint8_t>(2 * S);
    l.g.ints = c.take<int32_t>(10 * I);
    return l;
}

extern "C" int64_t p3_ffl_polygons_workspace_bytes(int64_t V, int B) {
    P3Carve c = {nullptr, 0};
    ffp_carve(V, B, c);
    return c.at;
}

extern "C" int p3_ffl_polygons(const float* out_pos, int64_t V, const int64_t* piece_slice, const int32_t* piece_batch, int Q, const float* indicator, int B, int H,
                               int W, double min_area, double seg_threshold, int force_fallback, int max_polygons, int max_rings, int max_vertices,
                               float* ring_pos, int64_t* ring_slice, int64_t* poly_rings, int32_t* poly_batch, float* poly_area, float* poly_prob,
                               int32_t* poly_flags, int32_t* image_status, int32_t* counts, int32_t* status, void* workspace, void* stream) {
    P3_CHECK(V >= 0 && Q >= 0 && max_polygons >= 0 && max_rings >= 0 && max_vertices >= 0, P3_EINVAL, "p3_ffl_polygons: a negative count (V, Q, capacities >= 0)");
    P3_CHECK(B >= 1 && H >= 2 && W >= 2 && (int64_t)H * W < ((int64_t)1 << 31), P3_EINVAL, "p3_ffl_polygons: bad map sizes (B >= 1, H, W >= 2, H W < 2^31)");
    P3_CHECK(3 * V + 4 * (int64_t)B < ((int64_t)1 << 29), P3_EINVAL, "p3_ffl_polygons: 3 V + 4 B must stay below 2^29");
    P3_CHECK(min_area == min_area && seg_threshold == seg_threshold, P3_EINVAL, "p3_ffl_polygons: a threshold is NaN (min_area, seg_threshold)");
    P3_CHECK(image_status && counts && status, P3_EINVAL, "p3_ffl_polygons: null pointer (image_status, counts, status)");
    P3_CHECK(Q == 0 || (piece_slice && piece_batch && out_pos), P3_EINVAL, "p3_ffl_polygons: null pointer (out_pos, piece_slice, piece_batch)");
    // host arrays: their values are checked here and the call is refused either way
    if (Q > 0 && (p3_host_array(piece_slice) || p3_host_array(piece_batch))) {
        if (p3_host_array(piece_batch))
            for (int q = 0; q < Q; ++q) P3_CHECK(piece_batch[q] >= 0 && piece_batch[q] < B, P3_EINVAL, "p3_ffl_polygons: piece_batch out of [0, B)");
        if (p3_host_array(piece_slice))
            for (int q = 0; q < Q; ++q)
                P3_CHECK(piece_slice[2 * q] >= 0 && piece_slice[2 * q] <= piece_slice[2 * q + 1] && piece_slice[2 * q + 1] <= V, P3_EINVAL,
                         "p3_ffl_polygons: a piece_slice row lies outside out_pos [0, V]");
        P3_CHECK(false, P3_EINVAL, "p3_ffl_polygons: piece_slice and piece_batch must be device memory");
    }
    P3_CHECK(indicator, P3_EINVAL, "p3_ffl_polygons: null pointer (indicator)");
    P3_CHECK((max_vertices == 0 || ring_pos) && (max_rings == 0 || ring_slice) && (max_polygons == 0 || (poly_rings && poly_batch && poly_area && poly_prob && poly_flags)),
             P3_EINVAL, "p3_ffl_polygons: null output with a capacity above 0");
    P3_CHECK(workspace, P3_EINVAL, "p3_ffl_polygons: null workspace (p3_ffl_polygons_workspace_bytes(V, B))");
    hipStream_t s = (hipStream_t)stream;
    P3Carve carve = {(char*)workspace, 0};
    const FfpWs l = ffp_carve(V, B, carve);
    FfpIn in = {(const float2*)out_pos, piece_slice, piece_batch, V, Q, B, H, W, min_area};
    FfpImages im = {l.slots, l.soff, l.S, l.pcount, image_status};
    P3_TRY(p3_memset(l.flag, 0, (char*)l.soff - (char*)l.flag, s));
    const int all_global = force_fallback ? 1 : 0;
    P3_TRY(p3_launch<ffp_count_kernel>(nullptr, B, FFP_THREADS, 0, s, in, l.slots, l.flag));
    P3_TRY(p3_launch<ffp_offsets_kernel>(nullptr, 1, FFP_SCAN_THREADS, 0, s, B, l.slots, l.soff));
    P3_TRY(p3_launch<ffp_lds_kernel>(force_fallback ? nullptr : "ffp_lds_kernel", B, FFP_THREADS, 0, s, in, im, l.st, all_global));
    P3_TRY(p3_launch<ffp_global_kernel>(force_fallback ? "ffp_global_kernel" : nullptr, B, FFP_THREADS, 0, s, in, im, l.st, l.g, all_global));
    P3_TRY(p3_launch<ffp_scan_kernel>(nullptr, 1, FFP_SCAN_THREADS, 0, s, B, l.pcount, l.ioff, max_polygons, max_rings, max_vertices, l.flag, counts, status));
    P3_TRY(p3_launch<ffp_emit_kernel>(nullptr, B, FFP_THREADS, 0, s, B, im, l.st, l.ioff, max_polygons, max_rings, max_vertices, (float2*)ring_pos, ring_slice, poly_rings,
                                      poly_batch, poly_area));
    if (max_polygons > 0) {
        const int grid = max_polygons < 4096 ? max_polygons : 4096;
        P3_TRY(p3_launch<ffp_prob_kernel>(nullptr, grid, FFP_PROB_THREADS, 0, s, B, H, W, indicator, im, l.st, l.ioff, max_polygons, seg_threshold, poly_prob,
                                          poly_flags));
    }
    return P3_OK;
}
