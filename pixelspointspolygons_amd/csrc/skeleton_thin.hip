// p3hip - FFL active-skeleton initialisation from the segmentation map, on the device: init_method "skeleton_device" (DESIGN.md section 20 and the header
// comment of p3_skeleton_from_seg in include/p3hip.h hold the definition).  The reference's route (predict/ffl/polygonize_asm.py:655-675 compute_skeletons,
// get_skeleton: skimage binary_closing, skimage skeletonize, skan.Skeleton) is restated as: edge mask, pad 2, closing by the 3 x 3 cross, Zhang-Suen thinning,
// crop, the link rule, maximal degree-2 chains.
//
// Three launches whatever the data, no memset, no host synchronisation:
//   1 st_bitmap   ONE workgroup per image.  The working image (H+4) x (W+4) lives bit-packed in LDS, 32 pixels a word, two planes.  Edge bits: a wave takes 64
//                 pixels of a row, __ballot packs them.  Closing and thinning work on whole words: a neighbour in the row is a shift with the carry of the next
//                 word, B (the neighbour count) is a bit-sliced 4-bit counter, A == 1 (one 0 -> 1 step) is "some step and no second step".  A sub-iteration
//                 reads one plane and writes the other, one barrier each, and __syncthreads_or says whether a pixel went.  Then the pad is cleared and pixels
//                 without a neighbour go: the bitmap (working frame, pad = 0).  The graph is read off it where it lies, in LDS, a thread per word:
//                 chains   from every pixel of degree != 2, along every link, to the next pixel of degree != 2; the interior pixels are marked in the free
//                          plane; the reading is kept or not; the word's kept paths and slots are summed;
//                 cycles   a degree-2 pixel no chain marked lies on a cycle; it walks on until it is back (it is the smallest: the start) or meets a
//                          smaller pixel (it is not).
//                 A chain never leaves its image, so one workgroup sees all of it.  A walk is serial, one lane, and its time is steps x the latency of a
//                 step: where the CU's LDS takes them beside the planes (ST_LDS_MAX: up to 354 x 354, or 358 x 350) every skeleton pixel's link mask is written out
//                 once as a byte, and a step is one LDS byte read and a dozen instructions; a larger image reads the nine bits of the bitmap at every step.
//   2 st_scan     one workgroup: exclusive scans of nodes, paths and slots over the words, which is raster order image after image, which is node order:
//                 every word's first node id, first path number and first slot.  batch_delim, counts, status, the last path_delim entry.  The words are
//                 taken 1024 at a time by this one workgroup, B (H+4) ceil((W+4)/32) / 1024 passes one after the other: 29 at 16 x 224 x 224, 8 for one 508 x 508 image, and about 16 000 at the 2^29 pixels the entry accepts at most.  It is not split into a
//                 scan per image and one over the B totals; a batch of hundreds of large images pays for that here.
//   3 st_emit     one workgroup per image, the bitmap and the words' first node ids in LDS, a thread per word: pos / degrees / batch of its nodes, and its
//                 kept paths, walked once more and written.
// Inside an image a pixel's raster index orders like its node id, so 1 compares pixel indices and no node id exists before 2.  A node id is (first id of the
// word) + (set bits below the pixel in the word).
// A link mask has bit k for direction k of NW, N, NE, W, E, SW, S, SE: ascending neighbour id, and 7 - k is the way back.  It holds a pixel's
// neighbours instead of a list of their ids and comes from nine bits of the bitmap; no link mask has more than four bits (a diagonal link needs both
// 4-neighbours beside it empty).  What passes from 1 to 3 is a byte a pixel: the links along which a kept path starts.
// Every output element has one writer.  The one atomic is an or in LDS (interior marks: both readings set the same bits).  The longest path is a maximum over
// the workgroup (wg_max), one entry an image written by one thread, and 2 takes the maximum of the B entries: no word of the workspace is written by two blocks.
// Walks are bounded by the pixel count of the working image whatever the bitmap holds.
#include "p3_common.h"

#pragma clang fp contract(off)

typedef unsigned long long st_u64;

#define ST_BITMAP_THREADS 1024
#define ST_SCAN_THREADS 1024
#define ST_MAX_SIDE 512          // H + 4 and W + 4: two planes of 512 x 16 words are 64 KB of LDS
#define ST_LDS_MAX (160 * 1024 - 512)          // what a workgroup may ask of the CU's LDS
#define ST_LDS_PAD 64            // bytes: the largest image then asks for more than 64 KB and p3_launch raises the kernel's limit

struct StIn {
    const float* seg;
    int64_t sb, sc;
    int B, C, H, W;
    float level;
};
struct StWs {
    uint32_t* bitmap;          // [B][H+4][WW]
    uint8_t* kept;             // [B][H+4][W+4], written and read at skeleton pixels only: the links of a pixel along which a kept path starts
    st_u64* tot;               // [words] kept (paths << 32 | slots) of a word, after st_scan those in front of it
    int* node0;                // [words] nodes in front of a word
    int* longest;              // [B] the longest kept path of every image
};
struct StDim { int B, Hp, Wp, WW; };

__device__ __forceinline__ int st_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }
// direction k of NW, N, NE, W, E, SW, S, SE: its row and column step, and its raster index step
__device__ __forceinline__ int st_dr(int k) { return k < 3 ? -1 : (k < 5 ? 0 : 1); }
__device__ __forceinline__ int st_dc(int k) { return (k == 0 || k == 3 || k == 5) ? -1 : ((k == 1 || k == 6) ? 0 : 1); }
__device__ __forceinline__ int st_step(int k, int Wp) { return st_dr(k) * Wp + st_dc(k); }
// bit i of the result: the pixel west / east of bit i of x; lo / hi: the words before / behind x in the row
__device__ __forceinline__ uint32_t st_west(uint32_t x, uint32_t lo) { return (x << 1) | (lo >> 31); }
__device__ __forceinline__ uint32_t st_east(uint32_t x, uint32_t hi) { return (x >> 1) | (hi << 31); }

// step 1 of the definition at pixel (y, x) of the H x W image
__device__ __forceinline__ bool st_edge(const StIn& in, const float* img, int y, int x) {
    const int W = in.W, y0 = st_clamp(y - 1, in.H), y2 = st_clamp(y + 1, in.H), x0 = st_clamp(x - 1, W), x2 = st_clamp(x + 1, W);
    const float lv = in.level;
    const int64_t r0 = (int64_t)y0 * W, r1 = (int64_t)y * W, r2 = (int64_t)y2 * W;
    const float a00 = lv < img[r0 + x0] ? 1.f : 0.f, a01 = lv < img[r0 + x] ? 1.f : 0.f, a02 = lv < img[r0 + x2] ? 1.f : 0.f;
    const float a10 = lv < img[r1 + x0] ? 1.f : 0.f, a12 = lv < img[r1 + x2] ? 1.f : 0.f;
    const float a20 = lv < img[r2 + x0] ? 1.f : 0.f, a21 = lv < img[r2 + x] ? 1.f : 0.f, a22 = lv < img[r2 + x2] ? 1.f : 0.f;
    const float gx = ((a02 - a00) + 2.f * (a12 - a10) + (a22 - a20)) / 8.f, gy = ((a20 - a00) + 2.f * (a21 - a01) + (a22 - a02)) / 8.f;          // all exact
    float g = __fsqrt_rn((2.f * gx) * (2.f * gx) + (2.f * gy) * (2.f * gy));
    if (in.C >= 2) {
        const float v = img[in.sc + r1 + x] + g;
        g = v != v ? v : fminf(fmaxf(v, 0.f), 1.f);          // torch.clamp hands a NaN on
    }
    return lv < g;
}

// the 3 x 3 word neighbourhood of word (r, w) of a plane, as the eight neighbour words P2 .. P9 and the centre; outside the image reads as `fill`
struct StNb { uint32_t c, p2, p3, p4, p5, p6, p7, p8, p9; };
__device__ __forceinline__ uint32_t st_word(const uint32_t* pl, int r, int w, int Hp, int WW, uint32_t tail, uint32_t fill) {
    if (r < 0 || r >= Hp || w < 0 || w >= WW) return fill;
    const uint32_t x = pl[r * WW + w];
    return w == WW - 1 ? (x & tail) | (fill & ~tail) : x;
}
__device__ __forceinline__ StNb st_neigh(const uint32_t* pl, int r, int w, int Hp, int WW, uint32_t tail, uint32_t fill) {
    const uint32_t n0 = st_word(pl, r - 1, w - 1, Hp, WW, tail, fill), n1 = st_word(pl, r - 1, w, Hp, WW, tail, fill), n2 = st_word(pl, r - 1, w + 1, Hp, WW, tail, fill);
    const uint32_t c0 = st_word(pl, r, w - 1, Hp, WW, tail, fill), c1 = st_word(pl, r, w, Hp, WW, tail, fill), c2 = st_word(pl, r, w + 1, Hp, WW, tail, fill);
    const uint32_t s0 = st_word(pl, r + 1, w - 1, Hp, WW, tail, fill), s1 = st_word(pl, r + 1, w, Hp, WW, tail, fill), s2 = st_word(pl, r + 1, w + 1, Hp, WW, tail, fill);
    StNb n;
    n.c = c1;
    n.p2 = n1; n.p3 = st_east(n1, n2); n.p4 = st_east(c1, c2); n.p5 = st_east(s1, s2);
    n.p6 = s1; n.p7 = st_west(s1, s0); n.p8 = st_west(c1, c0); n.p9 = st_west(n1, n0);
    return n;
}
// the pixels of a word that a Zhang-Suen sub-iteration (0: the first, 1: the second) deletes
__device__ __forceinline__ uint32_t st_deleted(const StNb& n, int sub) {
    const uint32_t p[9] = {n.p2, n.p3, n.p4, n.p5, n.p6, n.p7, n.p8, n.p9, n.p2};
    uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, one = 0, two = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t c0 = s0 & p[k];          // B: a 4-bit counter in every bit lane
        s0 ^= p[k];
        const uint32_t c1 = s1 & c0;
        s1 ^= c0;
        const uint32_t c2 = s2 & c1;
        s2 ^= c1;
        s3 |= c2;
        const uint32_t t = ~p[k] & p[k + 1];          // A: the 0 -> 1 steps
        two |= one & t;
        one |= t;
    }
    const uint32_t b_ok = (s3 | s2 | s1) & ~s3 & ~(s2 & s1 & s0);          // 2 <= B <= 6
    const uint32_t cond = sub == 0 ? ~(n.p2 & n.p4 & n.p6) & ~(n.p4 & n.p6 & n.p8) : ~(n.p2 & n.p4 & n.p8) & ~(n.p2 & n.p6 & n.p8);
    return n.c & b_ok & one & ~two & cond;
}

// ---- the graph on a bitmap in LDS (working frame, pad = 0) ---------------------------------------------------------------------------------------------
struct StImg { const uint32_t* pl; const uint8_t* lk; int Hp, Wp, WW; };          // lk: NULL, or the link mask of every skeleton pixel, a byte each
struct StEnd { int r, c, d, n; };
// pixels c - 1, c, c + 1 of row r as bits 0, 1, 2; outside the image is 0.  The two loads are unconditional (clamped indices, the value masked afterwards), so
// the six loads of a link mask are in flight together: a step of a walk waits for LDS once
__device__ __forceinline__ uint32_t st_row3(const StImg& im, int r, int c) {
    const int s = c - 1, w = s >> 5;          // c >= 0: w >= -1
    const int rr = st_clamp(r, im.Hp) * im.WW;
    const uint32_t a = im.pl[rr + st_clamp(w, im.WW)], b = im.pl[rr + st_clamp(w + 1, im.WW)];
    const bool row = r >= 0 && r < im.Hp;
    const uint32_t lo = (row && w >= 0 && w < im.WW) ? a : 0u, hi = (row && w + 1 < im.WW) ? b : 0u;
    return (uint32_t)(((((st_u64)hi) << 32) | lo) >> (s & 31)) & 7u;
}
// the link mask of pixel (r, c): 4-neighbours, and a diagonal neighbour when both pixels beside the pair are empty
__device__ __forceinline__ uint32_t st_links(const StImg& im, int r, int c) {
    const uint32_t n = st_row3(im, r - 1, c), m = st_row3(im, r, c), s = st_row3(im, r + 1, c);
    const uint32_t nw = n & 1u, nn = (n >> 1) & 1u, ne = n >> 2, we = m & 1u, ea = m >> 2, sw = s & 1u, ss = (s >> 1) & 1u, se = s >> 2;
    return (nw & ~we & ~nn) | (nn << 1) | ((ne & ~nn & ~ea) << 2) | (we << 3) | (ea << 4) | ((sw & ~ss & ~we) << 5) | (ss << 6) | ((se & ~ea & ~ss) << 7);
}
// a walk's link mask: a byte read where the masks fit in LDS beside the planes (st_fill_links), else the nine bits again
__device__ __forceinline__ uint32_t st_lm(const StImg& im, int r, int c) { return im.lk ? im.lk[r * im.Wp + c] : st_links(im, r, c); }
__device__ __forceinline__ void st_fill_links(const StImg& im, uint8_t* lk) {          // all threads; a barrier has to follow
    for (int i = threadIdx.x; i < im.Hp * im.WW; i += blockDim.x) {
        const int r = i / im.WW, w = i - r * im.WW;
        for (uint32_t rest = im.pl[i]; rest; rest &= rest - 1) {
            const int c = 32 * w + __ffs(rest) - 1;
            lk[r * im.Wp + c] = (uint8_t)st_links(im, r, c);
        }
    }
}
// the chain from pixel (ur, uc) along link k: over degree-2 pixels to the first pixel of another degree, or back to the start.  -> the end pixel, d: the
// direction of the last step, n: the pixels of the reading, both ends counted (the start twice when it ends where it began).  marks: a bit plane that takes
// the interior pixels (an or: both readings set the same bits).  Bounded by the pixel count whatever the bitmap holds.
__device__ __forceinline__ StEnd st_chain(const StImg& im, uint32_t* marks, int ur, int uc, int k) {
    StEnd e = {ur + st_dr(k), uc + st_dc(k), k, 2};
    for (int t = 0; t < im.Hp * im.Wp && e.r >= 0 && e.r < im.Hp && e.c >= 0 && e.c < im.Wp; ++t) {
        const uint32_t lm = st_lm(im, e.r, e.c);
        const uint32_t nx = lm & ~(1u << (7 - e.d));
        if ((e.r == ur && e.c == uc) || __popc(lm) != 2 || !nx) break;
        atomicOr(&marks[e.r * im.WW + (e.c >> 5)], 1u << (e.c & 31));
        e.d = __ffs(nx) - 1;
        e.r += st_dr(e.d);
        e.c += st_dc(e.d);
        ++e.n;
    }
    return e;
}

// 1: grid B, dynamic LDS two planes
__global__ __launch_bounds__(ST_BITMAP_THREADS) void st_bitmap_kernel(StIn in, StWs ws, int link_bytes) {
    extern __shared__ uint32_t st_lds[];
    __shared__ int red[ST_BITMAP_THREADS / 64];
    const int b = blockIdx.x, H = in.H, W = in.W, Hp = H + 4, Wp = W + 4, WW = (Wp + 31) >> 5, words = Hp * WW;
    const uint32_t tail = (Wp & 31) ? (1u << (Wp & 31)) - 1u : ~0u;          // the pixels of a row's last word
    uint32_t *pa = st_lds, *pb = st_lds + words;
    const float* img = in.seg + (int64_t)b * in.sb;
    // edge mask of the padded image: a wave per 64 pixels of a row
    const int lane = threadIdx.x & 63, chunks = (Wp + 63) >> 6;
    for (int item = threadIdx.x >> 6; item < Hp * chunks; item += ST_BITMAP_THREADS / 64) {
        const int r = item / chunks, ch = item - r * chunks, c = ch * 64 + lane;
        const bool e = c < Wp && st_edge(in, img, st_clamp(r - 2, H), st_clamp(c - 2, W));
        const st_u64 bal = __ballot(e);
        if (lane == 0) {
            pa[r * WW + 2 * ch] = (uint32_t)bal;
            if (2 * ch + 1 < WW) pa[r * WW + 2 * ch + 1] = (uint32_t)(bal >> 32);
        }
    }
    __syncthreads();
    // closing: dilation (outside = 0), erosion (outside = 1), the 3 x 3 cross
    for (int i = threadIdx.x; i < words; i += ST_BITMAP_THREADS) {
        const int r = i / WW, w = i - r * WW;
        const StNb n = st_neigh(pa, r, w, Hp, WW, tail, 0u);
        const uint32_t d = n.c | n.p2 | n.p4 | n.p6 | n.p8;
        pb[i] = w == WW - 1 ? d & tail : d;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < words; i += ST_BITMAP_THREADS) {
        const int r = i / WW, w = i - r * WW;
        const StNb n = st_neigh(pb, r, w, Hp, WW, tail, ~0u);
        const uint32_t e = n.c & n.p2 & n.p4 & n.p6 & n.p8;
        pa[i] = w == WW - 1 ? e & tail : e;
    }
    __syncthreads();
    // thinning: rounds of two sub-iterations until one deletes nothing.  Every round but the last deletes a pixel: at most (foreground + 1) rounds.
    for (;;) {
        int gone = 0;
        for (int i = threadIdx.x; i < words; i += ST_BITMAP_THREADS) {
            const int r = i / WW, w = i - r * WW;
            const StNb n = st_neigh(pa, r, w, Hp, WW, tail, 0u);
            const uint32_t del = st_deleted(n, 0);
            pb[i] = n.c & ~del;
            gone |= del != 0;
        }
        const int g1 = __syncthreads_or(gone);
        gone = 0;
        for (int i = threadIdx.x; i < words; i += ST_BITMAP_THREADS) {
            const int r = i / WW, w = i - r * WW;
            const StNb n = st_neigh(pb, r, w, Hp, WW, tail, 0u);
            const uint32_t del = st_deleted(n, 1);
            pa[i] = n.c & ~del;
            gone |= del != 0;
        }
        const int g2 = __syncthreads_or(gone);
        if (!(g1 | g2)) break;
    }
    // crop: the pad goes (rows and columns 0, 1 and the last two)
    for (int i = threadIdx.x; i < words; i += ST_BITMAP_THREADS) {
        const int r = i / WW, w = i - r * WW;
        uint32_t keep = 0;
        if (r >= 2 && r < Hp - 2) {
            const int lo = 2 - 32 * w, hi = Wp - 2 - 32 * w;          // the kept columns of this word: [lo, hi)
            const uint32_t from = lo <= 0 ? ~0u : (lo >= 32 ? 0u : ~0u << lo), to = hi >= 32 ? ~0u : (hi <= 0 ? 0u : (1u << hi) - 1u);
            keep = from & to;
        }
        pb[i] = pa[i] & keep;
    }
    __syncthreads();
    // a pixel without any neighbour has no link and is no node
    for (int i = threadIdx.x; i < words; i += ST_BITMAP_THREADS) {
        const int r = i / WW, w = i - r * WW;
        const StNb n = st_neigh(pb, r, w, Hp, WW, tail, 0u);
        pa[i] = n.c & (n.p2 | n.p3 | n.p4 | n.p5 | n.p6 | n.p7 | n.p8 | n.p9);
    }
    __syncthreads();
    // the graph, read off the bitmap in pa; pb takes the marks of the chains' interior pixels
    for (int i = threadIdx.x; i < words; i += ST_BITMAP_THREADS) {
        ws.bitmap[(int64_t)b * words + i] = pa[i];
        pb[i] = 0;
    }
    uint8_t* lk = link_bytes ? (uint8_t*)(st_lds + 2 * words) : nullptr;
    const StImg im = {pa, lk, Hp, Wp, WW};
    if (lk) st_fill_links(im, lk);
    __syncthreads();
    const int64_t pix0 = (int64_t)b * Hp * Wp;
    int longest = 0;
    // chains: from every pixel of degree != 2, along every link, to the next pixel of degree != 2
    for (int i = threadIdx.x; i < words; i += ST_BITMAP_THREADS) {
        const int r = i / WW, w = i - r * WW;
        int paths = 0, slots = 0;
        for (uint32_t rest = pa[i]; rest; rest &= rest - 1) {
            const int c = 32 * w + __ffs(rest) - 1;
            const uint32_t lm = st_lm(im, r, c);
            uint32_t km = 0;
            if (__popc(lm) != 2) {
                for (uint32_t lr = lm; lr; lr &= lr - 1) {
                    const int k = __ffs(lr) - 1;
                    const StEnd e = st_chain(im, pb, r, c, k);
                    // the other reading starts at the end pixel v and goes back along the last step first
                    const int u = r * Wp + c, v = e.r * Wp + e.c;
                    if (u < v || (u == v && u + st_step(k, Wp) < v - st_step(e.d, Wp))) {
                        km |= 1u << k;
                        ++paths;
                        slots += e.n;
                        longest = max(longest, e.n - (u == v ? 1 : 0));
                    }
                }
            }
            ws.kept[pix0 + (int64_t)r * Wp + c] = (uint8_t)km;
        }
        ws.tot[(int64_t)b * words + i] = p3_pack2(paths, slots);
    }
    __syncthreads();
    // cycles: a degree-2 pixel that no chain marked walks on until it is back (it is the smallest of its cycle: the start) or meets a smaller pixel
    for (int i = threadIdx.x; i < words; i += ST_BITMAP_THREADS) {
        const int r = i / WW, w = i - r * WW;
        int paths = 0, slots = 0;
        for (uint32_t rest = pa[i] & ~pb[i]; rest; rest &= rest - 1) {
            const int c = 32 * w + __ffs(rest) - 1, u = r * Wp + c;
            const uint32_t lm = st_lm(im, r, c);
            if (__popc(lm) != 2) continue;
            const int k = __ffs(lm) - 1;          // the smaller neighbour
            int pr = r + st_dr(k), pc = c + st_dc(k), d = k, n = 1;
            bool smallest = true;
            for (int t = 0; t < Hp * Wp && !(pr == r && pc == c); ++t) {
                if (pr < 0 || pr >= Hp || pc < 0 || pc >= Wp) { smallest = false; break; }          // cannot happen: links lead to skeleton pixels
                const uint32_t nx = st_lm(im, pr, pc) & ~(1u << (7 - d));
                if (pr * Wp + pc < u || !nx) { smallest = false; break; }          // !nx cannot happen: links are symmetric
                d = __ffs(nx) - 1;
                pr += st_dr(d);
                pc += st_dc(d);
                ++n;
            }
            if (smallest && pr == r && pc == c) {
                ws.kept[pix0 + u] = (uint8_t)(1u << k);
                ++paths;
                slots += n + 1;
                longest = max(longest, n);
            }
        }
        if (paths) ws.tot[(int64_t)b * words + i] += p3_pack2(paths, slots);
    }
    longest = wg_max(longest, red);
    if (threadIdx.x == 0) ws.longest[b] = longest;
}

// 2: one workgroup
__global__ __launch_bounds__(ST_SCAN_THREADS) void st_scan_kernel(StDim dm, StWs ws, int max_nodes, int max_slots, int max_paths, int64_t* path_delim, int64_t* batch_delim,
                                                                  int32_t* counts, int32_t* status) {
    __shared__ st_u64 lds64[ST_SCAN_THREADS / 64];
    __shared__ int lds32[ST_SCAN_THREADS / 64];
    const int per = dm.Hp * dm.WW;
    const int64_t words = (int64_t)dm.B * per;
    st_u64 carry = 0;          // paths << 32 | slots
    int carry_nodes = 0;
    for (int64_t at = 0; at < words; at += ST_SCAN_THREADS) {
        const int64_t i = at + threadIdx.x;
        const st_u64 v = i < words ? ws.tot[i] : 0ull;
        const int nv = i < words ? __popc(ws.bitmap[i]) : 0;
        const st_u64 ex = wg_excl(v, lds64, carry);
        const int exn = wg_excl(nv, lds32, carry_nodes);
        if (i < words) {
            ws.tot[i] = ex;
            ws.node0[i] = exn;
            if (i % per == 0) batch_delim[i / per] = p3_hi32(ex);
        }
    }
    int longest = 0;
    for (int b = threadIdx.x; b < dm.B; b += ST_SCAN_THREADS) longest = max(longest, ws.longest[b]);
    longest = wg_max(longest, lds32);
    if (threadIdx.x == 0) {
        const int paths = p3_hi32(carry), slots = p3_lo32(carry);
        batch_delim[dm.B] = paths;
        counts[0] = carry_nodes; counts[1] = slots; counts[2] = paths; counts[3] = longest;
        status[0] = (carry_nodes > max_nodes || slots > max_slots || paths > max_paths) ? 1 : 0;
        if (paths > 0 && paths <= max_paths) path_delim[paths] = slots;          // path_delim has max_paths + 1 entries
    }
}

// 3: grid B, dynamic LDS: the image's bitmap and every word's first node id
__global__ __launch_bounds__(ST_BITMAP_THREADS) void st_emit_kernel(StDim dm, StWs ws, int max_nodes, int max_slots, int max_paths, float2* pos, int64_t* degrees,
                                                                    int64_t* path_index, int64_t* path_delim, int64_t* batch, int link_bytes) {
    extern __shared__ uint32_t st_lds[];
    const int b = blockIdx.x, Hp = dm.Hp, Wp = dm.Wp, WW = dm.WW, words = Hp * WW;
    uint32_t* pl = st_lds;
    int* node0 = (int*)(st_lds + words);
    for (int i = threadIdx.x; i < words; i += ST_BITMAP_THREADS) {
        pl[i] = ws.bitmap[(int64_t)b * words + i];
        node0[i] = ws.node0[(int64_t)b * words + i];
    }
    __syncthreads();
    uint8_t* lk = link_bytes ? (uint8_t*)(st_lds + 2 * words) : nullptr;
    const StImg im = {pl, lk, Hp, Wp, WW};
    if (lk) {
        st_fill_links(im, lk);
        __syncthreads();
    }
    const int64_t pix0 = (int64_t)b * Hp * Wp;
    for (int i = threadIdx.x; i < words; i += ST_BITMAP_THREADS) {
        const uint32_t x = pl[i];
        if (!x) continue;
        const int r = i / WW, w = i - r * WW;
        const st_u64 first = ws.tot[(int64_t)b * words + i];
        int id = node0[i], q = p3_hi32(first), at = p3_lo32(first);
        for (uint32_t rest = x; rest; rest &= rest - 1, ++id) {
            const int c = 32 * w + __ffs(rest) - 1;
            if (id < max_nodes) {
                pos[id] = make_float2((float)(r - 2), (float)(c - 2));
                degrees[id] = __popc(st_lm(im, r, c));
                batch[id] = b;
            }
            for (uint32_t kr = ws.kept[pix0 + (int64_t)r * Wp + c]; kr; kr &= kr - 1, ++q) {
                if (q < max_paths) path_delim[q] = at;
                if (at < max_slots) path_index[at] = id;
                ++at;
                int d = __ffs(kr) - 1, pr = r + st_dr(d), pc = c + st_dc(d);
                for (int t = 0; t < Hp * Wp && pr >= 0 && pr < Hp && pc >= 0 && pc < Wp; ++t) {
                    const int wi = pr * WW + (pc >> 5);
                    if (at < max_slots) path_index[at] = node0[wi] + __popc(pl[wi] & ((1u << (pc & 31)) - 1u));
                    ++at;
                    const uint32_t lp = st_lm(im, pr, pc);
                    const uint32_t nx = lp & ~(1u << (7 - d));
                    if ((pr == r && pc == c) || __popc(lp) != 2 || !nx) break;
                    d = __ffs(nx) - 1;
                    pr += st_dr(d);
                    pc += st_dc(d);
                }
            }
        }
    }
}

static StWs st_carve(int B, int H, int W, P3Carve& c) {
    StWs l;
    const int64_t b = B > 0 ? B : 0, Hp = (int64_t)H + 4, Wp = (int64_t)W + 4, words = b * Hp * ((Wp + 31) >> 5), pix = b * Hp * Wp;
    l.bitmap = c.take<uint32_t>(words);
    l.kept = c.take<uint8_t>(pix);
    l.tot = c.take<st_u64>(words);
    l.node0 = c.take<int>(words);
    l.longest = c.take<int>(b);
    return l;
}

extern "C" int64_t p3_skeleton_from_seg_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H < 1 || W < 1) return 0;
    P3Carve c = {nullptr, 0};
    st_carve(B, H, W, c);
    return c.at;
}

extern "C" int p3_skeleton_from_seg(const float* seg, int B, int C, int H, int W, int64_t stride_b, int64_t stride_c, double level, int max_nodes, int max_slots,
                                    int max_paths, float* out_pos, int64_t* degrees, int64_t* path_index, int64_t* path_delim, int64_t* batch, int64_t* batch_delim,
                                    int32_t* counts, int32_t* status, void* workspace, void* stream) {
    P3_CHECK(B >= 0 && C >= 1 && H >= 1 && W >= 1 && max_nodes >= 0 && max_slots >= 0 && max_paths >= 0, P3_ESHAPE,
             "p3_skeleton_from_seg: bad sizes (B >= 0; C, H, W >= 1; capacities >= 0)");
    P3_CHECK(H + 4 <= ST_MAX_SIDE && W + 4 <= ST_MAX_SIDE, P3_ESHAPE, "p3_skeleton_from_seg: H + 4 and W + 4 must not exceed 512 (two bit planes in 64 KB of LDS)");
    P3_CHECK((int64_t)B * (H + 4) * (W + 4) < ((int64_t)1 << 29), P3_ESHAPE, "p3_skeleton_from_seg: B (H + 4) (W + 4) must stay below 2^29");
    P3_CHECK(batch_delim && counts && status, P3_EINVAL, "p3_skeleton_from_seg: null pointer");
    P3_CHECK(B == 0 || (seg && path_delim && workspace), P3_EINVAL, "p3_skeleton_from_seg: null pointer");
    P3_CHECK(B == 0 || ((max_nodes == 0 || (out_pos && degrees && batch)) && (max_slots == 0 || path_index)), P3_EINVAL,
             "p3_skeleton_from_seg: null output with a capacity above 0");
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) {
        P3_TRY(p3_memset(batch_delim, 0, sizeof(int64_t), s));
        P3_TRY(p3_memset(counts, 0, 4 * sizeof(int32_t), s));
        return p3_memset(status, 0, sizeof(int32_t), s);
    }
    StIn in;
    in.seg = seg; in.sb = stride_b; in.sc = stride_c; in.B = B; in.C = C; in.H = H; in.W = W; in.level = (float)level;
    P3Carve carve = {(char*)workspace, 0};
    const StWs ws = st_carve(B, H, W, carve);
    StDim dm;
    dm.B = B; dm.Hp = H + 4; dm.Wp = W + 4; dm.WW = (dm.Wp + 31) >> 5;
    size_t lds = 2 * (size_t)dm.Hp * dm.WW * sizeof(uint32_t) + ST_LDS_PAD;          // two bit planes; in st_emit the bitmap and an int a word
    const size_t with_links = lds + (((size_t)dm.Hp * dm.Wp + 3) & ~(size_t)3);              // and a link mask byte a pixel behind them where the CU's 160 KB take it
    const int link_bytes = with_links <= ST_LDS_MAX ? 1 : 0;
    if (link_bytes) lds = with_links;
    P3_TRY(p3_launch<st_bitmap_kernel>(nullptr, B, ST_BITMAP_THREADS, lds, s, in, ws, link_bytes));
    P3_TRY(p3_launch<st_scan_kernel>(nullptr, 1, ST_SCAN_THREADS, 0, s, dm, ws, max_nodes, max_slots, max_paths, path_delim, batch_delim, counts, status));
    return p3_launch<st_emit_kernel>(nullptr, B, ST_BITMAP_THREADS, lds, s, dm, ws, max_nodes, max_slots, max_paths, (float2*)out_pos, degrees, path_index, path_delim, batch,
                                     link_bytes);
}
