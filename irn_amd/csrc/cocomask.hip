// COCO run-length code of binary masks on the GPU (include/irn_hip.h "COCO mask encoding"): the arithmetic behind
// step/make_cocoann.py — per mask the run lengths in column-major pixel order, the area and the tight box.
//
// The masks are row-major and the code is column-major.  A workgroup owns one (mask, strip of 64 columns): lane l of
// every wave owns column l of the strip, so the 64 lanes of a wave read 64 consecutive bytes of one row, and the four
// waves split the rows of the column into four segments.  A thread's piece (column x, rows y0..y1-1) is a contiguous
// range of column-major positions j = x*h + y; the pieces of a strip are ordered by (column, segment) and the strips by
// their index, so a run that crosses a piece, a column seam or a strip seam needs only the pixel before the piece.
//
//   k_rle_count  every piece: number of 0<->1 transitions, position of its last transition, area and box partials;
//                pieces and strip totals go to scratch
//   k_rle_scan   one wave per mask: exclusive prefix of the strips' transition counts and the running maximum of their
//                last transition; n_runs = transitions + 1, area, bbox
//   k_rle_emit   every piece again: its first transition is count number (transitions before it), and every transition
//                at position p closes the run that began at the previous transition: counts[k] = p - prev
//
// Integers only; every output word has one writer, so the result is bit-reproducible by construction.
//
// The second half of the file traces the same masks' boundaries into polygons (k_poly_*, described there).
#include "common.hpp"

#include <climits>

using irn::fail;

namespace {

constexpr int COLS = 64;                  // columns of a strip: one per lane
constexpr int SEGS = 4;                   // row segments of a column: one per wave
constexpr int TPB = COLS * SEGS;
constexpr int STRIP_WORDS = 8;            // transitions, last transition, area, x0, x1, y0, y1, (pad)
constexpr int ROWS_AHEAD = 8;             // rows loaded before any of them is looked at

struct Scratch {
    int32_t *strip;                       // [n * S][STRIP_WORDS]
    int32_t *pre;                         // [n * S][2]: transitions before the strip, last transition before the strip
    int32_t *piece;                       // [n * S][TPB][2]: transitions, last transition (0 = none)
};

inline int strips(int w) { return (w + COLS - 1) / COLS; }

inline Scratch carve(void *scratch, int n, int w) {
    const size_t ns = (size_t)n * strips(w);
    Scratch s;
    s.strip = static_cast<int32_t *>(scratch);
    s.pre = s.strip + ns * STRIP_WORDS;
    s.piece = s.pre + ns * 2;
    return s;
}

struct Piece {
    const uint8_t *col;                   // &mask[0][x]
    int x, y0, y1, prev;                  // prev: the pixel before the piece in column-major order (0 before the mask)
    bool live;
};

__device__ inline Piece piece_of(const uint8_t *masks, int h, int w, int S) {
    const int b = blockIdx.x, m = b / S, s = b - m * S;
    const int lane = threadIdx.x & (COLS - 1), seg = threadIdx.x / COLS;
    const int rows = h / SEGS + (h % SEGS != 0);
    Piece p;
    const int64_t x = (int64_t)s * COLS + lane;            // beyond int32 only past the last column
    p.x = (int)min(x, (int64_t)w);
    p.y0 = (int)min((int64_t)seg * rows, (int64_t)h);
    p.y1 = p.y0 + min(rows, h - p.y0);
    p.live = x < w && p.y0 < p.y1;
    p.prev = 0;
    p.col = nullptr;
    if (p.live) {
        const uint8_t *mask = masks + (size_t)m * h * w;
        p.col = mask + p.x;
        if (p.y0 > 0) p.prev = p.col[(size_t)(p.y0 - 1) * w] != 0;
        else if (p.x > 0) p.prev = mask[(size_t)(h - 1) * w + p.x - 1] != 0;
    }
    return p;
}

// f(y, bit, changed) for every row of the piece, top to bottom
template <class F>
__device__ inline void walk(const Piece &p, int w, F &&f) {
    int prev = p.prev;
    for (int y = p.y0; y < p.y1; y += ROWS_AHEAD) {
        uint8_t v[ROWS_AHEAD];
#pragma unroll
        for (int k = 0; k < ROWS_AHEAD; ++k) v[k] = y + k < p.y1 ? p.col[(size_t)(y + k) * w] : 0;
#pragma unroll
        for (int k = 0; k < ROWS_AHEAD; ++k) {
            if (y + k >= p.y1) break;
            const int bit = v[k] != 0;
            f(y + k, bit, bit != prev);
            prev = bit;
        }
    }
}

__global__ void __launch_bounds__(TPB) k_rle_count(const uint8_t *__restrict__ masks, int h, int w, int S,
                                                   int32_t *__restrict__ strip, int32_t *__restrict__ piece) {
    __shared__ int s_cnt, s_last, s_area, s_x0, s_x1, s_y0, s_y1;
    if (threadIdx.x == 0) {
        s_cnt = s_last = s_area = 0;
        s_x0 = s_y0 = INT_MAX;
        s_x1 = s_y1 = -1;
    }
    __syncthreads();
    const Piece p = piece_of(masks, h, w, S);
    int cnt = 0, last = 0, area = 0, ya = INT_MAX, yb = -1;
    if (p.live) {
        const int pos0 = p.x * h;
        walk(p, w, [&](int y, int bit, bool changed) {
            if (changed) {
                ++cnt;
                last = pos0 + y;
            }
            if (bit) {
                ++area;
                ya = min(ya, y);
                yb = y;
            }
        });
    }
    const size_t id = (size_t)blockIdx.x * TPB + threadIdx.x;
    piece[id * 2] = cnt;
    piece[id * 2 + 1] = last;
    if (cnt) {
        atomicAdd(&s_cnt, cnt);
        atomicMax(&s_last, last);
    }
    if (area) {
        atomicAdd(&s_area, area);
        atomicMin(&s_x0, p.x);
        atomicMax(&s_x1, p.x);
        atomicMin(&s_y0, ya);
        atomicMax(&s_y1, yb);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t *r = strip + (size_t)blockIdx.x * STRIP_WORDS;
        r[0] = s_cnt, r[1] = s_last, r[2] = s_area, r[3] = s_x0, r[4] = s_x1, r[5] = s_y0, r[6] = s_y1, r[7] = 0;
    }
}

__global__ void __launch_bounds__(64) k_rle_scan(int S, const int32_t *__restrict__ strip, int32_t *__restrict__ pre,
                                                 int32_t *__restrict__ n_runs, int64_t *__restrict__ area,
                                                 int32_t *__restrict__ bbox) {
    const int m = blockIdx.x, lane = threadIdx.x;
    int carry_cnt = 0, carry_last = 0;
    long long a = 0;
    int x0 = INT_MAX, x1 = -1, y0 = INT_MAX, y1 = -1;
    for (int base = 0; base < S; base += 64) {
        const int s = base + lane;
        int cnt = 0, last = 0;
        if (s < S) {
            const int32_t *r = strip + ((size_t)m * S + s) * STRIP_WORDS;
            cnt = r[0], last = r[1];
            a += r[2];
            x0 = min(x0, r[3]), x1 = max(x1, r[4]), y0 = min(y0, r[5]), y1 = max(y1, r[6]);
        }
        int inc = cnt, mx = last;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int c = __shfl_up(inc, d, 64), l = __shfl_up(mx, d, 64);
            if (lane >= d) {
                inc += c;
                mx = max(mx, l);
            }
        }
        const int before = __shfl_up(mx, 1, 64);
        if (s < S) {
            int32_t *o = pre + ((size_t)m * S + s) * 2;
            o[0] = carry_cnt + inc - cnt;
            o[1] = max(carry_last, lane ? before : 0);
        }
        carry_cnt += __shfl(inc, 63, 64);
        carry_last = max(carry_last, __shfl(mx, 63, 64));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a += __shfl_xor(a, d, 64);
        x0 = min(x0, __shfl_xor(x0, d, 64)), x1 = max(x1, __shfl_xor(x1, d, 64));
        y0 = min(y0, __shfl_xor(y0, d, 64)), y1 = max(y1, __shfl_xor(y1, d, 64));
    }
    if (lane == 0) {
        n_runs[m] = carry_cnt + 1;
        area[m] = a;
        int32_t *b = bbox + (size_t)m * 4;
        if (a) b[0] = x0, b[1] = y0, b[2] = x1 - x0 + 1, b[3] = y1 - y0 + 1;
        else b[0] = b[1] = b[2] = b[3] = 0;
    }
}

__global__ void __launch_bounds__(TPB) k_rle_emit(const uint8_t *__restrict__ masks, int h, int w, int S,
                                                  const int32_t *__restrict__ pre, const int32_t *__restrict__ piece,
                                                  const int64_t *__restrict__ offsets, uint32_t *__restrict__ counts) {
    __shared__ int sc[TPB], sl[TPB];
    const int tid = threadIdx.x, lane = tid & (COLS - 1), seg = tid / COLS;
    const int order = lane * SEGS + seg;                   // pieces in column-major order
    const size_t id = (size_t)blockIdx.x * TPB + tid;
    sc[order] = piece[id * 2];
    sl[order] = piece[id * 2 + 1];
    __syncthreads();
    if (tid < COLS) {                                      // wave 0: lane = column, exclusive scan over the strip's pieces
        int c[SEGS], l[SEGS], tot = 0, mx = 0;
#pragma unroll
        for (int k = 0; k < SEGS; ++k) {
            c[k] = sc[tid * SEGS + k], l[k] = sl[tid * SEGS + k];
            tot += c[k];
            mx = max(mx, l[k]);
        }
        int inc = tot, imx = mx;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int cc = __shfl_up(inc, d, 64), ll = __shfl_up(imx, d, 64);
            if (tid >= d) {
                inc += cc;
                imx = max(imx, ll);
            }
        }
        int ec = inc - tot, el = __shfl_up(imx, 1, 64);
        if (tid == 0) el = 0;
#pragma unroll
        for (int k = 0; k < SEGS; ++k) {
            sc[tid * SEGS + k] = ec, sl[tid * SEGS + k] = el;
            ec += c[k];
            el = max(el, l[k]);
        }
    }
    __syncthreads();
    const Piece p = piece_of(masks, h, w, S);
    if (!p.live) return;
    const int m = blockIdx.x / S;
    const int64_t off = offsets[m], room = offsets[m + 1] - off;      // a count beyond the caller's room is not written
    uint32_t *out = counts + off;
    int64_t k = (int64_t)pre[(size_t)blockIdx.x * 2] + sc[order];
    int prev = max(pre[(size_t)blockIdx.x * 2 + 1], sl[order]);
    const int pos0 = p.x * h;
    walk(p, w, [&](int y, int, bool changed) {
        if (changed) {
            const int pos = pos0 + y;
            if (k < room) out[k] = (uint32_t)(pos - prev);
            ++k;
            prev = pos;
        }
    });
    if (p.x == w - 1 && p.y1 == h && k < room) out[k] = (uint32_t)(h * w - prev);   // the run that reaches the end
}

// h*w + 1 counts must fit an int32, and so must the grid
bool shape_ok(int n, int h, int w) {
    return n >= 0 && h >= 1 && w >= 1 && (int64_t)h * w < (int64_t)INT_MAX && (int64_t)n * strips(w) <= (int64_t)INT_MAX;
}

}  // namespace

extern "C" size_t irn_mask_rle_scratch_bytes(int n, int h, int w) {
    if (!shape_ok(n, h, w)) {
        fail(IRN_ERR_ARG, "irn_mask_rle_scratch_bytes: bad argument (n=%d, h=%d, w=%d; h*w < 2^31 - 1)", n, h, w);
        return 0;
    }
    return (size_t)n * strips(w) * (STRIP_WORDS + 2 + 2 * TPB) * sizeof(int32_t);
}

extern "C" int irn_mask_rle_count(const uint8_t *masks_dev, int n, int h, int w, int32_t *n_runs_dev, int64_t *area_dev,
                                  int32_t *bbox_dev, void *scratch_dev, void *stream) {
    if (!shape_ok(n, h, w) || (n > 0 && (!masks_dev || !n_runs_dev || !area_dev || !bbox_dev || !scratch_dev)))
        return fail(IRN_ERR_ARG, "irn_mask_rle_count: bad argument (n=%d, h=%d, w=%d; h*w < 2^31 - 1, no null pointer)", n,
                    h, w);
    if (n == 0) return IRN_OK;
    const int S = strips(w);
    const Scratch s = carve(scratch_dev, n, w);
    hipLaunchKernelGGL(k_rle_count, dim3(n * S), dim3(TPB), 0, (hipStream_t)stream, masks_dev, h, w, S, s.strip, s.piece);
    IRN_LAUNCH_CHECK("k_rle_count");
    hipLaunchKernelGGL(k_rle_scan, dim3(n), dim3(64), 0, (hipStream_t)stream, S, s.strip, s.pre, n_runs_dev, area_dev,
                       bbox_dev);
    IRN_LAUNCH_CHECK("k_rle_scan");
    return IRN_OK;
}

extern "C" int irn_mask_rle_emit(const uint8_t *masks_dev, int n, int h, int w, const int64_t *offsets_dev,
                                 uint32_t *counts_dev, void *scratch_dev, void *stream) {
    if (!shape_ok(n, h, w) || (n > 0 && (!masks_dev || !offsets_dev || !counts_dev || !scratch_dev)))
        return fail(IRN_ERR_ARG, "irn_mask_rle_emit: bad argument (n=%d, h=%d, w=%d; h*w < 2^31 - 1, no null pointer)", n,
                    h, w);
    if (n == 0) return IRN_OK;
    const int S = strips(w);
    const Scratch s = carve(scratch_dev, n, w);
    hipLaunchKernelGGL(k_rle_emit, dim3(n * S), dim3(TPB), 0, (hipStream_t)stream, masks_dev, h, w, S, s.pre, s.piece,
                       offsets_dev, counts_dev);
    IRN_LAUNCH_CHECK("k_rle_emit");
    return IRN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Polygon segmentations (include/irn_hip.h "COCO mask polygons"): the boundary of a mask along pixel edges as closed
// integer loops, outer loops emitted as their corners.
//
// A grid point (x, y), 0 <= x <= w, 0 <= y <= h, is the top-left corner of pixel (x, y).  It owns two edge positions: the
// horizontal unit segment to (x+1, y) (x < w) and the vertical one to (x, y+1) (y < h).  A position holds a directed edge
// when the two pixels across it differ, with the mask on the edge's right: +x above a set pixel, -x below one, +y right of
// one, -y left of one.  Directions are numbered 0 +x, 1 +y, 2 -x, 3 -y, so that a right turn is d+1 and a left turn d+3.
//
//   k_poly_count   a thread per grid point, 256 to a workgroup: the edges the point owns (0..2), their exclusive prefix
//                  inside the workgroup (uint16) and the workgroup's sum
//   k_scan_sums    one workgroup: exclusive scan of the workgroup sums; every mask's first edge number       [read-back 1]
//   k_poly_link    a thread per grid point again: the dense number of each of its edges, and per edge its successor (right
//                  turn, else straight on, else left turn at the head vertex), the head vertex, whether the successor
//                  turns (a corner), the shoelace term and the jumping label (own number for +x, INT_MAX for the others)
//   k_poly_jump    R launches: label = min(label, label[jump]), jump = jump[jump]; then every edge knows the lowest +x
//                  edge of its loop, the start edge
//   k_poly_cut     the edge in front of a start edge ends its list
//   k_poly_rank    R launches of Wyllie's ranking: corners and doubled area from an edge to the end of its list
//   k_poly_loops   per start edge (corners if outer, 1 if outer, 1 if hole), scanned inside workgroups of 256 edges
//   k_scan_sums    the workgroup sums of the three columns
//   k_poly_totals  a thread per mask: loops, holes, corners                                                  [read-back 2]
//   k_poly_emit    a thread per edge: the corner at the head of an outer loop's turning edge goes to
//                  xy[first corner of the loop + corners before it]; a start edge writes its loop's size     [read-back 3]
//
// R = ceil(log2(most edges of one mask)), made even, comes from read-back 1.  No kernel waits for another workgroup, no
// thread follows a chain: every loop in device code is bounded by a launch argument, and an index read from memory is
// range-checked before it is used, so a wrong `succ` gives wrong corners and nothing else.  Integers only, one writer per
// output word.
// The work is some thirty dependent launches over a few thousand words each: launch- and latency-bound.
// ---------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int PTS = 256;                  // grid points, and later edges, per workgroup
constexpr int SCAN_TPB = 1024;            // the one workgroup of k_scan_sums

struct GridScratch {                      // sized by (n, h, w)
    int32_t *bsum;                        // [NB + 1]: edges before the workgroup, after the scan; [NB] = all edges
    uint16_t *lpre;                       // [NB * PTS]: edges before the grid point inside its workgroup
};

struct TraceScratch {                     // sized by the number of edges
    int64_t *area[2];                     // shoelace terms from the edge to the end of its list
    int32_t *succ, *hx, *hy;
    int32_t *lab[2], *nxt[2], *cnt[2];    // jumping label; jump pointer, then list pointer; corners to the end of the list
    int32_t *sums;                        // [3][NBE + 1]: corners, outer loops, holes before the workgroup of edges
    uint8_t *turn;
};

inline int64_t grid_points(int h, int w) { return ((int64_t)h + 1) * ((int64_t)w + 1); }
inline int64_t blocks_per_mask(int h, int w) { return (grid_points(h, w) + PTS - 1) / PTS; }

// two edge positions per grid point must fit an int32 over the whole call
bool poly_shape_ok(int n, int h, int w) {
    return shape_ok(n, h, w) && (int64_t)n * blocks_per_mask(h, w) * PTS * 2 <= (int64_t)INT_MAX;
}

inline GridScratch carve_grid(void *scratch, int n, int h, int w) {
    const size_t nb = (size_t)n * blocks_per_mask(h, w);
    GridScratch g;
    g.bsum = static_cast<int32_t *>(scratch);
    g.lpre = reinterpret_cast<uint16_t *>(g.bsum + irn::round_up(nb + 1, 4));
    return g;
}

inline size_t edge_blocks(int n_edges) { return ((size_t)n_edges + PTS - 1) / PTS; }
inline size_t edge_room(int n_edges) { return irn::round_up((size_t)n_edges + 1, 64); }

inline TraceScratch carve_trace(void *scratch, int n_edges) {
    const size_t e = edge_room(n_edges);
    TraceScratch t;
    t.area[0] = static_cast<int64_t *>(scratch);
    t.area[1] = t.area[0] + e;
    int32_t *p = reinterpret_cast<int32_t *>(t.area[1] + e);
    t.succ = p, t.hx = p + e, t.hy = p + 2 * e;
    t.lab[0] = p + 3 * e, t.lab[1] = p + 4 * e;
    t.nxt[0] = p + 5 * e, t.nxt[1] = p + 6 * e;
    t.cnt[0] = p + 7 * e, t.cnt[1] = p + 8 * e;
    t.sums = p + 9 * e;
    t.turn = reinterpret_cast<uint8_t *>(t.sums + irn::round_up(3 * (edge_blocks(n_edges) + 1), 64));
    return t;
}

inline size_t trace_bytes(int n_edges) {
    return edge_room(n_edges) * (2 * sizeof(int64_t) + 9 * sizeof(int32_t) + 1) +
           irn::round_up(3 * (edge_blocks(n_edges) + 1), 64) * sizeof(int32_t);
}

// exclusive prefix of v over the workgroup's threads in thread order; total = the workgroup's sum.  TPB / 64 <= 64 waves.
template <int TPB_>
__device__ inline int block_scan(int v, int &total) {
    __shared__ int s_wave[TPB_ / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(inc, d, 64);
        if (lane >= d) inc += u;
    }
    __syncthreads();                                       // the previous use of s_wave is over
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < TPB_ / 64; ++k) {
        const int t = s_wave[k];
        if (k < wave) before += t;
        all += t;
    }
    total = all;
    return before + inc - v;
}

struct Pixels {
    const uint8_t *mask;
    int h, w;
    __device__ int operator()(int x, int y) const {
        return x >= 0 && y >= 0 && x < w && y < h && mask[(size_t)y * w + x] != 0;
    }
};

struct Point {
    int m, x, y;                          // mask, grid point
    bool live;
};

__device__ inline Point point_of(int h, int w, int bpm) {
    const int b = blockIdx.x, m = b / bpm;
    const int64_t r = (int64_t)(b - m * bpm) * PTS + threadIdx.x;
    Point p;
    p.m = m;
    p.live = r < ((int64_t)h + 1) * (w + 1);
    p.y = p.live ? (int)(r / (w + 1)) : 0;
    p.x = p.live ? (int)(r - (int64_t)p.y * (w + 1)) : 0;
    return p;
}

// the edges grid point (x, y) owns: bit 0 horizontal, bit 1 vertical
__device__ inline int owned(const Pixels &px, int x, int y) {
    const int d = px(x, y);
    const int hor = x < px.w && px(x, y - 1) != d;
    const int ver = y < px.h && px(x - 1, y) != d;
    return hor | ver << 1;
}

__global__ void __launch_bounds__(PTS) k_poly_count(const uint8_t *__restrict__ masks, int h, int w, int bpm,
                                                    int32_t *__restrict__ bsum, uint16_t *__restrict__ lpre) {
    const Point p = point_of(h, w, bpm);
    const Pixels px{masks + (size_t)p.m * h * w, h, w};
    const int own = p.live ? owned(px, p.x, p.y) : 0;
    int total;
    const int before = block_scan<PTS>((own & 1) + (own >> 1), total);
    lpre[(size_t)blockIdx.x * PTS + threadIdx.x] = (uint16_t)before;
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// s[c][0 .. nb]: in-place exclusive scan of the nb sums of every column, the column's total at [nb].  One workgroup.
// With moff: moff[m] = s[0][m * bpm] for m = 0 .. n.
__global__ void __launch_bounds__(SCAN_TPB) k_scan_sums(int32_t *__restrict__ s, int nb, int ncol, int32_t *__restrict__ moff,
                                                         int n, int bpm) {
    for (int c = 0; c < ncol; ++c) {
        int32_t *col = s + (size_t)c * ((size_t)nb + 1);
        int carry = 0;
        for (int base = 0; base < nb; base += SCAN_TPB) {
            const int i = base + (int)threadIdx.x;
            const int v = i < nb ? col[i] : 0;
            int total;
            const int before = block_scan<SCAN_TPB>(v, total);
            if (i < nb) col[i] = carry + before;
            carry += total;
        }
        if (threadIdx.x == 0) col[nb] = carry;
    }
    if (moff) {
        __syncthreads();
        for (int m = threadIdx.x; m <= n; m += SCAN_TPB) moff[m] = s[(size_t)m * bpm];
    }
}

__global__ void __launch_bounds__(PTS) k_poly_link(const uint8_t *__restrict__ masks, int h, int w, int bpm, int n_edges,
                                                   const int32_t *__restrict__ bsum, const uint16_t *__restrict__ lpre,
                                                   int32_t *__restrict__ succ, int32_t *__restrict__ hx, int32_t *__restrict__ hy,
                                                   uint8_t *__restrict__ turn, int32_t *__restrict__ lab, int32_t *__restrict__ jump,
                                                   int32_t *__restrict__ cnt, int64_t *__restrict__ area) {
    const Point p = point_of(h, w, bpm);
    if (!p.live) return;
    const Pixels px{masks + (size_t)p.m * h * w, h, w};
    const int own = owned(px, p.x, p.y);
    if (!own) return;
    const int first = bsum[blockIdx.x] + lpre[(size_t)blockIdx.x * PTS + threadIdx.x];
    const int set = px(p.x, p.y);
    // the dense number of an edge position of this mask: grid point (x, y), vertical or horizontal
    auto number = [&](int x, int y, bool vertical) {
        const int64_t r = (int64_t)y * (w + 1) + x;
        const int b = p.m * bpm + (int)(r / PTS);
        int e = bsum[b] + lpre[(size_t)b * PTS + (int)(r % PTS)];
        if (vertical) e += x < w && px(x, y - 1) != px(x, y);
        return e;
    };
    for (int k = 0; k < 2; ++k) {
        if (!(own >> k & 1)) continue;
        const int e = first + (k == 1 && (own & 1));
        if (e < 0 || e >= n_edges) continue;               // the caller's room is smaller than the mask's edges
        // direction, head vertex and shoelace term x0*y1 - x1*y0
        int d, vx, vy;
        int64_t term;
        if (k == 0) {
            d = set ? 0 : 2;                               // +x above a set pixel, -x below one
            vx = set ? p.x + 1 : p.x, vy = p.y;
            term = set ? -(int64_t)p.y : (int64_t)p.y;
        } else {
            d = set ? 3 : 1;                               // -y left of a set pixel, +y right of one
            vx = p.x, vy = set ? p.y : p.y + 1;
            term = set ? -(int64_t)p.x : (int64_t)p.x;
        }
        const int nw = px(vx - 1, vy - 1), ne = px(vx, vy - 1), sw = px(vx - 1, vy), se = px(vx, vy);
        const bool out[4] = {se && !ne, sw && !se, nw && !sw, ne && !nw};      // the edges that leave the head vertex
        int nd = (d + 1) & 3;
        if (!out[nd]) nd = d;
        if (!out[nd]) nd = (d + 3) & 3;
        int s = e;                                         // (an edge always has a successor; a list of one otherwise)
        if (out[nd]) s = nd == 0 ? number(vx, vy, false) : nd == 1 ? number(vx, vy, true) : nd == 2 ? number(vx - 1, vy, false)
                                                                                                   : number(vx, vy - 1, true);
        if (s < 0 || s >= n_edges) s = e;
        succ[e] = s, jump[e] = s;
        hx[e] = vx, hy[e] = vy;
        turn[e] = nd != d;
        cnt[e] = nd != d;
        area[e] = term;
        lab[e] = d == 0 ? e : INT_MAX;
    }
}

__device__ inline bool in_range(int i, int n) { return i >= 0 && i < n; }

__global__ void __launch_bounds__(PTS) k_poly_jump(int n_edges, const int32_t *__restrict__ lab_in, const int32_t *__restrict__ jump_in,
                                                   int32_t *__restrict__ lab_out, int32_t *__restrict__ jump_out) {
    const int e = blockIdx.x * PTS + threadIdx.x;
    if (e >= n_edges) return;
    int j = jump_in[e];
    if (!in_range(j, n_edges)) j = e;
    lab_out[e] = min(lab_in[e], lab_in[j]);
    const int jj = jump_in[j];
    jump_out[e] = in_range(jj, n_edges) ? jj : e;
}

__global__ void __launch_bounds__(PTS) k_poly_cut(int n_edges, const int32_t *__restrict__ succ, const int32_t *__restrict__ lab,
                                                  int32_t *__restrict__ nxt) {
    const int e = blockIdx.x * PTS + threadIdx.x;
    if (e >= n_edges) return;
    const int s = succ[e];
    nxt[e] = in_range(s, n_edges) && lab[s] != s ? s : -1;
}

__global__ void __launch_bounds__(PTS) k_poly_rank(int n_edges, const int32_t *__restrict__ nxt_in, const int32_t *__restrict__ cnt_in,
                                                   const int64_t *__restrict__ area_in, int32_t *__restrict__ nxt_out,
                                                   int32_t *__restrict__ cnt_out, int64_t *__restrict__ area_out) {
    const int e = blockIdx.x * PTS + threadIdx.x;
    if (e >= n_edges) return;
    const int j = nxt_in[e];
    const bool go = in_range(j, n_edges);
    cnt_out[e] = cnt_in[e] + (go ? cnt_in[j] : 0);
    area_out[e] = area_in[e] + (go ? area_in[j] : 0);
    nxt_out[e] = go ? nxt_in[j] : -1;
}

// per workgroup of edges: exclusive prefixes of (corners of outer loops, outer loops, holes) over its start edges
__global__ void __launch_bounds__(PTS) k_poly_loops(int n_edges, int nbe, const int32_t *__restrict__ lab, const int32_t *__restrict__ cnt,
                                                    const int64_t *__restrict__ area, int32_t *__restrict__ pre_v,
                                                    int32_t *__restrict__ pre_l, int32_t *__restrict__ pre_h, int32_t *__restrict__ sums) {
    const int e = blockIdx.x * PTS + threadIdx.x;
    const bool start = e < n_edges && lab[e] == e;
    const int64_t a = start ? area[e] : 0;
    const int outer = a > 0, hole = a < 0, corners = outer ? cnt[e] : 0;
    int tv, tl, th;
    const int bv = block_scan<PTS>(corners, tv), bl = block_scan<PTS>(outer, tl), bh = block_scan<PTS>(hole, th);
    if (e < n_edges) pre_v[e] = bv, pre_l[e] = bl, pre_h[e] = bh;
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = tv;
        sums[(size_t)(nbe + 1) + blockIdx.x] = tl;
        sums[(size_t)2 * (nbe + 1) + blockIdx.x] = th;
    }
}

// what lies before edge i in column c (i == n_edges: everything)
__device__ inline int before_edge(const int32_t *sums, const int32_t *pre, int nbe, int c, int i, int n_edges) {
    const int32_t *col = sums + (size_t)c * (nbe + 1);
    return i >= n_edges ? col[nbe] : col[i / PTS] + pre[i];
}

__global__ void __launch_bounds__(PTS) k_poly_totals(int n, int n_edges, int nbe, const int32_t *__restrict__ moff,
                                                     const int32_t *__restrict__ sums, const int32_t *__restrict__ pre_v,
                                                     const int32_t *__restrict__ pre_l, const int32_t *__restrict__ pre_h,
                                                     int32_t *__restrict__ n_loops, int32_t *__restrict__ n_holes,
                                                     int32_t *__restrict__ n_vertices) {
    const int m = blockIdx.x * PTS + threadIdx.x;
    if (m >= n) return;
    const int i0 = min(max(moff[m], 0), n_edges), i1 = min(max(moff[m + 1], i0), n_edges);
    n_vertices[m] = before_edge(sums, pre_v, nbe, 0, i1, n_edges) - before_edge(sums, pre_v, nbe, 0, i0, n_edges);
    n_loops[m] = before_edge(sums, pre_l, nbe, 1, i1, n_edges) - before_edge(sums, pre_l, nbe, 1, i0, n_edges);
    n_holes[m] = before_edge(sums, pre_h, nbe, 2, i1, n_edges) - before_edge(sums, pre_h, nbe, 2, i0, n_edges);
}

__global__ void __launch_bounds__(PTS) k_poly_emit(int n_edges, int nbe, const int32_t *__restrict__ lab, const int32_t *__restrict__ cnt,
                                                   const int64_t *__restrict__ area, const uint8_t *__restrict__ turn,
                                                   const int32_t *__restrict__ hx, const int32_t *__restrict__ hy,
                                                   const int32_t *__restrict__ sums, const int32_t *__restrict__ pre_v,
                                                   const int32_t *__restrict__ pre_l, int32_t *__restrict__ loop_sizes,
                                                   int64_t loops_room, int32_t *__restrict__ xy, int64_t xy_room) {
    const int e = blockIdx.x * PTS + threadIdx.x;
    if (e >= n_edges) return;
    const int s = lab[e];
    if (!in_range(s, n_edges) || lab[s] != s || area[s] <= 0) return;          // holes are counted, not written
    const int corners = cnt[s];
    if (e == s) {
        const int64_t at = before_edge(sums, pre_l, nbe, 1, s, n_edges);
        if (at < loops_room) loop_sizes[at] = corners;
    }
    if (!turn[e]) return;
    // corners from the start edge up to this one; the edge in front of the start edge carries the start vertex
    int k = corners - cnt[e] + 1;
    if (k == corners) k = 0;
    if (k < 0 || k >= corners) return;
    const int64_t at = (int64_t)before_edge(sums, pre_v, nbe, 0, s, n_edges) + k;
    if (at < xy_room) xy[2 * at] = hx[e], xy[2 * at + 1] = hy[e];
}

// 2^r >= longest, and r even: the double-buffered rounds then end in buffer 0 (a round past the last changes nothing)
inline int jump_rounds(int longest) {
    int r = 0;
    while (r < 31 && ((int64_t)1 << r) < longest) ++r;
    return r + (r & 1);
}

}  // namespace

extern "C" size_t irn_mask_polygon_scratch_bytes(int n, int h, int w) {
    if (!poly_shape_ok(n, h, w)) {
        fail(IRN_ERR_ARG, "irn_mask_polygon_scratch_bytes: bad argument (n=%d, h=%d, w=%d; h*w < 2^31 - 1, 2*n*(h+1)*(w+1) < 2^31)",
             n, h, w);
        return 0;
    }
    if (n == 0) return 0;
    const size_t nb = (size_t)n * blocks_per_mask(h, w);
    return irn::round_up(nb + 1, 4) * sizeof(int32_t) + nb * PTS * sizeof(uint16_t);
}

extern "C" size_t irn_mask_polygon_trace_scratch_bytes(int n_edges) {
    if (n_edges < 0) {
        fail(IRN_ERR_ARG, "irn_mask_polygon_trace_scratch_bytes: bad argument (n_edges=%d)", n_edges);
        return 0;
    }
    return n_edges ? trace_bytes(n_edges) : 0;
}

extern "C" int irn_mask_polygon_edges(const uint8_t *masks_dev, int n, int h, int w, int32_t *edge_offsets_dev,
                                      void *scratch_dev, void *stream) {
    if (!poly_shape_ok(n, h, w) || (n > 0 && (!masks_dev || !edge_offsets_dev || !scratch_dev)))
        return fail(IRN_ERR_ARG,
                    "irn_mask_polygon_edges: bad argument (n=%d, h=%d, w=%d; h*w < 2^31 - 1, 2*n*(h+1)*(w+1) < 2^31, no null pointer)",
                    n, h, w);
    if (n == 0) return IRN_OK;
    const int bpm = (int)blocks_per_mask(h, w), nb = n * bpm;
    const GridScratch g = carve_grid(scratch_dev, n, h, w);
    hipLaunchKernelGGL(k_poly_count, dim3(nb), dim3(PTS), 0, (hipStream_t)stream, masks_dev, h, w, bpm, g.bsum, g.lpre);
    IRN_LAUNCH_CHECK("k_poly_count");
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(SCAN_TPB), 0, (hipStream_t)stream, g.bsum, nb, 1, edge_offsets_dev, n, bpm);
    IRN_LAUNCH_CHECK("k_scan_sums");
    return IRN_OK;
}

extern "C" int irn_mask_polygon_count(const uint8_t *masks_dev, int n, int h, int w, const int32_t *edge_offsets_dev,
                                      int n_edges, int max_mask_edges, int32_t *n_loops_dev, int32_t *n_holes_dev,
                                      int32_t *n_vertices_dev, void *scratch_dev, void *trace_scratch_dev, void *stream) {
    if (!poly_shape_ok(n, h, w) || n_edges < 0 || max_mask_edges < 0 || max_mask_edges > n_edges ||
        (n > 0 && (!masks_dev || !edge_offsets_dev || !n_loops_dev || !n_holes_dev || !n_vertices_dev || !scratch_dev)) ||
        (n > 0 && n_edges > 0 && !trace_scratch_dev))
        return fail(IRN_ERR_ARG,
                    "irn_mask_polygon_count: bad argument (n=%d, h=%d, w=%d, n_edges=%d, max_mask_edges=%d; h*w < 2^31 - 1, "
                    "2*n*(h+1)*(w+1) < 2^31, 0 <= max_mask_edges <= n_edges, no null pointer)", n, h, w, n_edges, max_mask_edges);
    if (n == 0) return IRN_OK;
    hipStream_t st = (hipStream_t)stream;
    if (n_edges == 0) {                                    // no mask has a pixel
        IRN_HIP_TRY(hipMemsetAsync(n_loops_dev, 0, (size_t)n * sizeof(int32_t), st));
        IRN_HIP_TRY(hipMemsetAsync(n_holes_dev, 0, (size_t)n * sizeof(int32_t), st));
        IRN_HIP_TRY(hipMemsetAsync(n_vertices_dev, 0, (size_t)n * sizeof(int32_t), st));
        return IRN_OK;
    }
    const int bpm = (int)blocks_per_mask(h, w), nb = n * bpm, nbe = (int)edge_blocks(n_edges);
    const GridScratch g = carve_grid(scratch_dev, n, h, w);
    const TraceScratch t = carve_trace(trace_scratch_dev, n_edges);
    hipLaunchKernelGGL(k_poly_link, dim3(nb), dim3(PTS), 0, st, masks_dev, h, w, bpm, n_edges, g.bsum, g.lpre, t.succ, t.hx, t.hy,
                       t.turn, t.lab[0], t.nxt[0], t.cnt[0], t.area[0]);
    IRN_LAUNCH_CHECK("k_poly_link");
    const int rounds = jump_rounds(max_mask_edges);
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(k_poly_jump, dim3(nbe), dim3(PTS), 0, st, n_edges, t.lab[r & 1], t.nxt[r & 1], t.lab[~r & 1], t.nxt[~r & 1]);
        IRN_LAUNCH_CHECK("k_poly_jump");
    }
    hipLaunchKernelGGL(k_poly_cut, dim3(nbe), dim3(PTS), 0, st, n_edges, t.succ, t.lab[0], t.nxt[0]);
    IRN_LAUNCH_CHECK("k_poly_cut");
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(k_poly_rank, dim3(nbe), dim3(PTS), 0, st, n_edges, t.nxt[r & 1], t.cnt[r & 1], t.area[r & 1], t.nxt[~r & 1],
                           t.cnt[~r & 1], t.area[~r & 1]);
        IRN_LAUNCH_CHECK("k_poly_rank");
    }
    // the list pointers and the other label buffer are free now: the three prefix columns
    int32_t *pre_v = t.lab[1], *pre_l = t.nxt[0], *pre_h = t.nxt[1];
    hipLaunchKernelGGL(k_poly_loops, dim3(nbe), dim3(PTS), 0, st, n_edges, nbe, t.lab[0], t.cnt[0], t.area[0], pre_v, pre_l, pre_h,
                       t.sums);
    IRN_LAUNCH_CHECK("k_poly_loops");
    hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(SCAN_TPB), 0, st, t.sums, nbe, 3, (int32_t *)nullptr, 0, 0);
    IRN_LAUNCH_CHECK("k_scan_sums");
    hipLaunchKernelGGL(k_poly_totals, dim3(irn::cdiv(n, PTS)), dim3(PTS), 0, st, n, n_edges, nbe, edge_offsets_dev, t.sums, pre_v, pre_l,
                       pre_h, n_loops_dev, n_holes_dev, n_vertices_dev);
    IRN_LAUNCH_CHECK("k_poly_totals");
    return IRN_OK;
}

extern "C" int irn_mask_polygon_emit(int n_edges, int32_t *loop_sizes_dev, int64_t loops_room, int32_t *xy_dev, int64_t xy_room,
                                     void *trace_scratch_dev, void *stream) {
    if (n_edges < 0 || loops_room < 0 || xy_room < 0 ||
        (n_edges > 0 && !trace_scratch_dev) || (loops_room > 0 && !loop_sizes_dev) || (xy_room > 0 && !xy_dev))
        return fail(IRN_ERR_ARG,
                    "irn_mask_polygon_emit: bad argument (n_edges=%d, loops_room=%lld, xy_room=%lld; none negative, no null pointer)",
                    n_edges, (long long)loops_room, (long long)xy_room);
    if (n_edges == 0) return IRN_OK;
    const int nbe = (int)edge_blocks(n_edges);
    const TraceScratch t = carve_trace(trace_scratch_dev, n_edges);
    hipLaunchKernelGGL(k_poly_emit, dim3(nbe), dim3(PTS), 0, (hipStream_t)stream, n_edges, nbe, t.lab[0], t.cnt[0], t.area[0], t.turn,
                       t.hx, t.hy, t.sums, t.lab[1], t.nxt[0], loop_sizes_dev, loops_room, xy_dev, xy_room);
    IRN_LAUNCH_CHECK("k_poly_emit");
    return IRN_OK;
}
