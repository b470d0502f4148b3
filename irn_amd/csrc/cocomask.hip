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
