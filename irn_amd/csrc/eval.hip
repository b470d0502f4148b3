// Evaluation counts on the GPU (include/irn_hip.h "Evaluation counts"): the confusion matrices behind
// step/eval_cam.py and step/eval_sem_seg.py, the mask_iou counts behind step/eval_ins_seg.py, and the confusion matrices
// of a whole fg x bg threshold grid of IR labels (step/tune_ir_label.py; not in the reference), and the boundary bands and
// band counts of Boundary IoU / Boundary AP (--boundary_iou_ratio of the two label evaluation steps; not in the reference).
//
// Every kernel privatises its counters in LDS (one uint32 per bin, at most 4096 pixels per block, so a bin cannot
// overflow) and flushes the non-zero bins once per block with 64-bit integer atomics into the caller's int64
// accumulators.  Integer sums do not depend on arrival order: every result is exact and reproducible.  The threshold
// histogram of irn_cam_confusion is counted by thres_hist.hpp, the code the label sweep (label.hip) counts with.
#include "thres_hist.hpp"

#include <algorithm>
#include <cmath>

using irn::cdiv;
using irn::fail;
namespace thist = irn::thist;
using thist::add64, thist::gt_row, thist::kMaxKeys, thist::classes_ok;

namespace {

constexpr int TPB = 256;                  // threads per block
constexpr int PPT = 16;                   // pixels per thread (kept in registers by the CAM kernel)
constexpr int PIX = TPB * PPT;            // pixels per block: bin counts stay below 2^32
// ncls, everywhere below: classes including the background, a launch argument (2..IRN_EVAL_MAX_CLASSES)
constexpr int CAP = 16384;                // LDS bins of one pass of the CAM kernel (64 KiB)
static_assert(TPB == thist::kThreads, "thres_hist.hpp counts with blocks of this size");

// ---------------------------------------------------------------------------------------------------------------------
// CAM confusion, counting pass: per pixel the GT row, the first arg-max plane c and the maximum m; the bins and their
// counting are thres_hist.hpp's.  Without planes (k = 0) every pixel predicts class 0: one channel whose column is 0.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) k_cam_hist(const float *__restrict__ cam, const int64_t *__restrict__ keys, int k,
                                                  const uint8_t *__restrict__ gt, int n, const float *__restrict__ thres,
                                                  int t, int ncls, int64_t *__restrict__ hist,
                                                  int64_t *__restrict__ bad) {
    __shared__ uint32_t bins[CAP];
    __shared__ float th[IRN_EVAL_MAX_THRES];
    __shared__ int col[kMaxKeys];
    __shared__ uint32_t nbad;
    const int tid = threadIdx.x;
    if (k == 0 && tid == 0) col[0] = 0;
    uint32_t local_bad = thist::stage(thres, t, keys, k, blockIdx.x == 0, ncls, th, col, &nbad);

    const int kc = k > 0 ? k : 1;
    uint32_t bin[PPT];
    const int base = blockIdx.x * PIX + tid;
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        bin[i] = thist::kSkip;
        const int p = base + i * TPB;
        if (p >= n) continue;
        const int row = gt_row(gt[p], ncls);
        if (row < 0) {
            ++local_bad;
            continue;
        }
        if (k == 0) {
            bin[i] = thist::bin_of(0, row, 0, kc, ncls);
            continue;
        }
        float m = cam[p];
        bool nan = std::isnan(m);
        int c = 0;
        for (int ch = 1; ch < k; ++ch) {
            const float v = cam[(size_t)ch * n + p];
            nan |= std::isnan(v);
            if (v > m) {               // strict: the first plane that reaches the maximum keeps it (np.argmax)
                m = v;
                c = ch;
            }
        }
        if (nan) {
            ++local_bad;
            continue;
        }
        bin[i] = thist::bin_of(thist::count_below(th, t, m), row, c, kc, ncls);
    }
    local_bad += thist::count(bin, bins, CAP, (uint32_t)(t + 1) * (uint32_t)(ncls + 1) * (uint32_t)kc, kc, col, t, ncls, hist);
    thist::flush_bad(local_bad, &nbad, bad);
}

// hist [ncls+1][ncls][t+1] -> conf [t][ncls][ncls] (+ void [t][ncls]).  One thread per (row, column) of the histogram: a pixel of
// column c >= 1 and count j predicts c at thresholds 0..j-1 and 0 from j on; column 0 predicts 0 throughout.
__global__ void __launch_bounds__(TPB) k_cam_reduce(const int64_t *__restrict__ hist, int t, int NC,
                                                    int64_t *__restrict__ conf, int64_t *__restrict__ void_) {
    const int id = blockIdx.x * TPB + threadIdx.x;
    if (id >= (NC + 1) * NC) return;
    const int row = id / NC, c = id % NC;
    if (row == NC && !void_) return;
    const int64_t *h = hist + (size_t)id * (t + 1);
    int64_t tot = 0;
    for (int j = 0; j <= t; ++j) tot += h[j];
    if (tot == 0) return;
    auto at = [&](int i, int cl) -> int64_t * {
        return row < NC ? conf + ((size_t)i * NC + row) * NC + cl : void_ + (size_t)i * NC + cl;
    };
    int64_t above = 0;                 // pixels of this bin whose maximum lies above thres[i]
    for (int i = t - 1; i >= 0; --i) {
        above += c ? h[i + 1] : 0;
        if (above) *at(i, c) += above;                                 // the only writer of (i, row, c >= 1)
        if (tot - above)
            atomicAdd(reinterpret_cast<unsigned long long *>(at(i, 0)), (unsigned long long)(tot - above));
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// label confusion: bins [ncls+1][ncls] per block, in dynamic LDS sized by the call
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) k_label_hist(const uint8_t *__restrict__ pred, const uint8_t *__restrict__ gt, int n,
                                                    int map255, int NC, int64_t *__restrict__ conf,
                                                    int64_t *__restrict__ void_, int64_t *__restrict__ bad) {
    extern __shared__ uint32_t bins[];
    __shared__ uint32_t nbad;
    const int tid = threadIdx.x;
    const int n_bins = (NC + 1) * NC;
    for (int b = tid; b < n_bins; b += TPB) bins[b] = 0;
    if (tid == 0) nbad = 0;
    __syncthreads();
    uint32_t local_bad = 0;
    const int base = blockIdx.x * PIX + tid;
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        const int p = base + i * TPB;
        if (p >= n) continue;
        const int row = gt_row(gt[p], NC);
        int q = pred[p];
        if (q == 255 && map255 >= 0) q = map255;
        if (row < 0 || q >= NC) {
            ++local_bad;
            continue;
        }
        atomicAdd(&bins[row * NC + q], 1u);
    }
    if (local_bad) atomicAdd(&nbad, local_bad);
    __syncthreads();
    for (int b = tid; b < n_bins; b += TPB) {
        const uint32_t v = bins[b];
        if (!v) continue;
        if (b < NC * NC) add64(conf + b, v);
        else if (void_) add64(void_ + (b - NC * NC), v);
    }
    if (tid == 0 && nbad) add64(bad, nbad);
}

// ---------------------------------------------------------------------------------------------------------------------
// mask overlap: block (x, y) counts pixels of one pixel range by instance id, within mask y (y < n) or over the whole
// image (y == n: the GT areas and the range check of the instance map, done once)
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) k_mask_overlap(const uint8_t *__restrict__ masks, int n_masks,
                                                      const uint8_t *__restrict__ inst, int g, int n,
                                                      int64_t *__restrict__ inter, int64_t *__restrict__ area_pred,
                                                      int64_t *__restrict__ area_gt, int64_t *__restrict__ bad) {
    __shared__ uint32_t cnt[256];
    __shared__ uint32_t total;
    const int tid = threadIdx.x;
    const int y = blockIdx.y;
    cnt[tid] = 0;
    if (tid == 0) total = 0;
    __syncthreads();
    const uint8_t *mask = y < n_masks ? masks + (size_t)y * n : nullptr;
    uint32_t mine = 0;
    const int base = blockIdx.x * PIX + tid;
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        const int p = base + i * TPB;
        if (p >= n) continue;
        if (mask && !mask[p]) continue;
        ++mine;
        const uint8_t id = inst[p];
        if (id) atomicAdd(&cnt[id], 1u);
    }
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    const uint32_t v = cnt[tid];
    if (tid >= 1 && v) {
        if (tid > g) {
            if (!mask) add64(bad, v);                 // counted once, by the whole-image row
        } else if (mask) {
            add64(inter + (size_t)y * g + (tid - 1), v);
        } else {
            add64(area_gt + (tid - 1), v);
        }
    }
    if (tid == 0 && mask && total) add64(area_pred + y, total);
}

// ---------------------------------------------------------------------------------------------------------------------
// IR-label grid confusion: every (fg, bg) pair of a threshold grid from the CRF label planes, no label map written.
// The label of pair (i, j) is fgv if fgv != 0, else 0 if bgv == 0, else 255.  A pixel with fgv != 0 is in the same cell
// for every j, and one with fgv == 0 is in column 0 or ncls by j alone, so a block counts
//     az[i][row][v]   pixels whose plane fg[i] reads v (v = 0..ncls-1)
//     un[i][j][row]   those of them with v == 0 whose plane bg[j] is not 0 (the unsure ones)
// as uint32 in LDS (f*(ncls+1)*ncls + f*b*(ncls+1) words, sized by the launch's f and b: 51 KiB at 16 x 16 and 21 classes,
// 1.8 KiB at 2 x 2), f + (number of unsure pairs) atomics per pixel instead of f*b, and expands them when it flushes:
// column v >= 1 of every j gets az[i][row][v], column ncls gets un, column 0 gets az[i][row][0] - un.
// A launch counts the fg values i0 .. i0+f-1 of the call's grid: the host gives one launch as many as fit kIrLdsBytes
// (all 16 at 21 classes, 2 at 81) and loops over the rest.  Every cell of hist belongs to one fg value, so the grouping
// cannot change a count; the out-of-range pixels are the same in every launch and only the first one reports them.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int IR_MAX = IRN_CRF_MAX_SWEEP;     // planes, and pairs per axis
constexpr size_t kIrLdsBytes = 65536 - 64;    // dynamic LDS of a launch: what a workgroup gets without an attribute, less nbad

// words of LDS a launch over f fg values needs
constexpr size_t ir_lds_words(int f, int b, int ncls) { return (size_t)f * (ncls + 1) * ncls + (size_t)f * b * (ncls + 1); }
static_assert(ir_lds_words(IR_MAX, IR_MAX, IRN_EVAL_CLASSES) * 4 <= kIrLdsBytes, "a 16 x 16 grid at 21 classes is one launch");
static_assert(ir_lds_words(1, IR_MAX, IRN_EVAL_MAX_CLASSES) * 4 <= kIrLdsBytes, "one fg value always fits");

struct PairIdx {
    uint8_t fg[IR_MAX], bg[IR_MAX];
};

// four bytes of a plane from pixel p on: one 32-bit load where the address allows it (`valid` = pixels left, 1..4)
__device__ __forceinline__ uint32_t load4(const uint8_t *__restrict__ q, int valid) {
    if (valid == 4 && (reinterpret_cast<uintptr_t>(q) & 3) == 0) return *reinterpret_cast<const uint32_t *>(q);
    uint32_t v = 0;
    for (int k = 0; k < valid; ++k) v |= (uint32_t)q[k] << (8 * k);
    return v;
}

// KNC: the class count as a constant (the instantiation for IRN_EVAL_CLASSES: with run-time divisors in the flush a 16 x 16
// grid measured 2.6 % slower), or 0 = the launch argument.
template <int KNC>
__global__ void __launch_bounds__(TPB) k_ir_label_hist(const uint8_t *__restrict__ planes, int t_count, PairIdx idx, int i0,
                                                       int f, int b, int ncls, const uint8_t *__restrict__ gt, int n,
                                                       int64_t *__restrict__ hist, int64_t *__restrict__ bad) {
    extern __shared__ uint32_t lds[];
    __shared__ uint32_t nbad;
    const int tid = threadIdx.x;
    const int NC = KNC ? KNC : ncls;
    const int kRows = NC + 1, IR_COLS = NC + 1;   // rows: GT 0..ncls-1 and void; columns: labels 0..ncls-1 and 255
    const int n_az = f * kRows * NC, n_un = f * b * kRows;
    uint32_t *az = lds, *un = lds + n_az;
    for (int c = tid; c < n_az + n_un; c += TPB) lds[c] = 0;
    if (tid == 0) nbad = 0;
    __syncthreads();
    uint32_t local_bad = 0;
    const int base = blockIdx.x * PIX + tid * 4;
#pragma unroll 1
    for (int g = 0; g < PPT / 4; ++g) {
        const int p = base + g * TPB * 4;
        if (p >= n) break;
        const int valid = min(4, n - p);
        const uint32_t gw = load4(gt + p, valid);
        // which planes read 0 at each of the four pixels, and which pixels are out of range in any plane
        uint32_t zero[4] = {0, 0, 0, 0}, skip = 0;
        for (int t = 0; t < t_count; ++t) {
            const uint32_t w = load4(planes + (size_t)t * n + p, valid);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t v = (w >> (8 * k)) & 255u;
                zero[k] |= (v == 0 ? 1u : 0u) << t;
                skip |= (v > (uint32_t)(NC - 1) ? 1u : 0u) << k;
            }
        }
        int row[4];
        uint32_t unsure[4];                   // bit j: plane bg[j] is not 0
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            row[k] = gt_row((uint8_t)(gw >> (8 * k)), NC);
            if (k < valid && (row[k] < 0 || ((skip >> k) & 1u))) {
                ++local_bad;
                row[k] = -1;
            }
            if (k >= valid) row[k] = -1;
            unsure[k] = 0;
        }
        for (int j = 0; j < b; ++j) {
#pragma unroll
            for (int k = 0; k < 4; ++k) unsure[k] |= ((~zero[k] >> idx.bg[j]) & 1u) << j;
        }
        for (int i = 0; i < f; ++i) {
            const int ti = idx.fg[i0 + i];
            const uint32_t w = load4(planes + (size_t)ti * n + p, valid);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (row[k] < 0) continue;
                const uint32_t v = (w >> (8 * k)) & 255u;
                atomicAdd(&az[(i * kRows + row[k]) * NC + (int)v], 1u);
                if (v) continue;
                for (uint32_t m = unsure[k]; m; m &= m - 1)
                    atomicAdd(&un[(i * b + (__ffs(m) - 1)) * kRows + row[k]], 1u);
            }
        }
    }
    if (local_bad) atomicAdd(&nbad, local_bad);
    __syncthreads();
    // flush: one pass over az, a non-zero cell going to its column of every j
    for (int c = tid; c < n_az; c += TPB) {
        const uint32_t cnt = az[c];
        if (!cnt) continue;
        const int v = c % NC, ir = c / NC, r = ir % kRows, i = ir / kRows;
        for (int j = 0; j < b; ++j) {
            int64_t *cell = hist + (((size_t)(i0 + i) * b + j) * kRows + r) * IR_COLS;
            if (v) {
                add64(cell + v, cnt);
                continue;
            }
            const uint32_t u = un[(i * b + j) * kRows + r];
            if (cnt - u) add64(cell, cnt - u);
            if (u) add64(cell + NC, u);
        }
    }
    if (tid == 0 && nbad && i0 == 0) add64(bad, nbad);
}

// ---------------------------------------------------------------------------------------------------------------------
// Boundary bands (Boundary IoU; not in the reference, DESIGN.md "Boundary IoU"): band(L, d)[y][x] = 1 iff the square
// window |dy| <= d, |dx| <= d around (y, x) leaves the image or holds a byte other than L[y][x].  All 256 bytes are labels.
//
// A block owns a tile of BT_H x BT_W pixels and stages it with a halo of d cells in LDS (cells outside the image are told
// by their coordinates, never by a value).  The window is separable: a row pass marks every cell of the tile's columns
// (halo rows included) whose 2d+1 row segment is uniform and inside the image, a column pass marks the pixels whose 2d+1
// marked cells above and below carry the pixel's value.  Both are run-length scans, one thread per row (then per column),
// once in each direction: a cell's segment is uniform iff the run of equal cells that ends at it is longer than d from
// both sides.  That is 2 reads per staged cell and pass whatever d is, at the price of few busy threads (BT_H + 2d of 256
// in the row pass, BT_W in the column pass); the counting around it is what the rest of the block is for.
// LDS of a launch, sized by its d: the haloed tile (pitch x (BT_H+2d) bytes), the row flags (68 x (BT_H+2d)) and the
// tile's result (BT_H x BT_W): 10.8 KB at d = 12 (375x500 at ratio 0.02), 43.3 KB at the largest d, 64, where a block
// stages 160 x 192 cells for its 32 x 64 pixels (15x the pixels; 2.4x at d = 12).  A 64 x 64 tile would stage 9x there but
// take 53.5 KB and halve the blocks of an image.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int BT_W = 64, BT_H = 32;             // pixels of a tile
constexpr int BPT = BT_W * BT_H / TPB;          // pixels per thread: column tid % BT_W, rows tid / BT_W + (TPB / BT_W) * i
constexpr int BT_RSTEP = TPB / BT_W;
constexpr int FLAG_PITCH = BT_W + 4;            // 17 words: the row pass writes one column from many rows
static_assert(BPT * TPB == BT_W * BT_H && BT_RSTEP * BT_W == TPB && BPT <= 32, "a thread's pixels, and one bit for each");

// bytes between two rows of the haloed tile: a multiple of 4 with an odd word count (threads of the row pass read one
// column of many rows)
__host__ __device__ constexpr int band_pitch(int d) {
    const int p = (BT_W + 2 * d + 3) & ~3;
    return (p / 4) % 2 == 0 ? p + 4 : p;
}
__host__ __device__ constexpr size_t band_lds_bytes(int d) {
    return (size_t)(band_pitch(d) + FLAG_PITCH) * (BT_H + 2 * d) + BT_W * BT_H;
}
static_assert(band_lds_bytes(IRN_BAND_MAX_D) + 256 * 4 + 64 <= 65536, "the haloed tile of the largest d and the counters fit a workgroup");

// how a kernel reads the bytes it bands
struct AsLabel {
    __device__ int operator()(uint8_t v) const { return v; }
};
struct Map255 {                                   // a prediction: 255 reads as `as` when that is >= 0
    int as;
    __device__ int operator()(uint8_t v) const { return v == 255 && as >= 0 ? as : (int)v; }
};
struct AsMask {                                   // a mask: two values
    __device__ int operator()(uint8_t v) const { return v != 0; }
};

struct BandTile {
    const uint8_t *tile;      // haloed values: pixel (ty, tx) of the tile at tile[(ty + d) * pitch + tx + d]
    const uint8_t *inner;     // [BT_H][BT_W]: 1 = the whole window equals the pixel (not band)
    int pitch, d;
    __device__ int value(int ty, int tx) const { return tile[(ty + d) * pitch + tx + d]; }
    __device__ bool band(int ty, int tx) const { return !inner[ty * BT_W + tx]; }
};

// length of the run of equal in-image values that ends at a cell; v < 0 = outside the image (or, in the column pass, a
// cell whose row segment is not uniform)
__device__ __forceinline__ int run_step(int run, int prev, int v) { return v < 0 ? 0 : (v == prev ? run + 1 : 1); }

// Bands the tile at (x0, y0) of map[h][w], read through `read`, in `lds` (band_lds_bytes(d) bytes).  Every thread of the
// block calls it; it starts and ends with a barrier, so a second call may follow once the first result is in registers.
template <class Read>
__device__ BandTile band_tile(const uint8_t *__restrict__ map, Read read, int h, int w, int d, int x0, int y0, uint8_t *lds) {
    const int tid = threadIdx.x;
    const int pitch = band_pitch(d), rows = BT_H + 2 * d, cols = BT_W + 2 * d;
    uint8_t *tile = lds, *flag = lds + (size_t)pitch * rows, *inner = flag + (size_t)FLAG_PITCH * rows;
    __syncthreads();
    for (int r = tid / BT_W; r < rows; r += BT_RSTEP) {
        const int y = y0 - d + r;
        const bool row_in = y >= 0 && y < h;
        for (int c = tid % BT_W; c < cols; c += BT_W) {
            const int x = x0 - d + c;
            tile[r * pitch + c] = row_in && x >= 0 && x < w ? (uint8_t)read(map[(size_t)y * w + x]) : 0;
        }
    }
    __syncthreads();
    for (int r = tid; r < rows; r += TPB) {
        const int y = y0 - d + r;
        const bool row_in = y >= 0 && y < h;
        const uint8_t *t = tile + r * pitch;
        uint8_t *f = flag + r * FLAG_PITCH;
        int run = 0, prev = -1;
        for (int c = 0; c < d + BT_W; ++c) {
            const int x = x0 - d + c;
            const int v = row_in && x >= 0 && x < w ? (int)t[c] : -1;
            run = run_step(run, prev, v);
            prev = v;
            if (c >= d) f[c - d] = run > d;
        }
        run = 0, prev = -1;
        for (int c = cols - 1; c >= d; --c) {
            const int x = x0 - d + c;
            const int v = row_in && x >= 0 && x < w ? (int)t[c] : -1;
            run = run_step(run, prev, v);
            prev = v;
            if (c < d + BT_W) f[c - d] = f[c - d] && run > d;
        }
    }
    __syncthreads();
    for (int x = tid; x < BT_W; x += TPB) {
        int run = 0, prev = -1;
        for (int r = 0; r < d + BT_H; ++r) {
            const int v = flag[r * FLAG_PITCH + x] ? (int)tile[r * pitch + x + d] : -1;
            run = run_step(run, prev, v);
            prev = v;
            if (r >= d) inner[(r - d) * BT_W + x] = run > d;
        }
        run = 0, prev = -1;
        for (int r = rows - 1; r >= d; --r) {
            const int v = flag[r * FLAG_PITCH + x] ? (int)tile[r * pitch + x + d] : -1;
            run = run_step(run, prev, v);
            prev = v;
            if (r < d + BT_H) inner[(r - d) * BT_W + x] = inner[(r - d) * BT_W + x] && run > d;
        }
    }
    __syncthreads();
    return {tile, inner, pitch, d};
}

__global__ void __launch_bounds__(TPB) k_label_band(const uint8_t *__restrict__ map, int h, int w, int d, int tiles_x,
                                                    uint8_t *__restrict__ out) {
    extern __shared__ uint32_t band_lds[];        // band_lds_bytes(d) bytes, here and in the two kernels below
    const int x0 = (blockIdx.x % tiles_x) * BT_W, y0 = (blockIdx.x / tiles_x) * BT_H;
    const BandTile b = band_tile(map, AsLabel{}, h, w, d, x0, y0, reinterpret_cast<uint8_t *>(band_lds));
    const int tx = threadIdx.x % BT_W, x = x0 + tx;
#pragma unroll
    for (int i = 0; i < BPT; ++i) {
        const int ty = threadIdx.x / BT_W + BT_RSTEP * i, y = y0 + ty;
        if (y < h && x < w) out[(size_t)y * w + x] = b.band(ty, tx);
    }
}

// Semantic boundary counts: the prediction's band first (values and band bits into registers), then the GT's in the same
// LDS; bins [NC][3] = (both bands and the same class, prediction band, GT band).
__global__ void __launch_bounds__(TPB) k_label_boundary(const uint8_t *__restrict__ pred, const uint8_t *__restrict__ gt, int h,
                                                        int w, int d, int map255, int NC, int tiles_x,
                                                        int64_t *__restrict__ counts, int64_t *__restrict__ bad) {
    extern __shared__ uint32_t band_lds[];
    __shared__ uint32_t bins[3 * IRN_EVAL_MAX_CLASSES];
    __shared__ uint32_t nbad;
    const int tid = threadIdx.x;
    for (int b = tid; b < 3 * NC; b += TPB) bins[b] = 0;
    if (tid == 0) nbad = 0;
    uint8_t *lds = reinterpret_cast<uint8_t *>(band_lds);
    const int x0 = (blockIdx.x % tiles_x) * BT_W, y0 = (blockIdx.x / tiles_x) * BT_H;
    const int tx = tid % BT_W, x = x0 + tx;
    uint8_t pv[BPT];
    uint32_t pband = 0;
    {
        const BandTile p = band_tile(pred, Map255{map255}, h, w, d, x0, y0, lds);
#pragma unroll
        for (int i = 0; i < BPT; ++i) {
            const int ty = tid / BT_W + BT_RSTEP * i;
            pv[i] = (uint8_t)p.value(ty, tx);
            pband |= (p.band(ty, tx) ? 1u : 0u) << i;
        }
    }
    const BandTile g = band_tile(gt, AsLabel{}, h, w, d, x0, y0, lds);
    uint32_t local_bad = 0;
#pragma unroll
    for (int i = 0; i < BPT; ++i) {
        const int ty = tid / BT_W + BT_RSTEP * i;
        if (y0 + ty >= h || x >= w) continue;
        const int row = gt_row((uint8_t)g.value(ty, tx), NC), q = pv[i];
        if (row < 0 || q >= NC) {
            ++local_bad;
            continue;
        }
        if (row == NC) continue;              // void: a label when the GT band was formed, counted nowhere
        const bool pb = (pband >> i) & 1u, gb = g.band(ty, tx);
        if (gb) atomicAdd(&bins[row * 3 + 2], 1u);
        if (pb) atomicAdd(&bins[q * 3 + 1], 1u);
        if (pb && gb && q == row) atomicAdd(&bins[row * 3], 1u);
    }
    if (local_bad) atomicAdd(&nbad, local_bad);
    __syncthreads();
    for (int b = tid; b < 3 * NC; b += TPB)
        if (bins[b]) add64(counts + b, bins[b]);
    if (tid == 0 && nbad) add64(bad, nbad);
}

// Instance boundary counts: block (x, y) counts the tile x by instance id, within the band of mask y that lies in the
// instances' band (y < n_masks) or over the instances' band alone (y == n_masks: the GT band sizes, and the range check of
// the instance map over every pixel, done once).  inst_band = band(inst, d), written by k_label_band before this launch.
__global__ void __launch_bounds__(TPB) k_mask_boundary(const uint8_t *__restrict__ masks, int n_masks,
                                                       const uint8_t *__restrict__ inst, const uint8_t *__restrict__ inst_band,
                                                       int g, int h, int w, int d, int tiles_x, int64_t *__restrict__ inter_b,
                                                       int64_t *__restrict__ band_pred, int64_t *__restrict__ band_gt,
                                                       int64_t *__restrict__ bad) {
    extern __shared__ uint32_t band_lds[];
    __shared__ uint32_t cnt[256];
    __shared__ uint32_t total;
    const int tid = threadIdx.x;
    const int m = blockIdx.y;
    cnt[tid] = 0;
    if (tid == 0) total = 0;
    const int x0 = (blockIdx.x % tiles_x) * BT_W, y0 = (blockIdx.x / tiles_x) * BT_H;
    const int tx = tid % BT_W, x = x0 + tx;
    const bool is_mask = m < n_masks;
    BandTile b{};
    if (is_mask) b = band_tile(masks + (size_t)m * h * w, AsMask{}, h, w, d, x0, y0, reinterpret_cast<uint8_t *>(band_lds));
    else __syncthreads();
    uint32_t mine = 0;
#pragma unroll
    for (int i = 0; i < BPT; ++i) {
        const int ty = tid / BT_W + BT_RSTEP * i, y = y0 + ty;
        if (y >= h || x >= w) continue;
        const size_t p = (size_t)y * w + x;
        if (is_mask) {
            if (!b.value(ty, tx) || !b.band(ty, tx)) continue;
            ++mine;
            const uint8_t id = inst[p];
            if (id && inst_band[p]) atomicAdd(&cnt[id], 1u);
        } else {
            const uint8_t id = inst[p];
            if (id && (id > g || inst_band[p])) atomicAdd(&cnt[id], 1u);
        }
    }
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    const uint32_t v = cnt[tid];
    if (tid >= 1 && v) {
        if (tid > g) {
            if (!is_mask) add64(bad, v);              // counted once, by the whole-image row
        } else if (is_mask) {
            add64(inter_b + (size_t)m * g + (tid - 1), v);
        } else {
            add64(band_gt + (tid - 1), v);
        }
    }
    if (tid == 0 && is_mask && total) add64(band_pred + m, total);
}

bool pixels_ok(int h, int w) { return h >= 1 && w >= 1 && (int64_t)h * w <= (int64_t)0x7fffffff - PIX; }
bool band_d_ok(int d) { return d >= 1 && d <= IRN_BAND_MAX_D; }
int band_tiles(int h, int w) { return cdiv(w, BT_W) * cdiv(h, BT_H); }      // below h*w/2048 + h/32 + w/64 + 1: an int where pixels_ok holds

}  // namespace

// Every entry with a class count refuses one outside 2..IRN_EVAL_MAX_CLASSES by name.
extern "C" int irn_cam_confusion(const float *high_res_dev, const int64_t *keys_dev, int k, const uint8_t *gt_dev, int h,
                                 int w, const float *thres_dev, int t, int n_classes, int64_t *hist_dev, int64_t *bad_dev,
                                 void *stream) {
    if (!classes_ok(n_classes))
        return fail(IRN_ERR_ARG, "irn_cam_confusion: n_classes %d outside 2..%d", n_classes, IRN_EVAL_MAX_CLASSES);
    if (!gt_dev || !thres_dev || !hist_dev || !bad_dev || k < 0 || k > n_classes - 1 || (k > 0 && (!high_res_dev || !keys_dev)) ||
        t < 1 || t > IRN_EVAL_MAX_THRES || !pixels_ok(h, w))
        return fail(IRN_ERR_ARG, "irn_cam_confusion: bad argument (k=%d, h=%d, w=%d, t=%d; 0 <= k <= %d, 1 <= t <= %d)",
                    k, h, w, t, n_classes - 1, IRN_EVAL_MAX_THRES);
    const int n = h * w;
    hipLaunchKernelGGL(k_cam_hist, dim3(cdiv(n, PIX)), dim3(TPB), 0, (hipStream_t)stream, high_res_dev, keys_dev, k, gt_dev,
                       n, thres_dev, t, n_classes, hist_dev, bad_dev);
    IRN_LAUNCH_CHECK("k_cam_hist");
    return IRN_OK;
}

extern "C" int irn_cam_confusion_reduce(const int64_t *hist_dev, int t, int n_classes, int64_t *conf_dev,
                                        int64_t *void_dev, void *stream) {
    if (!classes_ok(n_classes))
        return fail(IRN_ERR_ARG, "irn_cam_confusion_reduce: n_classes %d outside 2..%d", n_classes, IRN_EVAL_MAX_CLASSES);
    if (!hist_dev || !conf_dev || t < 1 || t > IRN_EVAL_MAX_THRES)
        return fail(IRN_ERR_ARG, "irn_cam_confusion_reduce: bad argument (t=%d)", t);
    hipLaunchKernelGGL(k_cam_reduce, dim3(cdiv((n_classes + 1) * n_classes, TPB)), dim3(TPB), 0, (hipStream_t)stream, hist_dev,
                       t, n_classes, conf_dev, void_dev);
    IRN_LAUNCH_CHECK("k_cam_reduce");
    return IRN_OK;
}

extern "C" int irn_label_confusion(const uint8_t *pred_dev, const uint8_t *gt_dev, int h, int w, int pred_255_as,
                                   int n_classes, int64_t *conf_dev, int64_t *void_dev, int64_t *bad_dev, void *stream) {
    if (!classes_ok(n_classes))
        return fail(IRN_ERR_ARG, "irn_label_confusion: n_classes %d outside 2..%d", n_classes, IRN_EVAL_MAX_CLASSES);
    if (!pred_dev || !gt_dev || !conf_dev || !bad_dev || pred_255_as >= n_classes || !pixels_ok(h, w))
        return fail(IRN_ERR_ARG, "irn_label_confusion: bad argument (h=%d, w=%d, pred_255_as=%d)", h, w, pred_255_as);
    const int n = h * w;
    const size_t lds = sizeof(uint32_t) * (n_classes + 1) * n_classes;          // 26.6 KB at 81 classes
    hipLaunchKernelGGL(k_label_hist, dim3(cdiv(n, PIX)), dim3(TPB), lds, (hipStream_t)stream, pred_dev, gt_dev, n,
                       pred_255_as, n_classes, conf_dev, void_dev, bad_dev);
    IRN_LAUNCH_CHECK("k_label_hist");
    return IRN_OK;
}

extern "C" int irn_ir_label_confusion(const uint8_t *planes_dev, int t_count, const int32_t *fg_idx, int f,
                                      const int32_t *bg_idx, int b, const uint8_t *gt_dev, int h, int w, int n_classes,
                                      int64_t *hist_dev, int64_t *bad_dev, void *stream) {
    if (!classes_ok(n_classes))
        return fail(IRN_ERR_ARG, "irn_ir_label_confusion: n_classes %d outside 2..%d", n_classes, IRN_EVAL_MAX_CLASSES);
    if (t_count < 1 || t_count > IR_MAX)
        return fail(IRN_ERR_ARG, "irn_ir_label_confusion: t_count %d outside 1..%d", t_count, IR_MAX);
    if (f < 1 || f > IR_MAX || b < 1 || b > IR_MAX)
        return fail(IRN_ERR_ARG, "irn_ir_label_confusion: grid f=%d x b=%d, each axis must be 1..%d", f, b, IR_MAX);
    if (!fg_idx || !bg_idx) return fail(IRN_ERR_ARG, "irn_ir_label_confusion: fg_idx or bg_idx is a null pointer");
    PairIdx idx{};
    for (int i = 0; i < f; ++i) {
        if (fg_idx[i] < 0 || fg_idx[i] >= t_count)
            return fail(IRN_ERR_ARG, "irn_ir_label_confusion: fg_idx[%d] = %d outside [0, t_count = %d)", i, fg_idx[i], t_count);
        idx.fg[i] = (uint8_t)fg_idx[i];
    }
    for (int j = 0; j < b; ++j) {
        if (bg_idx[j] < 0 || bg_idx[j] >= t_count)
            return fail(IRN_ERR_ARG, "irn_ir_label_confusion: bg_idx[%d] = %d outside [0, t_count = %d)", j, bg_idx[j], t_count);
        idx.bg[j] = (uint8_t)bg_idx[j];
    }
    if (!pixels_ok(h, w) || (int64_t)h * w * t_count > (int64_t)0x7fffffff)
        return fail(IRN_ERR_ARG, "irn_ir_label_confusion: bad image size %dx%d for %d planes", h, w, t_count);
    if (!planes_dev || !gt_dev || !hist_dev || !bad_dev)
        return fail(IRN_ERR_ARG, "irn_ir_label_confusion: a null pointer (planes, gt, hist or bad)");
    const int n = h * w;
    // fg values per launch: as many as fit the LDS of a workgroup (>= 1 by the static_assert above)
    const int per = (int)std::min<size_t>((size_t)f, kIrLdsBytes / (ir_lds_words(1, b, n_classes) * sizeof(uint32_t)));
    for (int i0 = 0; i0 < f; i0 += per) {
        const int fi = std::min(per, f - i0);
        const auto kernel = n_classes == IRN_EVAL_CLASSES ? k_ir_label_hist<IRN_EVAL_CLASSES> : k_ir_label_hist<0>;
        hipLaunchKernelGGL(kernel, dim3(cdiv(n, PIX)), dim3(TPB), ir_lds_words(fi, b, n_classes) * sizeof(uint32_t),
                           (hipStream_t)stream, planes_dev, t_count, idx, i0, fi, b, n_classes, gt_dev, n, hist_dev, bad_dev);
        IRN_LAUNCH_CHECK("k_ir_label_hist");
    }
    return IRN_OK;
}

extern "C" int irn_mask_overlap(const uint8_t *masks_dev, int n, const uint8_t *inst_dev, int g, int h, int w,
                                int64_t *inter_dev, int64_t *area_pred_dev, int64_t *area_gt_dev, int64_t *bad_dev,
                                void *stream) {
    if (!inst_dev || !bad_dev || n < 0 || n > 65534 || g < 0 || g > 255 || (n > 0 && (!masks_dev || !area_pred_dev)) ||
        (g > 0 && !area_gt_dev) || (n > 0 && g > 0 && !inter_dev) || !pixels_ok(h, w))
        return fail(IRN_ERR_ARG, "irn_mask_overlap: bad argument (n=%d, g=%d, h=%d, w=%d)", n, g, h, w);
    const int px = h * w;
    hipLaunchKernelGGL(k_mask_overlap, dim3(cdiv(px, PIX), n + 1), dim3(TPB), 0, (hipStream_t)stream, masks_dev, n,
                       inst_dev, g, px, inter_dev, area_pred_dev, area_gt_dev, bad_dev);
    IRN_LAUNCH_CHECK("k_mask_overlap");
    return IRN_OK;
}

// Boundary bands and the counts behind Boundary IoU / Boundary AP (include/irn_hip.h "Boundary counts").
extern "C" int irn_label_band(const uint8_t *map_dev, int h, int w, int d, uint8_t *band_dev, void *stream) {
    if (!band_d_ok(d)) return fail(IRN_ERR_ARG, "irn_label_band: d %d outside 1..%d", d, IRN_BAND_MAX_D);
    if (!map_dev || !band_dev || !pixels_ok(h, w)) return fail(IRN_ERR_ARG, "irn_label_band: bad argument (h=%d, w=%d)", h, w);
    hipLaunchKernelGGL(k_label_band, dim3(band_tiles(h, w)), dim3(TPB), band_lds_bytes(d), (hipStream_t)stream, map_dev, h, w, d,
                       cdiv(w, BT_W), band_dev);
    IRN_LAUNCH_CHECK("k_label_band");
    return IRN_OK;
}

extern "C" int irn_label_boundary_counts(const uint8_t *pred_dev, const uint8_t *gt_dev, int h, int w, int d, int pred_255_as,
                                         int n_classes, int64_t *counts_dev, int64_t *bad_dev, void *stream) {
    if (!classes_ok(n_classes))
        return fail(IRN_ERR_ARG, "irn_label_boundary_counts: n_classes %d outside 2..%d", n_classes, IRN_EVAL_MAX_CLASSES);
    if (!band_d_ok(d)) return fail(IRN_ERR_ARG, "irn_label_boundary_counts: d %d outside 1..%d", d, IRN_BAND_MAX_D);
    if (!pred_dev || !gt_dev || !counts_dev || !bad_dev || pred_255_as >= n_classes || !pixels_ok(h, w))
        return fail(IRN_ERR_ARG, "irn_label_boundary_counts: bad argument (h=%d, w=%d, pred_255_as=%d)", h, w, pred_255_as);
    hipLaunchKernelGGL(k_label_boundary, dim3(band_tiles(h, w)), dim3(TPB), band_lds_bytes(d), (hipStream_t)stream, pred_dev,
                       gt_dev, h, w, d, pred_255_as, n_classes, cdiv(w, BT_W), counts_dev, bad_dev);
    IRN_LAUNCH_CHECK("k_label_boundary");
    return IRN_OK;
}

extern "C" int irn_mask_boundary_overlap(const uint8_t *masks_dev, int n, const uint8_t *inst_dev, uint8_t *inst_band_dev, int g,
                                         int h, int w, int d, int64_t *inter_b_dev, int64_t *band_pred_dev,
                                         int64_t *band_gt_dev, int64_t *bad_dev, void *stream) {
    if (!band_d_ok(d)) return fail(IRN_ERR_ARG, "irn_mask_boundary_overlap: d %d outside 1..%d", d, IRN_BAND_MAX_D);
    if (!inst_dev || !inst_band_dev || !bad_dev || n < 0 || n > 65534 || g < 0 || g > 255 ||
        (n > 0 && (!masks_dev || !band_pred_dev)) || (g > 0 && !band_gt_dev) || (n > 0 && g > 0 && !inter_b_dev) || !pixels_ok(h, w))
        return fail(IRN_ERR_ARG, "irn_mask_boundary_overlap: bad argument (n=%d, g=%d, h=%d, w=%d)", n, g, h, w);
    const int tiles = band_tiles(h, w), tiles_x = cdiv(w, BT_W);
    hipLaunchKernelGGL(k_label_band, dim3(tiles), dim3(TPB), band_lds_bytes(d), (hipStream_t)stream, inst_dev, h, w, d, tiles_x,
                       inst_band_dev);
    IRN_LAUNCH_CHECK("k_label_band");
    hipLaunchKernelGGL(k_mask_boundary, dim3(tiles, n + 1), dim3(TPB), band_lds_bytes(d), (hipStream_t)stream, masks_dev, n,
                       inst_dev, inst_band_dev, g, h, w, d, tiles_x, inter_b_dev, band_pred_dev, band_gt_dev, bad_dev);
    IRN_LAUNCH_CHECK("k_mask_boundary");
    return IRN_OK;
}
