// Multi-scale segmentation inference in one launch (gfx950): bilinear upsampling of up to 16 logit maps of different sizes to
// the image's size, softmax of each, their mean, and its arg-max (include/irn_hip.h, irn_seg_fuse).
//
// Composed from torch ops the same thing writes a [C, H, W] tensor per map for the upsampling, another for the softmax, and
// the running sum.  Here the upsampled logits and the per-map probabilities exist in registers only:
//   z_m[c, Y, X] = upsample_blend over upsample_tap(Y, h_m, ry_m), upsample_tap(X, w_m, rx_m)      (upsample.hpp, bit for bit)
//   p_m = softmax_c(z_m),  P = (p_0 + ... + p_{M-1}) * (1 / M),  label = the first class that attains the maximum of P.
// A workgroup of 256 threads owns a T x T tile of output pixels.  For every map it stages the coarse rectangle the tile's taps
// touch — rows upsample_tap(first row).i0 .. upsample_tap(last row).i1, likewise columns, taken from the tap function itself:
// the fp32 mapping is monotone in the output index — into LDS, all classes of a cell side by side at seg_loss.hip's odd class
// stride.  Each pixel then makes two passes:
//   over the maps:    taps, maximum and 1 / sum of exp(z - max) of each map: seven registers a map, C stays a run-time argument;
//   over the classes: P_c = sum over the maps of exp(z_mc - max_m) * (1 / sum_m) in map order, the running arg-max and the
//                     optional store.
// Every element of `label` and `prob` is written once with a plain store; nothing is accumulated in memory.
// The host evaluates the same tap function over every tile of the output to size each map's rectangle, and picks the largest
// T of 32, 16, 8 whose rectangles fit in 64 KB.
#include <algorithm>

#include "common.hpp"
#include "upsample.hpp"

namespace irn {

namespace {

constexpr int kMaxMaps = IRN_SEG_FUSE_MAX_MAPS;
constexpr int kMaxSide = 32768;
constexpr size_t kLdsBudget = 64 * 1024 - 512;        // a workgroup's 64 KB less the static table below

__host__ __device__ constexpr int class_stride(int C) { return C | 1; }

// by value in the kernel's arguments: 16 x 32 bytes
struct FuseMaps {
    const float *map[kMaxMaps];
    int h[kMaxMaps], w[kMaxMaps];
    float ry[kMaxMaps], rx[kMaxMaps];
    int lh[kMaxMaps], lw[kMaxMaps];                   // the largest rectangle any tile needs, rows and columns: the LDS carved
};

// a tile's rectangle of one map, worked out once by thread 0: first row, first column, rows, columns, LDS word offset
struct Rect {
    int y0, x0, rows, cols, off;
};

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// grid (tiles of the output).  kMaps: the per-pixel state is held for that many maps, M <= kMaps (the arithmetic does not depend on it)
template <int kMaps>
__global__ __launch_bounds__(256) void seg_fuse_kernel(FuseMaps a, int M, int C, int H, int W, int tshift, int tiles_x, float inv_maps,
                                                       unsigned char *__restrict__ label, float *__restrict__ prob) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    __shared__ Rect rect[kMaxMaps];
    const int cs = class_stride(C);
    const int T = 1 << tshift;
    const int Y0 = ((int)blockIdx.x / tiles_x) << tshift, X0 = ((int)blockIdx.x % tiles_x) << tshift;
    const int Yl = min(Y0 + T, H) - 1, Xl = min(X0 + T, W) - 1;

    if (threadIdx.x == 0) {
        int off = 0;
        for (int m = 0; m < M; ++m) {
            const int y0 = clampi(upsample_tap(Y0, a.h[m], a.ry[m]).i0, a.h[m] - 1);
            const int x0 = clampi(upsample_tap(X0, a.w[m], a.rx[m]).i0, a.w[m] - 1);
            // (never above lh x lw: the host took them from these very expressions; the clamp keeps every write inside LDS)
            const int rows = clampi(upsample_tap(Yl, a.h[m], a.ry[m]).i1 - y0 + 1, a.lh[m]);
            const int cols = clampi(upsample_tap(Xl, a.w[m], a.rx[m]).i1 - x0 + 1, a.lw[m]);
            rect[m] = Rect{y0, x0, max(rows, 1), max(cols, 1), off};
            off += a.lh[m] * a.lw[m] * cs;
        }
    }
    __syncthreads();

    for (int m = 0; m < M; ++m) {
        const Rect r = rect[m];
        const float *__restrict__ src = a.map[m];
        const int h = a.h[m], w = a.w[m];
        const size_t plane = (size_t)h * w;
        const int cells = r.rows * r.cols;
        for (int i = threadIdx.x; i < cells * C; i += 256) {
            const int c = i / cells, cell = i - c * cells;
            const int ly = cell / r.cols, lx = cell - ly * r.cols;
            const int gy = min(r.y0 + ly, h - 1), gx = min(r.x0 + lx, w - 1);
            tile[r.off + cell * cs + c] = src[c * plane + (size_t)gy * w + gx];
        }
    }
    __syncthreads();

    const size_t HW = (size_t)H * W;
    for (int p = threadIdx.x; p < T * T; p += 256) {
        const int Y = Y0 + (p >> tshift), X = X0 + (p & (T - 1));
        if (Y > Yl || X > Xl) continue;
        // per map: LDS word of the (i0, i0) tap, the steps to the i1 row and column, the weights, the maximum and 1 / sum
        int base[kMaps], dyo[kMaps], dxo[kMaps];
        float wy[kMaps], wx[kMaps], mx[kMaps], inv[kMaps];
#pragma unroll
        for (int m = 0; m < kMaps; ++m) {
            if (m < M) {
                const Rect r = rect[m];
                const UpsampleTap ty = upsample_tap(Y, a.h[m], a.ry[m]), tx = upsample_tap(X, a.w[m], a.rx[m]);
                const int r0 = clampi(ty.i0 - r.y0, r.rows - 1), r1 = clampi(ty.i1 - r.y0, r.rows - 1);
                const int c0 = clampi(tx.i0 - r.x0, r.cols - 1), c1 = clampi(tx.i1 - r.x0, r.cols - 1);
                const int b = r.off + (r0 * r.cols + c0) * cs, dy = (r1 - r0) * r.cols * cs, dx = (c1 - c0) * cs;
                const float ly = ty.l, lx = tx.l, ly0 = 1.f - ly, lx0 = 1.f - lx;
                float top = -INFINITY;
                for (int c = 0; c < C; ++c) {
                    const float z = upsample_blend(tile[b + c], tile[b + dx + c], tile[b + dy + c], tile[b + dy + dx + c], lx0, lx, ly0, ly);
                    top = z > top ? z : top;
                }
                float s = 0.f;
                for (int c = 0; c < C; ++c) {
                    const float z = upsample_blend(tile[b + c], tile[b + dx + c], tile[b + dy + c], tile[b + dy + dx + c], lx0, lx, ly0, ly);
                    s += expf(z - top);
                }
                base[m] = b, dyo[m] = dy, dxo[m] = dx, wy[m] = ly, wx[m] = lx, mx[m] = top, inv[m] = 1.f / s;
            }
        }
        const size_t at = (size_t)Y * W + X;
        float best = 0.f;
        int arg = 0;
        for (int c = 0; c < C; ++c) {
            float P = 0.f;
#pragma unroll
            for (int m = 0; m < kMaps; ++m) {
                if (m < M) {
                    const int b = base[m] + c, dy = dyo[m], dx = dxo[m];
                    const float z = upsample_blend(tile[b], tile[b + dx], tile[b + dy], tile[b + dy + dx], 1.f - wx[m], wx[m], 1.f - wy[m], wy[m]);
                    P += expf(z - mx[m]) * inv[m];
                }
            }
            P *= inv_maps;
            // strict: the first of equals stays; the first NaN is the maximum and stays (irn_seg_argmax)
            if (c == 0 || (best == best && (P > best || P != P))) {
                best = P;
                arg = c;
            }
            if (prob) prob[c * HW + at] = P;
        }
        if (label) label[at] = (unsigned char)arg;
    }
}

bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// The most cells along one axis that a tile of T outputs touches in a map of n cells: the kernel's own expressions, over every tile.
int axis_extent(int N, int T, int n, float rscale) {
    int ext = 1;
    for (int first = 0; first < N; first += T) {
        const int last = std::min(first + T, N) - 1;
        const int i0 = std::min(upsample_tap(first, n, rscale).i0, n - 1);
        ext = std::max(ext, upsample_tap(last, n, rscale).i1 - i0 + 1);
    }
    return std::min(ext, n);
}

}  // namespace

}  // namespace irn

using namespace irn;

extern "C" int irn_seg_fuse(const float *const *maps, const int32_t *h, const int32_t *w, const int32_t *Hs, const int32_t *Ws, int M,
                            int C, int stride, int H, int W, uint8_t *label, float *prob, void *stream_) {
    const char *who = "irn_seg_fuse";
    if (!maps || !h || !w || !Hs || !Ws) return fail(IRN_ERR_ARG, "%s: null pointer (maps, h, w, Hs or Ws)", who);
    if (!label && !prob) return fail(IRN_ERR_ARG, "%s: null pointer (label and prob are both NULL)", who);
    if (M < 1 || M > kMaxMaps) return fail(IRN_ERR_ARG, "%s: M %d outside 1..%d", who, M, kMaxMaps);
    if (C < 2 || C > IRN_EVAL_MAX_CLASSES) return fail(IRN_ERR_ARG, "%s: C %d outside 2..%d", who, C, IRN_EVAL_MAX_CLASSES);
    if (stride < 1 || stride > 64) return fail(IRN_ERR_ARG, "%s: stride %d outside 1..64", who, stride);
    if (H < 1 || H > kMaxSide || W < 1 || W > kMaxSide) return fail(IRN_ERR_ARG, "%s: output %dx%d outside 1..%d", who, H, W, kMaxSide);
    if (!aligned(prob, 4)) return fail(IRN_ERR_ARG, "%s: prob must be 4-byte aligned", who);
    FuseMaps a{};
    for (int m = 0; m < M; ++m) {
        if (!maps[m]) return fail(IRN_ERR_ARG, "%s: maps[%d] is a null pointer", who, m);
        if (!aligned(maps[m], 4)) return fail(IRN_ERR_ARG, "%s: maps[%d] must be 4-byte aligned", who, m);
        if (h[m] < 1 || h[m] > kMaxSide || w[m] < 1 || w[m] > kMaxSide)
            return fail(IRN_ERR_ARG, "%s: map %d of %dx%d cells outside 1..%d", who, m, h[m], w[m], kMaxSide);
        if (Hs[m] < 1 || Hs[m] > h[m] * stride || Ws[m] < 1 || Ws[m] > w[m] * stride)
            return fail(IRN_ERR_ARG, "%s: Hs, Ws[%d] = %dx%d outside 1..%dx%d (h, w * stride)", who, m, Hs[m], Ws[m], h[m] * stride,
                        w[m] * stride);
        if (Hs[m] > stride * H || Ws[m] > stride * W)
            return fail(IRN_ERR_ARG, "%s: Hs, Ws[%d] = %dx%d above %dx%d (stride * H, W): a map finer than the output", who, m, Hs[m],
                        Ws[m], stride * H, stride * W);
        a.map[m] = maps[m], a.h[m] = h[m], a.w[m] = w[m];
        a.ry[m] = (float)((double)Hs[m] / ((double)stride * H));
        a.rx[m] = (float)((double)Ws[m] / ((double)stride * W));
    }
    // the largest tile whose rectangles fit
    const int cs = class_stride(C);
    int tshift = 0;
    for (int ts = 5; ts >= 3; --ts) {
        const int T = 1 << ts;
        size_t words = 0;
        int lh[kMaxMaps], lw[kMaxMaps];
        for (int m = 0; m < M; ++m) {
            lh[m] = axis_extent(H, T, h[m], a.ry[m]);
            lw[m] = axis_extent(W, T, w[m], a.rx[m]);
            words += (size_t)lh[m] * lw[m] * cs;
        }
        if (words * sizeof(float) > kLdsBudget) continue;
        tshift = ts;
        for (int m = 0; m < M; ++m) a.lh[m] = lh[m], a.lw[m] = lw[m];
        break;
    }
    if (!tshift)
        return fail(IRN_ERR_ARG, "%s: geometry (M %d, C %d, stride %d, output %dx%d): the maps' rectangles of an 8 x 8 tile exceed %zu bytes of LDS",
                    who, M, C, stride, H, W, kLdsBudget);
    const int T = 1 << tshift;
    size_t words = 0;
    for (int m = 0; m < M; ++m) words += (size_t)a.lh[m] * a.lw[m] * cs;
    const auto kernel = M <= 4 ? seg_fuse_kernel<4> : (M <= 8 ? seg_fuse_kernel<8> : seg_fuse_kernel<kMaxMaps>);
    hipLaunchKernelGGL(kernel, dim3(cdiv(H, T) * cdiv(W, T)), dim3(256), words * sizeof(float), (hipStream_t)stream_, a, M, C, H, W, tshift,
                       cdiv(W, T), (float)(1.0 / M), label, prob);
    IRN_LAUNCH_CHECK("seg_fuse_kernel");
    return IRN_OK;
}
