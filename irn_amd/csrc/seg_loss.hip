// Fused bilinear upsampling + softmax cross-entropy of segmentation training, and the arg-max of inference (gfx950).
//
// Replaces, for the training step, F.interpolate(logits, scale_factor = f, bilinear) -> F.cross_entropy(ignore_index = 255):
// at batch 16, crop 512 and 21 labels that chain writes [16, 21, 512, 512] floats three times (logits, log-softmax, gradient,
// 352 MB each), and ATen's upsample_bilinear2d_backward scatters with float atomics.  Here the fine logits
//     z[b, c, Y, X] = bilinear interpolation of logits[b, c, :, :] at fine pixel (Y, X)      (upsample.hpp: the arithmetic of
// irn_upsample_bilinear, bit for bit) exist in registers only.  A workgroup owns a tile of kTile x kTile coarse cells and keeps
// their logits with a one-cell halo in LDS, all classes of a cell side by side:
//   forward:  the fine pixels whose first taps the tile holds ([ty0 * f, (ty0 + kTile) * f) rows, likewise columns), one pixel
//             per thread and pass: maximum over the classes, then sum of exp(z - max), fp32 as torch does it;
//             l = max + log(sum) - z[label] with the one logarithm per pixel in fp64.  Accumulation in fp64: lanes by shuffle,
//             the four waves in order, one partial per workgroup in the workspace, and a second kernel adds an image's
//             partials in a fixed order.  No float atomics.  The log-sum-exp kept for the backward is fp64 too: an fp32 one
//             of logits near 1e4 is off by up to 5e-4, which exp(z - lse) turns into a relative error of the gradient.
//   backward: a gather.  Thread <-> (coarse cell, class) of the tile, the classes of a cell in neighbouring lanes (their label
//             and log-sum-exp loads are one address, their LDS reads consecutive words).  It walks the cell's footprint of at most
//             2f x 2f fine pixels, Y ascending and X ascending within a row, recomputes z from LDS and adds
//             w(Y, X -> y, x) * (exp(z - lse) - [label == c]) in a register; one plain store per element of grad_logits.
//             No atomics of any kind, nothing is cleared first, an image's gradient does not depend on its batch.
//   argmax:   the forward's tiling; the first class that attains the maximum, a NaN counting as the maximum.
// Tile: (8 + 2)^2 cells x C floats (C rounded up to an odd stride: cells in different lanes then fall into different banks)
// = 32.4 KB at the class cap of 81, 8.4 KB at 21: four workgroups of the cap still share a CU's 160 KB.
#include "common.hpp"
#include "upsample.hpp"

namespace irn {

namespace {

constexpr int kTile = 8;                   // coarse cells per tile side
constexpr int kLW = kTile + 2;             // with the halo
constexpr int kCells = kLW * kLW;

__host__ __device__ constexpr int class_stride(int C) { return C | 1; }
__host__ __device__ constexpr size_t lds_bytes(int C) { return (size_t)kCells * class_stride(C) * sizeof(float); }

// Stage coarse rows [ty0 - 1, ty0 + kTile], columns [tx0 - 1, tx0 + kTile] of all C planes of one image: tile[cell * cs + c].
// Cells outside the grid are never a tap (the taps are clamped to the grid); they are filled with 0.
__device__ __forceinline__ void stage(const float *__restrict__ img, int C, int h, int w, int ty0, int tx0, float *tile) {
    const int cs = class_stride(C);
    const size_t plane = (size_t)h * w;
    for (int i = threadIdx.x; i < kCells * C; i += 256) {
        const int c = i / kCells, cell = i - c * kCells;
        const int ly = cell / kLW, lx = cell - ly * kLW;
        const int gy = ty0 - 1 + ly, gx = tx0 - 1 + lx;
        float v = 0.f;
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) v = img[c * plane + (size_t)gy * w + gx];
        tile[cell * cs + c] = v;
    }
}

// LDS word offsets of the four taps of fine pixel (Y, X) in the tile whose first cell is (ty0, tx0), and the blend's weights.
struct FineTaps {
    int o00, o01, o10, o11;
    float lx0, lx, ly0, ly;
};

__device__ __forceinline__ int tile_index(int i, int t0) {
    const int r = i - (t0 - 1);
    return r < 0 ? 0 : (r > kLW - 1 ? kLW - 1 : r);      // (in range by construction; the clamp keeps a reading inside LDS)
}

__device__ __forceinline__ FineTaps fine_taps(int Y, int X, int h, int w, float rscale, int ty0, int tx0, int cs) {
    const UpsampleTap ty = upsample_tap(Y, h, rscale), tx = upsample_tap(X, w, rscale);
    const int r0 = tile_index(ty.i0, ty0) * kLW, r1 = tile_index(ty.i1, ty0) * kLW;
    const int c0 = tile_index(tx.i0, tx0), c1 = tile_index(tx.i1, tx0);
    return FineTaps{(r0 + c0) * cs, (r0 + c1) * cs, (r1 + c0) * cs, (r1 + c1) * cs, 1.f - tx.l, tx.l, 1.f - ty.l, ty.l};
}

__device__ __forceinline__ float fine_logit(const float *tile, const FineTaps &t, int c) {
    return upsample_blend(tile[t.o00 + c], tile[t.o01 + c], tile[t.o10 + c], tile[t.o11 + c], t.lx0, t.lx, t.ly0, t.ly);
}

// The fine rectangle of tile (ty0, tx0) inside the H x W window: rows [Y0, Y1), columns [X0, X1).
struct FineRect {
    int Y0, X0, fh, fw;
};

__device__ __forceinline__ FineRect fine_rect(int ty0, int tx0, int factor, int H, int W) {
    const int Y0 = ty0 * factor, X0 = tx0 * factor;
    return FineRect{Y0, X0, min((ty0 + kTile) * factor, H) - Y0, min((tx0 + kTile) * factor, W) - X0};
}

// grid (tiles of the window, batch); part: [batch, tiles, 2] = fp64 sum, int64 count (as bits)
__global__ __launch_bounds__(256) void seg_loss_forward_kernel(const float *__restrict__ logits, const unsigned char *__restrict__ label,
                                                               int C, int h, int w, int factor, int H, int W, float rscale,
                                                               int tiles_x, double *__restrict__ lse_out, double *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int cs = class_stride(C);
    const int ty0 = ((int)blockIdx.x / tiles_x) * kTile, tx0 = ((int)blockIdx.x % tiles_x) * kTile;
    const size_t b = blockIdx.y;
    stage(logits + b * C * h * w, C, h, w, ty0, tx0, tile);
    __syncthreads();

    const FineRect r = fine_rect(ty0, tx0, factor, H, W);
    const unsigned char *lab_img = label + b * H * W;
    double acc = 0.0;
    long long cnt = 0;
    for (int p = threadIdx.x; p < r.fh * r.fw; p += 256) {
        const int dy = p / r.fw, Y = r.Y0 + dy, X = r.X0 + (p - dy * r.fw);
        const FineTaps t = fine_taps(Y, X, h, w, rscale, ty0, tx0, cs);
        const size_t at = (size_t)Y * W + X;
        const int lab = lab_img[at];
        float m = -INFINITY, zl = 0.f;
        for (int c = 0; c < C; ++c) {
            const float z = fine_logit(tile, t, c);
            m = z > m ? z : m;
            zl = c == lab ? z : zl;
        }
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += expf(fine_logit(tile, t, c) - m);
        // the one logarithm of a pixel and the two additions around it in fp64: the device's fp32 logarithm lies 0.6 ulp below
        // the true value ON AVERAGE (measured at s in [1, 21]), an error that does not average out over the pixels of a sum
        const double lse = (double)m + log((double)s);
        if (lse_out) lse_out[b * H * W + at] = lse;
        if (lab < C) {
            acc += lse - (double)zl;
            ++cnt;
        }
    }

    // workgroup partial, in a fixed order: lanes by shuffle, then the four waves one after the other
    for (int s = 32; s; s >>= 1) {
        acc += __shfl_down(acc, s, 64);
        cnt += __shfl_down(cnt, s, 64);
    }
    __shared__ double wave_sum[4];
    __shared__ long long wave_cnt[4];
    if ((threadIdx.x & 63) == 0) {
        wave_sum[threadIdx.x >> 6] = acc;
        wave_cnt[threadIdx.x >> 6] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *out = part + (b * gridDim.x + blockIdx.x) * 2;
        out[0] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
        out[1] = __longlong_as_double(wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3]);
    }
}

// One workgroup per image: thread t adds the image's partials t, t + 256, ... in ascending order, then a fixed tree.
__global__ __launch_bounds__(256) void seg_loss_finish_kernel(const double *__restrict__ part, int tiles, double *__restrict__ sums,
                                                              long long *__restrict__ counts) {
    __shared__ double red_sum[256];
    __shared__ long long red_cnt[256];
    const double *q = part + (size_t)blockIdx.x * tiles * 2;
    double v = 0.0;
    long long n = 0;
    for (int p = threadIdx.x; p < tiles; p += 256) {
        v += q[2 * p];
        n += __double_as_longlong(q[2 * p + 1]);
    }
    red_sum[threadIdx.x] = v;
    red_cnt[threadIdx.x] = n;
    __syncthreads();
    for (int s = 128; s; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red_sum[threadIdx.x] += red_sum[threadIdx.x + s];
            red_cnt[threadIdx.x] += red_cnt[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = red_sum[0];
        counts[blockIdx.x] = red_cnt[0];
    }
}

// grid (tiles of the whole coarse grid, batch): every (cell, class) of grad is stored once
__global__ __launch_bounds__(256) void seg_loss_backward_kernel(const float *__restrict__ logits, const unsigned char *__restrict__ label,
                                                                const double *__restrict__ lse, const float *__restrict__ coef, int C,
                                                                int h, int w, int factor, int H, int W, float rscale, int tiles_x,
                                                                float *__restrict__ grad) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int cs = class_stride(C);
    const int ty0 = ((int)blockIdx.x / tiles_x) * kTile, tx0 = ((int)blockIdx.x % tiles_x) * kTile;
    const size_t b = blockIdx.y;
    stage(logits + b * C * h * w, C, h, w, ty0, tx0, tile);
    __syncthreads();

    const unsigned char *lab_img = label + b * H * W;
    const double *lse_img = lse + b * H * W;
    const float cf = coef[b];
    const int below = upsample_below(factor), above = upsample_above(factor);
    for (int pair = threadIdx.x; pair < kTile * kTile * C; pair += 256) {
        const int cell = pair / C, c = pair - cell * C;
        const int y = ty0 + cell / kTile, x = tx0 + cell % kTile;
        if (y >= h || x >= w) continue;
        const int Ya = max(0, factor * y - below), Yb = min(H, factor * y + above);
        const int Xa = max(0, factor * x - below), Xb = min(W, factor * x + above);
        float acc = 0.f;
        for (int Y = Ya; Y < Yb; ++Y) {
            const float wy = upsample_weight(Y, y, h, rscale);
            if (wy == 0.f) continue;
            for (int X = Xa; X < Xb; ++X) {
                const float wx = upsample_weight(X, x, w, rscale);
                if (wx == 0.f) continue;
                const size_t at = (size_t)Y * W + X;
                const int lab = lab_img[at];
                if (lab >= C) continue;
                // a nonzero weight means that (y, x) is one of the pixel's taps: the other three are its neighbours, in the halo
                const FineTaps t = fine_taps(Y, X, h, w, rscale, ty0, tx0, cs);
                const float p = expf((float)((double)fine_logit(tile, t, c) - lse_img[at]));
                acc += (p - (lab == c ? 1.f : 0.f)) * (wy * wx);
            }
        }
        grad[(b * C + c) * h * w + (size_t)y * w + x] = cf * acc;
    }
}

// grid (tiles of the window, batch)
__global__ __launch_bounds__(256) void seg_argmax_kernel(const float *__restrict__ logits, int C, int h, int w, int factor, int H, int W,
                                                         float rscale, int tiles_x, unsigned char *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const int cs = class_stride(C);
    const int ty0 = ((int)blockIdx.x / tiles_x) * kTile, tx0 = ((int)blockIdx.x % tiles_x) * kTile;
    const size_t b = blockIdx.y;
    stage(logits + b * C * h * w, C, h, w, ty0, tx0, tile);
    __syncthreads();

    const FineRect r = fine_rect(ty0, tx0, factor, H, W);
    for (int p = threadIdx.x; p < r.fh * r.fw; p += 256) {
        const int dy = p / r.fw, Y = r.Y0 + dy, X = r.X0 + (p - dy * r.fw);
        const FineTaps t = fine_taps(Y, X, h, w, rscale, ty0, tx0, cs);
        float best = fine_logit(tile, t, 0);
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            const float z = fine_logit(tile, t, c);
            // strict: the first of equals stays; the first NaN is the maximum and stays (torch.argmax)
            if (best == best && (z > best || z != z)) {
                best = z;
                arg = c;
            }
        }
        out[b * H * W + (size_t)Y * W + X] = (unsigned char)arg;
    }
}

bool geometry_ok(int batch, int C, int h, int w, int factor, int H, int W) {
    return batch >= 1 && batch <= 65535 && C >= 2 && C <= IRN_EVAL_MAX_CLASSES && h >= 1 && h <= 32768 && w >= 1 && w <= 32768 &&
           factor >= 1 && factor <= 64 && H >= 1 && H <= h * factor && W >= 1 && W <= w * factor;
}

// tiles that hold the first taps of the window's fine pixels
int window_tiles_x(int factor, int W) { return cdiv(cdiv(W, factor), kTile); }
int window_tiles(int factor, int H, int W) { return cdiv(cdiv(H, factor), kTile) * window_tiles_x(factor, W); }

// everything that can be refused before a device is touched
int check_geometry(const char *who, int batch, int C, int h, int w, int factor, int H, int W) {
    if (batch < 1 || batch > 65535) return fail(IRN_ERR_ARG, "%s: batch must be in [1, 65535]", who);
    if (C < 2 || C > IRN_EVAL_MAX_CLASSES) return fail(IRN_ERR_ARG, "%s: C %d outside 2..%d", who, C, IRN_EVAL_MAX_CLASSES);
    if (h < 1 || h > 32768 || w < 1 || w > 32768) return fail(IRN_ERR_ARG, "%s: coarse grid %dx%d outside 1..32768", who, h, w);
    if (factor < 1 || factor > 64) return fail(IRN_ERR_ARG, "%s: factor %d outside 1..64", who, factor);
    if (H < 1 || H > h * factor) return fail(IRN_ERR_ARG, "%s: H %d outside 1..%d (h * factor)", who, H, h * factor);
    if (W < 1 || W > w * factor) return fail(IRN_ERR_ARG, "%s: W %d outside 1..%d (w * factor)", who, W, w * factor);
    return IRN_OK;
}

bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int check_workspace(const char *who, int batch, int C, int h, int w, int factor, int H, int W, const void *ws, size_t ws_bytes) {
    if (!aligned(ws, 8)) return fail(IRN_ERR_ARG, "%s: workspace must be 8-byte aligned", who);
    const size_t need = irn_seg_loss_workspace_bytes(batch, C, h, w, factor, H, W);
    if (ws_bytes < need)
        return fail(IRN_ERR_STATE, "%s: workspace of %zu bytes, irn_seg_loss_workspace_bytes asks for %zu", who, ws_bytes, need);
    return IRN_OK;
}

}  // namespace

}  // namespace irn

using namespace irn;

extern "C" size_t irn_seg_loss_workspace_bytes(int batch, int C, int h, int w, int factor, int H, int W) {
    if (!geometry_ok(batch, C, h, w, factor, H, W)) return 0;
    return (size_t)batch * window_tiles(factor, H, W) * 2 * sizeof(double);
}

extern "C" int irn_seg_loss_forward(const float *logits, const uint8_t *label, int batch, int C, int h, int w, int factor, int H,
                                    int W, double *sums, int64_t *counts, double *lse, void *ws, size_t ws_bytes, void *stream_) {
    const char *who = "irn_seg_loss_forward";
    if (!logits || !label || !sums || !counts || !ws) return fail(IRN_ERR_ARG, "%s: null pointer", who);
    if (int rc = check_geometry(who, batch, C, h, w, factor, H, W)) return rc;
    if (!aligned(sums, 8) || !aligned(counts, 8) || !aligned(lse, 8))
        return fail(IRN_ERR_ARG, "%s: sums, counts and lse must be 8-byte aligned", who);
    if (!aligned(logits, 4)) return fail(IRN_ERR_ARG, "%s: logits must be 4-byte aligned", who);
    if (int rc = check_workspace(who, batch, C, h, w, factor, H, W, ws, ws_bytes)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const int tiles = window_tiles(factor, H, W);
    const float rscale = (float)(1.0 / (double)factor);
    hipLaunchKernelGGL(seg_loss_forward_kernel, dim3(tiles, batch), dim3(256), lds_bytes(C), stream, logits, label, C, h, w, factor, H,
                       W, rscale, window_tiles_x(factor, W), lse, (double *)ws);
    IRN_LAUNCH_CHECK("seg_loss_forward_kernel");
    hipLaunchKernelGGL(seg_loss_finish_kernel, dim3(batch), dim3(256), 0, stream, (const double *)ws, tiles, sums,
                       (long long *)counts);
    IRN_LAUNCH_CHECK("seg_loss_finish_kernel");
    return IRN_OK;
}

extern "C" int irn_seg_loss_backward(const float *logits, const uint8_t *label, const double *lse, const float *coef, int batch, int C,
                                     int h, int w, int factor, int H, int W, float *grad_logits, void *ws, size_t ws_bytes,
                                     void *stream_) {
    const char *who = "irn_seg_loss_backward";
    if (!logits || !label || !lse || !coef || !grad_logits || !ws) return fail(IRN_ERR_ARG, "%s: null pointer", who);
    if (int rc = check_geometry(who, batch, C, h, w, factor, H, W)) return rc;
    if (!aligned(lse, 8)) return fail(IRN_ERR_ARG, "%s: lse must be 8-byte aligned", who);
    if (!aligned(logits, 4) || !aligned(coef, 4) || !aligned(grad_logits, 4))
        return fail(IRN_ERR_ARG, "%s: logits, coef and grad_logits must be 4-byte aligned", who);
    if (int rc = check_workspace(who, batch, C, h, w, factor, H, W, ws, ws_bytes)) return rc;
    const float rscale = (float)(1.0 / (double)factor);
    // tiles over the whole coarse grid: every element of grad_logits is stored once, nothing is cleared first
    hipLaunchKernelGGL(seg_loss_backward_kernel, dim3(cdiv(h, kTile) * cdiv(w, kTile), batch), dim3(256), lds_bytes(C),
                       (hipStream_t)stream_, logits, label, lse, coef, C, h, w, factor, H, W, rscale, cdiv(w, kTile), grad_logits);
    IRN_LAUNCH_CHECK("seg_loss_backward_kernel");
    return IRN_OK;
}

extern "C" int irn_seg_argmax(const float *logits, int batch, int C, int h, int w, int factor, int H, int W, uint8_t *out,
                              void *stream_) {
    const char *who = "irn_seg_argmax";
    if (!logits || !out) return fail(IRN_ERR_ARG, "%s: null pointer", who);
    if (int rc = check_geometry(who, batch, C, h, w, factor, H, W)) return rc;
    if (!aligned(logits, 4)) return fail(IRN_ERR_ARG, "%s: logits must be 4-byte aligned", who);
    const float rscale = (float)(1.0 / (double)factor);
    hipLaunchKernelGGL(seg_argmax_kernel, dim3(window_tiles(factor, H, W), batch), dim3(256), lds_bytes(C), (hipStream_t)stream_,
                       logits, C, h, w, factor, H, W, rscale, window_tiles_x(factor, W), out);
    IRN_LAUNCH_CHECK("seg_argmax_kernel");
    return IRN_OK;
}
