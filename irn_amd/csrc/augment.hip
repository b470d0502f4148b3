// Training-input pipeline of the CAM step on the device, for a whole batch of ragged images: random_resize_long (Pillow's
// 8-bit bicubic, as in msf.hip), TorchvisionNormalize, random mirror, random crop / zero pad and HWC -> CHW of reference
// voc12/dataloader.py:129-156 as step/train_cam.py:44-46 configures it, fused into two launches whatever the batch size.
//
// Everything that depends on the random draw lives in per-image tap tables the host builds (irn_amd.ops.augment_tables):
// the X table lists, for every column of the image's box in the crop, the taps of the resized column it shows (the mirror
// is a reversed table: the kernels never see it); the Y table does the same for the box's rows, rebased to the first
// source row any of them reads.  The kernels are then a plain windowed separable resample: only the source rows [r0, r1)
// go through the horizontal pass, only the columns of the box are produced, and the vertical pass writes every cell of
// the [B, 3, crop, crop] output exactly once — the normalised byte inside the box, 0.0f outside.  Integer arithmetic and a
// table look-up only: bit-exact against the PIL / numpy pipeline and bit-reproducible.
//
// Block shape: one thread per output pixel, 256 threads along x like msf.hip's passes — a wave stores 64 consecutive
// floats (256 B) per plane, the row index is uniform per block so descriptor and Y-table reads are the same address in
// every lane.  The batch's work is the 3 MB of floats per 512^2 image it writes (the byte gathers stay in L2); wider
// per-thread stores would need crop % 4 == 0 and a 16-byte aligned box edge, which a random box does not give.
//
// The kernels trust their tables, so the C entry does not: it takes descriptors and tables as HOST arrays, checks every
// bound before any HIP call, and only then copies them to the caller's device buffer on the stream and launches.
#include "common.hpp"

#pragma clang fp contract(off)

namespace irn {
namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;
constexpr int kDesc = IRN_AUGMENT_DESC_WORDS;
enum { D_H, D_W, D_CTOP, D_CLEFT, D_ROWS, D_COLS, D_R0, D_NROWS, D_KX, D_KY, D_SRC, D_MID, D_XTAB, D_YTAB };

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> kPrecisionBits;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// (a) pixels u8 [h, w, 3] of image z -> mid u8 [nrows, cols, 3]: source rows r0 .. r0 + nrows - 1, box columns only.
__global__ __launch_bounds__(256) void augment_rows_kernel(const uint8_t *__restrict__ pixels, uint8_t *__restrict__ mid,
                                                           const int32_t *__restrict__ meta) {
    const int32_t *d = meta + (size_t)blockIdx.z * kDesc;
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    const int cols = d[D_COLS];
    if (y >= d[D_NROWS] || x >= cols) return;
    const int kx = d[D_KX];
    const int32_t *tab = meta + d[D_XTAB];                       // lo [cols] | count [cols] | weights [cols, kx]
    const int x0 = tab[x], n = tab[cols + x];
    const int32_t *k = tab + 2 * (size_t)cols + (size_t)x * kx;
    const uint8_t *s = pixels + d[D_SRC] + ((size_t)(d[D_R0] + y) * d[D_W] + x0) * 3;
    int acc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = 1 << (kPrecisionBits - 1);
    for (int t = 0; t < n; ++t) {
        const int wgt = k[t];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += (int)s[t * 3 + c] * wgt;
    }
    uint8_t *o = mid + d[D_MID] + ((size_t)y * cols + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (uint8_t)clip8(acc[c]);
}

// (b) every cell of out fp32 [B, 3, crop, crop]: inside image z's box the vertical taps over mid, clip, lut; else 0.
__global__ __launch_bounds__(256) void augment_cols_kernel(const uint8_t *__restrict__ mid, float *__restrict__ out,
                                                           const int32_t *__restrict__ meta, const float *__restrict__ lut,
                                                           int crop) {
    const int32_t *d = meta + (size_t)blockIdx.z * kDesc;
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= crop) return;
    const size_t plane = (size_t)crop * crop;
    float *o = out + (size_t)blockIdx.z * 3 * plane + (size_t)y * crop + x;
    const int rows = d[D_ROWS], cols = d[D_COLS];
    const int yy = y - d[D_CTOP], xx = x - d[D_CLEFT];
    if (yy < 0 || yy >= rows || xx < 0 || xx >= cols) {
        o[0] = 0.0f, o[plane] = 0.0f, o[2 * plane] = 0.0f;
        return;
    }
    const int ky = d[D_KY];
    const int32_t *tab = meta + d[D_YTAB];                       // lo [rows] (from r0) | count [rows] | weights [rows, ky]
    const int y0 = tab[yy], n = tab[rows + yy];
    const int32_t *k = tab + 2 * (size_t)rows + (size_t)yy * ky;
    const uint8_t *s = mid + d[D_MID] + ((size_t)y0 * cols + xx) * 3;
    const size_t pitch = (size_t)cols * 3;
    int acc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] = 1 << (kPrecisionBits - 1);
    for (int t = 0; t < n; ++t) {
        const int wgt = k[t];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += (int)s[t * pitch + c] * wgt;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = lut[c * 256 + clip8(acc[c])];
}

// One axis table of image `i`: `n` entries at word `off` of meta, `ksize` weights per entry, taps inside [0, extent).
int check_table(const int32_t *meta, size_t meta_words, int n_images, int i, const char *axis, int64_t off, int n, int ksize,
                int extent) {
    if (ksize < 1) return fail(IRN_ERR_ARG, "irn_augment_batch: image %d: %s table with %d weights per entry", i, axis, ksize);
    const int64_t words = (int64_t)n * (2 + (int64_t)ksize);
    if (off < (int64_t)n_images * kDesc || off + words > (int64_t)meta_words)
        return fail(IRN_ERR_ARG, "irn_augment_batch: image %d: %s table at word %lld (+%lld) lies outside the %zu words passed", i, axis,
                    (long long)off, (long long)words, meta_words);
    const int32_t *lo = meta + off, *cnt = lo + n;
    for (int j = 0; j < n; ++j)
        if (lo[j] < 0 || cnt[j] < 0 || cnt[j] > ksize || (int64_t)lo[j] + cnt[j] > extent)
            return fail(IRN_ERR_ARG, "irn_augment_batch: image %d: %s tap %d reads [%d, %d + %d) of %d source cells (%d weights)", i, axis, j,
                        lo[j], lo[j], cnt[j], extent, ksize);
    return IRN_OK;
}

}  // namespace
}  // namespace irn

using namespace irn;

extern "C" int irn_augment_batch(int n_images, int crop, const int32_t *meta, size_t meta_words, const uint8_t *pixels_dev,
                                 size_t pixels_bytes, const float *lut_dev, float *out_dev, size_t out_elems, void *scratch_dev,
                                 size_t scratch_bytes, int32_t *meta_dev, size_t meta_dev_words, void *stream) {
    if (n_images < 0) return fail(IRN_ERR_ARG, "irn_augment_batch: n_images must be >= 0 (got %d)", n_images);
    if (crop < 1 || crop > 65535) return fail(IRN_ERR_ARG, "irn_augment_batch: crop must be in 1..65535 (got %d)", crop);
    if (n_images == 0) return IRN_OK;
    if (!meta || !pixels_dev || !lut_dev || !out_dev || !scratch_dev || !meta_dev) return fail(IRN_ERR_ARG, "irn_augment_batch: null pointer");
    if (n_images > 65535) return fail(IRN_ERR_ARG, "irn_augment_batch: at most 65535 images per call (got %d)", n_images);
    if (meta_words < (size_t)n_images * kDesc || meta_words > (size_t)INT32_MAX || meta_dev_words < meta_words)
        return fail(IRN_ERR_ARG, "irn_augment_batch: %zu descriptor / table words for %d images, device buffer of %zu", meta_words, n_images,
                    meta_dev_words);
    if (pixels_bytes > (size_t)INT32_MAX || scratch_bytes > (size_t)INT32_MAX)
        return fail(IRN_ERR_ARG, "irn_augment_batch: pixel and scratch buffers are addressed with 31 bits");
    if (out_elems < (size_t)n_images * 3 * crop * crop)
        return fail(IRN_ERR_ARG, "irn_augment_batch: output of %zu floats for [%d, 3, %d, %d]", out_elems, n_images, crop, crop);
    int max_nrows = 0;
    for (int i = 0; i < n_images; ++i) {
        const int32_t *d = meta + (size_t)i * kDesc;
        const int64_t h = d[D_H], w = d[D_W], rows = d[D_ROWS], cols = d[D_COLS], r0 = d[D_R0], nrows = d[D_NROWS];
        if (h < 1 || w < 1 || h > 65535) return fail(IRN_ERR_ARG, "irn_augment_batch: image %d: bad size %lldx%lld", i, (long long)h, (long long)w);
        if (rows < 1 || cols < 1 || d[D_CTOP] < 0 || d[D_CLEFT] < 0 || d[D_CTOP] + rows > crop || d[D_CLEFT] + cols > crop)
            return fail(IRN_ERR_ARG, "irn_augment_batch: image %d: box %lldx%lld at (%d, %d) is not inside the %d^2 crop", i, (long long)rows,
                        (long long)cols, d[D_CTOP], d[D_CLEFT], crop);
        if (r0 < 0 || nrows < 1 || r0 + nrows > h)
            return fail(IRN_ERR_ARG, "irn_augment_batch: image %d: source rows [%lld, %lld + %lld) of %lld", i, (long long)r0, (long long)r0,
                        (long long)nrows, (long long)h);
        if (d[D_SRC] < 0 || (int64_t)d[D_SRC] + h * w * 3 > (int64_t)pixels_bytes)
            return fail(IRN_ERR_ARG, "irn_augment_batch: image %d: pixels at byte %d (+%lld) lie outside the %zu bytes passed", i, d[D_SRC],
                        (long long)(h * w * 3), pixels_bytes);
        if (d[D_MID] < 0 || (int64_t)d[D_MID] + nrows * cols * 3 > (int64_t)scratch_bytes)
            return fail(IRN_ERR_ARG, "irn_augment_batch: image %d: intermediate at byte %d (+%lld) lies outside the %zu scratch bytes", i,
                        d[D_MID], (long long)(nrows * cols * 3), scratch_bytes);
        if (int rc = check_table(meta, meta_words, n_images, i, "X", d[D_XTAB], (int)cols, d[D_KX], (int)w)) return rc;
        if (int rc = check_table(meta, meta_words, n_images, i, "Y", d[D_YTAB], (int)rows, d[D_KY], (int)nrows)) return rc;
        if (nrows > max_nrows) max_nrows = (int)nrows;
    }
    hipStream_t st = (hipStream_t)stream;
    IRN_HIP_TRY(hipMemcpyAsync(meta_dev, meta, meta_words * sizeof(int32_t), hipMemcpyHostToDevice, st));
    augment_rows_kernel<<<dim3(cdiv(crop, 256), max_nrows, n_images), 256, 0, st>>>(pixels_dev, (uint8_t *)scratch_dev, meta_dev);
    IRN_LAUNCH_CHECK("augment_rows_kernel");
    augment_cols_kernel<<<dim3(cdiv(crop, 256), crop, n_images), 256, 0, st>>>((const uint8_t *)scratch_dev, out_dev, meta_dev, lut_dev, crop);
    IRN_LAUNCH_CHECK("augment_cols_kernel");
    return IRN_OK;
}
