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
//
// The label half of the IRNet step's (image, label) pair (reference voc12/dataloader.py:251-267: Pillow NEAREST rescale,
// mirror, the image's crop box into a container of 255, pil_rescale(label, 0.25, 0)) is one gather, augment_label_kernel:
// output cell (y, x) of the [crop / reduce]^2 map looks at container position (reduce * y + reduce / 2, reduce * x +
// reduce / 2) — what Pillow's NEAREST reads when it shrinks by an integer factor — which is 255 outside the image's box and
// source cell (row table[Y - c_top], column table[X - c_left]) inside it.  The tables are Pillow's nearest indices of the
// box's rows and columns (irn_amd.ops.nearest_plan; a mirrored image lists its columns reversed), so the kernel is integers
// only, has no atomics and writes every cell once.  64 x 4 threads per block, one thread per cell: a wave is 64 cells of
// one output row, image and row are uniform per wave, so descriptor and row-table reads are one address for all lanes.
// The whole output at the training shape (32 x 128 x 128) is 512 KB and the launch is latency-bound: byte stores are
// left as they are, wider ones would buy nothing measurable.
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

constexpr int kLabelDesc = IRN_AUGMENT_LABEL_DESC_WORDS;
enum { L_H, L_W, L_CTOP, L_CLEFT, L_ROWS, L_COLS, L_SRC, L_RTAB, L_CTAB };

// every cell of out u8 [B, grid, grid]: the label of image z under container position (reduce * y + half, reduce * x + half).
__global__ __launch_bounds__(256) void augment_label_kernel(const uint8_t *__restrict__ labels, uint8_t *__restrict__ out,
                                                            const int32_t *__restrict__ meta, int grid, int reduce) {
    const int32_t *d = meta + (size_t)blockIdx.z * kLabelDesc;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= grid || y >= grid) return;
    const int half = reduce / 2;
    const int yy = reduce * y + half - d[L_CTOP], xx = reduce * x + half - d[L_CLEFT];
    uint8_t v = 255;
    if (yy >= 0 && yy < d[L_ROWS] && xx >= 0 && xx < d[L_COLS])
        v = labels[d[L_SRC] + (size_t)meta[d[L_RTAB] + yy] * d[L_W] + meta[d[L_CTAB] + xx]];
    out[((size_t)blockIdx.z * grid + y) * grid + x] = v;
}

// One index table of image `i` of the label entry: `n` entries at word `off` of meta, each inside [0, extent).
int check_index_table(const int32_t *meta, size_t meta_words, int n_images, int i, const char *axis, int64_t off, int n, int extent) {
    if (off < (int64_t)n_images * kLabelDesc || off + n > (int64_t)meta_words)
        return fail(IRN_ERR_ARG, "irn_augment_label_batch: image %d: %s table at word %lld (+%d) lies outside the %zu words passed", i, axis,
                    (long long)off, n, meta_words);
    for (int j = 0; j < n; ++j)
        if (meta[off + j] < 0 || meta[off + j] >= extent)
            return fail(IRN_ERR_ARG, "irn_augment_label_batch: image %d: %s entry %d is %d, outside the %d source cells", i, axis, j,
                        meta[off + j], extent);
    return IRN_OK;
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

extern "C" int irn_augment_label_batch(int n_images, int crop, int reduce, const int32_t *meta, size_t meta_words,
                                       const uint8_t *labels_dev, size_t labels_bytes, uint8_t *out_dev, size_t out_elems,
                                       int32_t *meta_dev, size_t meta_dev_words, void *stream) {
    if (n_images < 0) return fail(IRN_ERR_ARG, "irn_augment_label_batch: n_images must be >= 0 (got %d)", n_images);
    if (crop < 1 || crop > 65535) return fail(IRN_ERR_ARG, "irn_augment_label_batch: crop must be in 1..65535 (got %d)", crop);
    if (reduce < 1 || crop % reduce != 0)
        return fail(IRN_ERR_ARG, "irn_augment_label_batch: reduce must be >= 1 and divide the crop (got %d for crop %d)", reduce, crop);
    if (n_images == 0) return IRN_OK;
    if (!meta || !labels_dev || !out_dev || !meta_dev) return fail(IRN_ERR_ARG, "irn_augment_label_batch: null pointer");
    if (n_images > 65535) return fail(IRN_ERR_ARG, "irn_augment_label_batch: at most 65535 images per call (got %d)", n_images);
    if (meta_words < (size_t)n_images * kLabelDesc || meta_words > (size_t)INT32_MAX || meta_dev_words < meta_words)
        return fail(IRN_ERR_ARG, "irn_augment_label_batch: %zu descriptor / table words for %d images, device buffer of %zu", meta_words,
                    n_images, meta_dev_words);
    if (labels_bytes > (size_t)INT32_MAX) return fail(IRN_ERR_ARG, "irn_augment_label_batch: the label buffer is addressed with 31 bits");
    const int grid = crop / reduce;
    if (out_elems < (size_t)n_images * grid * grid)
        return fail(IRN_ERR_ARG, "irn_augment_label_batch: output of %zu bytes for [%d, %d, %d]", out_elems, n_images, grid, grid);
    for (int i = 0; i < n_images; ++i) {
        const int32_t *d = meta + (size_t)i * kLabelDesc;
        const int64_t h = d[L_H], w = d[L_W], rows = d[L_ROWS], cols = d[L_COLS];
        if (h < 1 || w < 1) return fail(IRN_ERR_ARG, "irn_augment_label_batch: image %d: bad size %lldx%lld", i, (long long)h, (long long)w);
        if (rows < 1 || cols < 1 || d[L_CTOP] < 0 || d[L_CLEFT] < 0 || d[L_CTOP] + rows > crop || d[L_CLEFT] + cols > crop)
            return fail(IRN_ERR_ARG, "irn_augment_label_batch: image %d: box %lldx%lld at (%d, %d) is not inside the %d^2 crop", i,
                        (long long)rows, (long long)cols, d[L_CTOP], d[L_CLEFT], crop);
        if (d[L_SRC] < 0 || (int64_t)d[L_SRC] + h * w > (int64_t)labels_bytes)
            return fail(IRN_ERR_ARG, "irn_augment_label_batch: image %d: labels at byte %d (+%lld) lie outside the %zu bytes passed", i,
                        d[L_SRC], (long long)(h * w), labels_bytes);
        if (int rc = check_index_table(meta, meta_words, n_images, i, "row", d[L_RTAB], (int)rows, (int)h)) return rc;
        if (int rc = check_index_table(meta, meta_words, n_images, i, "column", d[L_CTAB], (int)cols, (int)w)) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    IRN_HIP_TRY(hipMemcpyAsync(meta_dev, meta, meta_words * sizeof(int32_t), hipMemcpyHostToDevice, st));
    augment_label_kernel<<<dim3(cdiv(grid, 64), cdiv(grid, 4), n_images), dim3(64, 4), 0, st>>>(labels_dev, out_dev, meta_dev, grid, reduce);
    IRN_LAUNCH_CHECK("augment_label_kernel");
    return IRN_OK;
}
