// Evaluation counts on the GPU (include/irn_hip.h "Evaluation counts"): the confusion matrices behind
// step/eval_cam.py and step/eval_sem_seg.py and the mask_iou counts behind step/eval_ins_seg.py.
//
// Every kernel privatises its counters in LDS (one uint32 per bin, at most 4096 pixels per block, so a bin cannot
// overflow) and flushes the non-zero bins once per block with 64-bit integer atomics into the caller's int64
// accumulators.  Integer sums do not depend on arrival order: every result is exact and reproducible.  The threshold
// histogram of irn_cam_confusion is counted by thres_hist.hpp, the code the label sweep (label.hip) counts with.
#include "thres_hist.hpp"

#include <cmath>

using irn::cdiv;
using irn::fail;
namespace thist = irn::thist;
using thist::add64, thist::gt_row, thist::kRows, thist::kMaxKeys;

namespace {

constexpr int TPB = 256;                  // threads per block
constexpr int PPT = 16;                   // pixels per thread (kept in registers by the CAM kernel)
constexpr int PIX = TPB * PPT;            // pixels per block: bin counts stay below 2^32
constexpr int NC = IRN_EVAL_CLASSES;      // 21 classes (background + 20)
constexpr int CAP = 16384;                // LDS bins of one pass of the CAM kernel (64 KiB)
static_assert(TPB == thist::kThreads, "thres_hist.hpp counts with blocks of this size");

// ---------------------------------------------------------------------------------------------------------------------
// CAM confusion, counting pass: per pixel the GT row, the first arg-max plane c and the maximum m; the bins and their
// counting are thres_hist.hpp's.  Without planes (k = 0) every pixel predicts class 0: one channel whose column is 0.
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) k_cam_hist(const float *__restrict__ cam, const int64_t *__restrict__ keys, int k,
                                                  const uint8_t *__restrict__ gt, int n, const float *__restrict__ thres,
                                                  int t, int64_t *__restrict__ hist, int64_t *__restrict__ bad) {
    __shared__ uint32_t bins[CAP];
    __shared__ float th[IRN_EVAL_MAX_THRES];
    __shared__ int col[kMaxKeys];
    __shared__ uint32_t nbad;
    const int tid = threadIdx.x;
    if (k == 0 && tid == 0) col[0] = 0;
    uint32_t local_bad = thist::stage(thres, t, keys, k, blockIdx.x == 0, th, col, &nbad);

    const int kc = k > 0 ? k : 1;
    uint32_t bin[PPT];
    const int base = blockIdx.x * PIX + tid;
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        bin[i] = thist::kSkip;
        const int p = base + i * TPB;
        if (p >= n) continue;
        const int row = gt_row(gt[p]);
        if (row < 0) {
            ++local_bad;
            continue;
        }
        if (k == 0) {
            bin[i] = thist::bin_of(0, row, 0, kc);
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
        bin[i] = thist::bin_of(thist::count_below(th, t, m), row, c, kc);
    }
    local_bad += thist::count(bin, bins, CAP, (uint32_t)(t + 1) * kRows * (uint32_t)kc, kc, col, t, hist);
    thist::flush_bad(local_bad, &nbad, bad);
}

// hist [22][21][t+1] -> conf [t][21][21] (+ void [t][21]).  One thread per (row, column) of the histogram: a pixel of
// column c >= 1 and count j predicts c at thresholds 0..j-1 and 0 from j on; column 0 predicts 0 throughout.
__global__ void __launch_bounds__(TPB) k_cam_reduce(const int64_t *__restrict__ hist, int t, int64_t *__restrict__ conf,
                                                    int64_t *__restrict__ void_) {
    const int id = blockIdx.x * TPB + threadIdx.x;
    if (id >= kRows * NC) return;
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
// label confusion: bins [22][21] per block
// ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TPB) k_label_hist(const uint8_t *__restrict__ pred, const uint8_t *__restrict__ gt, int n,
                                                    int map255, int64_t *__restrict__ conf, int64_t *__restrict__ void_,
                                                    int64_t *__restrict__ bad) {
    __shared__ uint32_t bins[kRows * NC];
    __shared__ uint32_t nbad;
    const int tid = threadIdx.x;
    for (int b = tid; b < kRows * NC; b += TPB) bins[b] = 0;
    if (tid == 0) nbad = 0;
    __syncthreads();
    uint32_t local_bad = 0;
    const int base = blockIdx.x * PIX + tid;
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        const int p = base + i * TPB;
        if (p >= n) continue;
        const int row = gt_row(gt[p]);
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
    for (int b = tid; b < kRows * NC; b += TPB) {
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

bool pixels_ok(int h, int w) { return h >= 1 && w >= 1 && (int64_t)h * w <= (int64_t)0x7fffffff - PIX; }

}  // namespace

extern "C" int irn_cam_confusion(const float *high_res_dev, const int64_t *keys_dev, int k, const uint8_t *gt_dev, int h,
                                 int w, const float *thres_dev, int t, int64_t *hist_dev, int64_t *bad_dev, void *stream) {
    if (!gt_dev || !thres_dev || !hist_dev || !bad_dev || k < 0 || k > kMaxKeys || (k > 0 && (!high_res_dev || !keys_dev)) ||
        t < 1 || t > IRN_EVAL_MAX_THRES || !pixels_ok(h, w))
        return fail(IRN_ERR_ARG, "irn_cam_confusion: bad argument (k=%d, h=%d, w=%d, t=%d; 0 <= k <= %d, 1 <= t <= %d)",
                    k, h, w, t, kMaxKeys, IRN_EVAL_MAX_THRES);
    const int n = h * w;
    hipLaunchKernelGGL(k_cam_hist, dim3(cdiv(n, PIX)), dim3(TPB), 0, (hipStream_t)stream, high_res_dev, keys_dev, k, gt_dev,
                       n, thres_dev, t, hist_dev, bad_dev);
    IRN_LAUNCH_CHECK("k_cam_hist");
    return IRN_OK;
}

extern "C" int irn_cam_confusion_reduce(const int64_t *hist_dev, int t, int64_t *conf_dev, int64_t *void_dev,
                                        void *stream) {
    if (!hist_dev || !conf_dev || t < 1 || t > IRN_EVAL_MAX_THRES)
        return fail(IRN_ERR_ARG, "irn_cam_confusion_reduce: bad argument (t=%d)", t);
    hipLaunchKernelGGL(k_cam_reduce, dim3(cdiv(kRows * NC, TPB)), dim3(TPB), 0, (hipStream_t)stream, hist_dev, t, conf_dev,
                       void_dev);
    IRN_LAUNCH_CHECK("k_cam_reduce");
    return IRN_OK;
}

extern "C" int irn_label_confusion(const uint8_t *pred_dev, const uint8_t *gt_dev, int h, int w, int pred_255_as,
                                   int64_t *conf_dev, int64_t *void_dev, int64_t *bad_dev, void *stream) {
    if (!pred_dev || !gt_dev || !conf_dev || !bad_dev || pred_255_as >= NC || !pixels_ok(h, w))
        return fail(IRN_ERR_ARG, "irn_label_confusion: bad argument (h=%d, w=%d, pred_255_as=%d)", h, w, pred_255_as);
    const int n = h * w;
    hipLaunchKernelGGL(k_label_hist, dim3(cdiv(n, PIX)), dim3(TPB), 0, (hipStream_t)stream, pred_dev, gt_dev, n,
                       pred_255_as, conf_dev, void_dev, bad_dev);
    IRN_LAUNCH_CHECK("k_label_hist");
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
