// The threshold histogram hist[ncls+1][ncls][t+1] of irn_cam_confusion (eval.hip) and irn_label_sweep_confusion
// (label.hip): one device copy, since irn_cam_confusion_reduce reduces both.  ncls = classes including the background, a
// launch argument (2..IRN_EVAL_MAX_CLASSES; the entries without the argument hand over IRN_EVAL_CLASSES).  A kernel decides
// per pixel the GT row, the first arg-max channel c, its maximum m and what a NaN means; the rest is here.  With
// j = count_below(th, t, m) the pixel is one count in bin (j * (ncls+1) + row) * nc + c of its image (nc channels).  A
// thread keeps its pixels' bins in registers (kSkip = none);
// `count` adds them up in uint32 LDS bins private to the block (at most 4096 pixels per call: no overflow), in passes over
// bin ranges of `cap`, and flushes the non-zero ones with 64-bit integer atomics into hist[row][col[c]][j]: exact
// whatever the grid and the arrival order.  col[c] = key + 1, or -1 for a key outside 0..ncls-2 (its pixels count as bad).
// Blocks of kThreads threads; everything inlines, so a constant `cap` folds.  Integer arithmetic and float comparisons
// only: the contraction setting of the including file (label.hip: off, eval.hip: default) cannot change a result.
#pragma once
#include "common.hpp"

namespace irn::thist {

constexpr int kThreads = 256;
constexpr int kMaxKeys = IRN_EVAL_MAX_CLASSES - 1;  // most channels (class keys) per image at the largest class count: col[]
constexpr uint32_t kSkip = 0xffffffffu;

__device__ __forceinline__ void add64(int64_t *p, uint32_t v) {
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
}

__host__ __device__ constexpr bool classes_ok(int ncls) { return ncls >= 2 && ncls <= IRN_EVAL_MAX_CLASSES; }

// GT byte -> histogram row (0..ncls-1, ncls = void) or -1 = out of range
__device__ __forceinline__ int gt_row(uint8_t g, int ncls) { return (int)g < ncls ? (int)g : (g == 255 ? ncls : -1); }

// Thresholds into th[IRN_EVAL_MAX_THRES], the columns of keys[0..k) into col[kMaxKeys], *nbad = 0, a barrier.  -> in the one
// block of a call for which `checks` holds, the NaN thresholds and descending pairs (the counts follow the list as given).
__device__ __forceinline__ uint32_t stage(const float *__restrict__ thres, int t, const int64_t *__restrict__ keys, int k,
                                          bool checks, int ncls, float *th, int *col, uint32_t *nbad) {
    const int tid = threadIdx.x;
    if (tid == 0) *nbad = 0;
    for (int i = tid; i < t; i += kThreads) th[i] = thres[i];
    if (tid < k) col[tid] = (keys[tid] >= 0 && keys[tid] < ncls - 1) ? (int)keys[tid] + 1 : -1;
    __syncthreads();
    uint32_t local_bad = 0;
    for (int i = tid; checks && i < t; i += kThreads)
        if (th[i] != th[i] || (i > 0 && !(th[i - 1] <= th[i]))) ++local_bad;
    return local_bad;
}

// number of thresholds < m: the lower bound in the ascending list
__device__ __forceinline__ int count_below(const float *th, int t, float m) {
    int lo = 0, hi = t;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (th[mid] < m) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t bin_of(int j, int row, int c, int nc, int ncls) {
    return ((uint32_t)j * (uint32_t)(ncls + 1) + (uint32_t)row) * (uint32_t)nc + (uint32_t)c;
}

// Counts the block's bin[] into hist through bins[cap].  -> this thread's share of the pixels whose key is out of range.
template <int N>
__device__ __forceinline__ uint32_t count(const uint32_t (&bin)[N], uint32_t *bins, uint32_t cap, uint32_t nbins, int nc,
                                          const int *col, int t, int ncls, int64_t *__restrict__ hist) {
    const uint32_t rows = (uint32_t)(ncls + 1);
    uint32_t local_bad = 0;
    for (uint32_t b0 = 0; b0 < nbins; b0 += cap) {
        const uint32_t nb = min(cap, nbins - b0);
        for (uint32_t b = threadIdx.x; b < nb; b += kThreads) bins[b] = 0;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (bin[i] - b0 < nb) atomicAdd(&bins[bin[i] - b0], 1u);
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < nb; b += kThreads) {
            const uint32_t v = bins[b];
            if (!v) continue;
            const uint32_t id = b0 + b, r = id / (uint32_t)nc;
            const int c = (int)(id % (uint32_t)nc), row = (int)(r % rows), j = (int)(r / rows);
            if (col[c] < 0) local_bad += v;        // a key outside 0..ncls-2: its pixels are out of range
            else add64(hist + ((size_t)row * ncls + col[c]) * (t + 1) + j, v);
        }
        __syncthreads();
    }
    return local_bad;
}

// the block's bad counts into *bad, with one atomic
__device__ __forceinline__ void flush_bad(uint32_t local_bad, uint32_t *nbad, int64_t *__restrict__ bad) {
    if (local_bad) atomicAdd(nbad, local_bad);
    __syncthreads();
    if (threadIdx.x == 0 && *nbad) add64(bad, *nbad);
}

}  // namespace irn::thist
