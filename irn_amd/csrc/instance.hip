// Instance front-end (gfx950): displacement-field centroid refinement, 4-connected component
// labelling with raster-order ids, centroid clustering.
//
// Replaces reference step/make_ins_seg_labels.py:18-75 (300 numpy iterations of bilinear gather on
// the CPU; skimage.measure.label; misc/imutils.compress_range).  Every pixel's trajectory is
// independent, so the refinement is one thread per pixel; dp (2*h*w fp32 = 128 KB at 128^2) stays
// in L2.  Bit-exactness with numpy needs the reference's mixed precision replayed exactly
// (SURVEY.md §3.5): float32 state, float64 increment evaluated left to right with NO fused
// multiply-add, float32 rounding after each +=, round-half-even at the end.
#include "kernels.hpp"

#include <climits>
#include <rocprim/rocprim.hpp>

namespace irn {
namespace {

// ---------------------------------------------------------------------------------------------
// find_centroids_with_refinement
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double bilinear_inc(const float *__restrict__ f, int w, int uy, int ly, int ux,
                                               int lx, double fy, double fx) {
    // f[uy,ux]*fy*fx + f[ly,ux]*(1-fy)*fx + f[uy,lx]*fy*(1-fx) + f[ly,lx]*(1-fy)*(1-fx)
    // (step/make_ins_seg_labels.py:39-42), float32 * float64 -> float64, evaluated left to right
    const double gy = __dsub_rn(1.0, fy), gx = __dsub_rn(1.0, fx);
    const double t0 = __dmul_rn(__dmul_rn((double)f[uy * w + ux], fy), fx);
    const double t1 = __dmul_rn(__dmul_rn((double)f[ly * w + ux], gy), fx);
    const double t2 = __dmul_rn(__dmul_rn((double)f[uy * w + lx], fy), gx);
    const double t3 = __dmul_rn(__dmul_rn((double)f[ly * w + lx], gy), gx);
    return __dadd_rn(__dadd_rn(__dadd_rn(t0, t1), t2), t3);
}

struct CenJob {
    const float *dp;     // [2,h,w]
    int32_t *out;        // [2,h,w]
    int h, w;
};

// grid.y = image of the batch (every pixel's trajectory is independent; a batch fills the chip where one 128x128
// image is 64 workgroups of latency-bound gathers)
__global__ __launch_bounds__(256) void centroid_kernel(const CenJob *__restrict__ jobs, int iters) {
    const CenJob J = jobs[blockIdx.y];
    const float *__restrict__ dp = J.dp;
    int32_t *__restrict__ out = J.out;
    const int h = J.h, w = J.w;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int n = h * w;
    if (p >= n) return;
    const float *dy_f = dp, *dx_f = dp + n;
    float cy = (float)(p / w), cx = (float)(p % w);
    const float ymax = (float)(h - 1), xmax = (float)(w - 1);
    for (int it = 0; it < iters; ++it) {
        const float cyu = ceilf(cy), cyl = floorf(cy), cxu = ceilf(cx), cxl = floorf(cx);
        const int uy = (int)cyu, ly = (int)cyl, ux = (int)cxu, lx = (int)cxl;
        const double fy = __dsub_rn((double)cy, (double)ly);   // float32 - int32 -> float64 in numpy
        const double fx = __dsub_rn((double)cx, (double)lx);
        const double iy = bilinear_inc(dy_f, w, uy, ly, ux, lx, fy, fx);
        const double ix = bilinear_inc(dx_f, w, uy, ly, ux, lx, fy, fx);
        cy = (float)__dadd_rn((double)cy, iy);                 // in-place += rounds back to float32
        cx = (float)__dadd_rn((double)cx, ix);
        cy = fminf(fmaxf(cy, 0.f), ymax);
        cx = fminf(fmaxf(cx, 0.f), xmax);
    }
    out[p] = (int32_t)rintf(cy);       // np.round: half to even
    out[n + p] = (int32_t)rintf(cx);
}

// ---------------------------------------------------------------------------------------------
// 4-connected component labelling: union-find with "smaller root wins", so a component's root
// is its first pixel in raster order; ids = rank of the root among roots (+1).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int uf_find(const int *parent, int a) {
    int r = a;
    while (true) {
        const int q = __hip_atomic_load(parent + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (q == r) return r;
        r = q;
    }
}

__device__ __forceinline__ void uf_union(int *parent, int a, int b) {
    while (true) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        // hang the larger root b under the smaller root a, unless b stopped being a root meanwhile
        const int old = atomicMin(parent + b, a);
        if (old == b) return;
        b = old;
    }
}

// The passes over a forest are written once, for every job type with the members parent, h and w (grid.y = image).
// Merge: every pixel of the mask (parent >= 0) is joined with its left and its upper neighbour.
template <class Job>
__global__ __launch_bounds__(256) void forest_merge_kernel(const Job *__restrict__ jobs) {
    const Job J = jobs[blockIdx.y];
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= J.h * J.w) return;
    int *parent = J.parent;
    if (parent[p] < 0) return;
    const int y = p / J.w, x = p - y * J.w;
    if (x > 0 && parent[p - 1] >= 0) uf_union(parent, p, p - 1);
    if (y > 0 && parent[p - J.w] >= 0) uf_union(parent, p, p - J.w);
}

// Flatten: every pixel points at its root.
template <class Job>
__global__ __launch_bounds__(256) void forest_flatten_kernel(const Job *__restrict__ jobs) {
    const Job J = jobs[blockIdx.y];
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= J.h * J.w) return;
    int *parent = J.parent;
    if (parent[p] < 0) return;
    // roots never change in this pass (all unions are done), so plain chasing is race-free
    int r = p;
    while (parent[r] != r) r = parent[r];
    parent[p] = r;   // may shortcut another thread's chase; every value it can read still leads to r
}

// Exclusive prefix of `cnt` over the 1024 threads of a workgroup (Hillis-Steele in LDS); the workgroup's total is left in
// sums[1023], visible to every thread.
__device__ __forceinline__ int block_scan_1024(int cnt, int *sums) {
    sums[threadIdx.x] = cnt;
    __syncthreads();
    for (int s = 1; s < 1024; s <<= 1) {
        const int v = threadIdx.x >= s ? sums[threadIdx.x - s] : 0;
        __syncthreads();
        sums[threadIdx.x] += v;
        __syncthreads();
    }
    return sums[threadIdx.x] - cnt;
}

// One workgroup of 1024 threads per image, each with a chunk of consecutive pixels: rank[root] = 1 + number of roots
// before it in raster order (skimage numbering).  The number of roots is left in sums[1023].
__device__ __forceinline__ void rank_roots(const int *parent, int *rank, int npx, int *sums) {
    const int chunk = (npx + 1023) / 1024;
    const int lo = min(npx, (int)threadIdx.x * chunk), hi = min(npx, lo + chunk);
    int cnt = 0;
    for (int p = lo; p < hi; ++p) cnt += (parent[p] == p);
    int run = block_scan_1024(cnt, sums);
    for (int p = lo; p < hi; ++p)
        if (parent[p] == p) rank[p] = ++run;
}

// irn_label4: one job per image of the [n,h,w] stack
struct CclJob {
    const uint8_t *mask;   // [h,w]
    int *parent, *rank;    // [npx] each; rank is separate from `labels`: relabel overwrites roots other pixels still need
    int32_t *labels;       // [h,w] out
    int32_t *n_labels;     // -> the image's component count, or null
    int h, w;
};

__global__ __launch_bounds__(256) void ccl_init_kernel(const CclJob *__restrict__ jobs) {
    const CclJob J = jobs[blockIdx.y];
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= J.h * J.w) return;
    J.parent[p] = J.mask[p] ? p : -1;
}

__global__ __launch_bounds__(1024) void ccl_rank_kernel(const CclJob *__restrict__ jobs) {
    __shared__ int sums[1024];
    const CclJob J = jobs[blockIdx.x];
    rank_roots(J.parent, J.rank, J.h * J.w, sums);
    if (threadIdx.x == 1023 && J.n_labels) *J.n_labels = sums[1023];
}

__global__ __launch_bounds__(256) void ccl_relabel_kernel(const CclJob *__restrict__ jobs) {
    const CclJob J = jobs[blockIdx.y];
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= J.h * J.w) return;
    const int r = J.parent[p];
    J.labels[p] = r < 0 ? 0 : J.rank[r];
}

// ---------------------------------------------------------------------------------------------
// cluster_centroids, batched (grid.y or grid.x = image): K of every image stays on the device, the caller reads
// all of them with ONE transfer per batch (step/make_ins_seg_labels.py:58-75 returns K to the host per image).
// ---------------------------------------------------------------------------------------------
struct ClusterJob {
    const int32_t *centroids;   // [2,h,w]
    const float *dp;            // [2,h,w]
    int32_t *cluster_map;       // [h,w] out
    int *parent, *rank;         // [npx] union-find forest of the weak-displacement mask / rank of its roots
    int32_t *picked;            // [npx]
    int *present;               // [npx + 2]
    int32_t *k_out;             // -> k_dev[i]
    int h, w;
};

// weak = |dp| < thres, np.sqrt(dp[1]**2 + dp[0]**2) in float32 with every operation rounded
// (step/make_ins_seg_labels.py:61); forest initialised on the mask; `present` cleared
__global__ __launch_bounds__(256) void cluster_init_kernel(const ClusterJob *__restrict__ jobs, float thres) {
    const ClusterJob J = jobs[blockIdx.y];
    const int n = J.h * J.w;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < 2) J.present[n + p] = 0;
    if (p >= n) return;
    const float a = J.dp[n + p], b = J.dp[p];
    const float s = __fsqrt_rn(__fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)));
    J.parent[p] = s < thres ? p : -1;
    J.present[p] = 0;
}

__global__ __launch_bounds__(1024) void cluster_rank_kernel(const ClusterJob *__restrict__ jobs) {
    __shared__ int sums[1024];
    const ClusterJob J = jobs[blockIdx.x];
    rank_roots(J.parent, J.rank, J.h * J.w, sums);
}

// picked[p] = label at centroid(p) (+1, as the reference adds before compress_range); mark presence
__global__ __launch_bounds__(256) void cluster_pick_kernel(const ClusterJob *__restrict__ jobs) {
    const ClusterJob J = jobs[blockIdx.y];
    const int n = J.h * J.w;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int c = J.centroids[p] * J.w + J.centroids[n + p];
    const int root = J.parent[c];
    const int v = (root < 0 ? 0 : J.rank[root]) + 1;
    J.picked[p] = v;
    J.present[v] = 1;
}

// one workgroup per image: renumber the distinct values of `picked` ascending to 0..K-1 (compress_range,
// misc/imutils.py:182-190; its final "- min" is a no-op because the smallest value maps to 0)
__global__ __launch_bounds__(1024) void cluster_compress_kernel(const ClusterJob *__restrict__ jobs) {
    __shared__ int sums[1024];
    const ClusterJob J = jobs[blockIdx.x];
    int *present = J.present;
    const int n_vals = J.h * J.w + 2;       // label values lie in [0, npx/2+1]; +1 shifts them to [1, npx/2+2]
    const int chunk = (n_vals + 1023) / 1024;
    const int lo = min(n_vals, (int)threadIdx.x * chunk), hi = min(n_vals, lo + chunk);
    int cnt = 0;
    for (int v = lo; v < hi; ++v) cnt += present[v] != 0;
    int run = block_scan_1024(cnt, sums);
    for (int v = lo; v < hi; ++v) present[v] = present[v] ? run++ : -1;   // now: new id of value v
    if (threadIdx.x == 1023) *J.k_out = sums[1023];
}

__global__ __launch_bounds__(256) void cluster_remap_kernel(const ClusterJob *__restrict__ jobs) {
    const ClusterJob J = jobs[blockIdx.y];
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= J.h * J.w) return;
    J.cluster_map[p] = J.present[J.picked[p]];
}

// ---------------------------------------------------------------------------------------------
// detect_instance (reference step/make_ins_seg_labels.py:82-105) on the device, batched over images.
//
// The reference labels the 4-connected components of every channel's mask separately; the masks are
// the one-hot planes of ONE argmax map (:145-147), so they are disjoint and all components come
// out of a single labelling pass over the class map (neighbours join when their classes agree).
// Detections are ordered like the reference's: channel ascending, then skimage's label order =
// raster order of each component's first pixel = of its union-find root.
// ---------------------------------------------------------------------------------------------
struct DetJob {
    const float *rw_up;         // [n_channels,h,w]
    const int32_t *cls;         // [h,w] argmax (0 = background, c+1 = channel c)
    int *parent, *prov, *newid, *area, *score_bits;   // [npx] each
    long long *keys;            // [npx]
    int32_t *counter;           // -> n_det_dev[i]
    float *score;               // [n_det]      (emit)
    int32_t *channel;           // [n_det]      (emit)
    uint8_t *mask;              // [n_det,h,w]  (emit)
    double min_area;
    int h, w, n_det;
};

// what the run-length entries keep per image next to its DetJob (see "Detections as COCO run lengths" below)
struct RleJob {
    int *idmap;                       // [npx] detection of every pixel, -1 = background
    int *x0, *x1, *y0, *y1, *runs;    // [n_det] box corners (inclusive) and number of run lengths
    int32_t *area_out, *n_runs_out, *bbox_out;   // the image's slice of the batch's outputs (count)
    unsigned long long *keys;         // the image's key segment (emit)
    unsigned *cursor;                 // keys appended so far, after the n_det map-end keys (emit)
    int room;                         // keys of the image = sum of its n_runs (emit)
    int g0;                           // index of the image's first detection in the batch
    int h, w, n_det;
};

// Labelling, stage 1: every 64 x 16 tile is labelled in LDS.  Row runs come from a segmented scan over the 16 lanes of a
// row (4 pixels per lane) — no atomics; runs of adjacent rows are joined by an LDS union-find ("smaller index wins": local
// raster order agrees with the image's inside a tile, so a local root is the component's first pixel of the tile), one
// union per PAIR of touching runs, not per pixel.  Every pixel leaves with parent = its local root's image index.  Per-pixel
// global atomics over the whole map (round 1-4: 0.056 ms per 512^2 image, the largest item of the instance stage,
// profiles/r05_s1_ins_breakdown_r5.txt) remain only along the tile borders (stage 2).
constexpr int kDetTW = 64, kDetTH = 16;

__device__ __forceinline__ int lds_find(volatile int *parent, int a) {
    int r = a;
    while (true) {
        const int q = parent[r];
        if (q == r) return r;
        r = q;
    }
}

__device__ __forceinline__ void lds_union(int *parent, int a, int b) {
    while (true) {
        a = lds_find(parent, a);
        b = lds_find(parent, b);
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(parent + b, a);
        if (old == b) return;
        b = old;
    }
}

__global__ __launch_bounds__(256) void det_local_kernel(const DetJob *__restrict__ jobs) {
    __shared__ int s_cls[kDetTH * kDetTW];
    __shared__ int s_parent[kDetTH * kDetTW];
    const DetJob J = jobs[blockIdx.y];
    const int H = J.h, W = J.w;
    const int tiles_x = (W + kDetTW - 1) / kDetTW, tiles_y = (H + kDetTH - 1) / kDetTH;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * kDetTH, x0 = tx * kDetTW;
    const int t = threadIdx.x, ly = t >> 4, lane16 = t & 15, lx0 = lane16 * 4;
    const int gy = y0 + ly, gx0 = x0 + lx0;
    const int idx0 = ly * kDetTW + lx0;
    int c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = (gy < H && gx0 + j < W) ? J.cls[(long)gy * W + gx0 + j] : 0;
    // links to the left neighbour inside the tile row
    int left = __shfl_up(c[3], 1, 16);
    if (lane16 == 0) left = -1;
    bool link[4];
    link[0] = c[0] > 0 && c[0] == left;
#pragma unroll
    for (int j = 1; j < 4; ++j) link[j] = c[j] > 0 && c[j] == c[j - 1];
    // run start of the lane's LAST pixel: `pass` = the incoming start runs through all four pixels
    bool pass = link[0] && link[1] && link[2] && link[3];
    int val = idx0 + 3;
#pragma unroll
    for (int j = 3; j >= 1; --j) {
        if (!link[j]) break;
        val = idx0 + j - 1;
    }
    // (val is only used when !pass: the start of the run that contains pixel 3)
    // inclusive segmented scan over the row's 16 lanes
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
        const int pv = __shfl_up(val, d, 16);
        const int pp = __shfl_up((int)pass, d, 16);
        if (lane16 >= d && pass) {
            val = pv;
            pass = pp != 0;
        }
    }
    int incoming = __shfl_up(val, 1, 16);     // run start of the left lane's last pixel (unused when !link[0])
    int start[4];
    int cur = link[0] ? incoming : idx0;
    start[0] = cur;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        cur = link[j] ? cur : idx0 + j;
        start[j] = cur;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s_cls[idx0 + j] = c[j];
        s_parent[idx0 + j] = c[j] > 0 ? start[j] : -1;
    }
    __syncthreads();
    if (ly > 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int up = idx0 + j - kDetTW;
            if (c[j] > 0 && s_cls[up] == c[j]) {
                // one union per pair of touching runs: where either run begins
                const bool here = start[j] == idx0 + j;
                const bool there = lx0 + j == 0 || s_cls[up - 1] != c[j];
                if (here || there) lds_union(s_parent, start[j], up);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (gy < H && gx0 + j < W) {
            int out = -1;
            if (c[j] > 0) {
                const int r = lds_find(s_parent, start[j]);
                out = (y0 + r / kDetTW) * W + x0 + (r % kDetTW);
            }
            J.parent[(long)gy * W + gx0 + j] = out;
        }
    }
}

// Labelling, stage 2: components are joined across tile borders — one global union per pair of touching border runs.
__global__ __launch_bounds__(256) void det_border_kernel(const DetJob *__restrict__ jobs) {
    const DetJob J = jobs[blockIdx.y];
    const int H = J.h, W = J.w;
    const int rows = (H + kDetTH - 1) / kDetTH - 1, cols = (W + kDetTW - 1) / kDetTW - 1;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int32_t *__restrict__ cls = J.cls;
    if (i < rows * W) {
        const int r = i / W, x = i - r * W;
        const int p = (r + 1) * kDetTH * W + x;
        const int c = cls[p];
        // (a border run restarts at every tile corner: p and p - 1 are only joined inside ONE tile)
        if (c > 0 && cls[p - W] == c && (x % kDetTW == 0 || cls[p - 1] != c || cls[p - W - 1] != c)) uf_union(J.parent, p, p - W);
        return;
    }
    const int k = i - rows * W;
    if (k < cols * H) {
        const int q = k / H, y = k - q * H;
        const int p = y * W + (q + 1) * kDetTW;
        const int c = cls[p];
        if (c > 0 && cls[p - 1] == c && (y % kDetTH == 0 || cls[p - W] != c || cls[p - W - 1] != c)) uf_union(J.parent, p, p - 1);
    }
}

// Every root (= first raster pixel of its component) claims a provisional id and records its sort key
// channel * npx + pixel: detections are ordered channel ascending, then by first pixel (skimage's
// label order inside a channel).
__global__ __launch_bounds__(256) void det_roots_kernel(const DetJob *__restrict__ jobs) {
    const DetJob J = jobs[blockIdx.y];
    const int npx = J.h * J.w;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= npx) return;
    if (J.parent[p] == p) {
        const int id = atomicAdd(J.counter, 1);
        J.prov[p] = id;
        J.keys[id] = (long long)(J.cls[p] - 1) * npx + p;
    }
}

// final id of provisional detection i = number of keys below its own (keys are distinct).  A handful to a few
// hundred detections is the normal case; a noisy class map can have tens of thousands of fragments, so the n^2
// comparisons are spread over ceil(n / 256) workgroups per image with the keys staged through LDS (the reference's
// labelling is linear in the fragment count; one 1024-thread workgroup would stall for seconds).  Also zeroes the
// statistics.
__global__ __launch_bounds__(256) void det_order_kernel(const DetJob *__restrict__ jobs) {
    __shared__ long long tile[1024];
    const DetJob J = jobs[blockIdx.y];
    const int n = J.n_det;
    if ((int)blockIdx.x * 256 >= n) return;
    const int npx = J.h * J.w;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const long long k = i < n ? J.keys[i] : 0;
    int r = 0;
    for (int base = 0; base < n; base += 1024) {
        const int cnt = min(1024, n - base);
        for (int j = threadIdx.x; j < cnt; j += 256) tile[j] = J.keys[base + j];
        __syncthreads();
        for (int j = 0; j < cnt; ++j) r += tile[j] < k;
        __syncthreads();
    }
    if (i < n) {
        J.newid[i] = r;
        J.channel[r] = (int32_t)(k / npx);
        J.area[i] = 0;
        J.score_bits[i] = 0;
    }
}

__global__ __launch_bounds__(256) void det_zero_masks_kernel(const DetJob *__restrict__ jobs) {
    const DetJob J = jobs[blockIdx.y];
    const size_t total = (size_t)J.n_det * J.h * J.w;
    if (total == 0) return;
    uint8_t *m = J.mask;
    // bytes up to the first 16-byte boundary, 16-byte stores for the body, bytes for the tail
    const size_t pre = std::min(total, (size_t)((16 - ((uintptr_t)m & 15)) & 15));
    const size_t n16 = (total - pre) / 16;
    uint4 *m16 = reinterpret_cast<uint4 *>(m + pre);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) m16[i] = make_uint4(0, 0, 0, 0);
    if (blockIdx.x == 0) {
        for (size_t i = threadIdx.x; i < pre; i += 256) m[i] = 0;
        for (size_t i = pre + n16 * 16 + threadIdx.x; i < total; i += 256) m[i] = 0;
    }
}

// Pixel p belongs to detection newid[prov[root(p)]]; area / max score per detection.  Scores are compared as int bit
// patterns: the reference takes max(score * mask), which is >= 0 whatever the scores are, and so is a maximum that
// starts from +0.  The dense form (RLE = false, rjobs unused) sets the pixel's byte in its detection's mask plane; the
// run-length form stores the id (-1 = background) in the image's id map and keeps the box next to area and score.
template <bool RLE>
__global__ __launch_bounds__(256) void det_stats_kernel(const DetJob *__restrict__ jobs, const RleJob *__restrict__ rjobs) {
    const DetJob J = jobs[blockIdx.y];
    if (J.n_det < 1) return;
    const int npx = J.h * J.w;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int c = p < npx ? J.cls[p] : 0;
    const bool fg = c > 0;
    int d = -1, bits = 0;
    if (fg) {
        d = J.newid[J.prov[J.parent[p]]];
        if (!RLE) J.mask[(long)d * npx + p] = 1;
        const float sc = J.rw_up[(long)(c - 1) * npx + p];
        bits = sc > 0.f ? __float_as_int(sc) : 0;
    }
    const RleJob R = RLE ? rjobs[blockIdx.y] : RleJob{};
    const int y = p / J.w, x = p - y * J.w;
    if (RLE && p < npx) R.idmap[p] = d;
    // A wave's 64 consecutive pixels nearly always lie in ONE detection: one set of atomics per wave then
    // (per-pixel atomics onto a handful of addresses took 1.4 ms per 512^2 image — 80 % of the whole step).
    const unsigned long long act = __ballot(fg);
    if (act == 0) return;
    const int d0 = __shfl(d, __ffsll((long long)act) - 1);
    if (__all(!fg || d == d0)) {
        int mx = bits, xa = fg ? x : INT_MAX, xb = fg ? x : -1, ya = fg ? y : INT_MAX, yb = fg ? y : -1;
        for (int sft = 32; sft > 0; sft >>= 1) {
            mx = max(mx, __shfl_xor(mx, sft));
            if (RLE) {
                xa = min(xa, __shfl_xor(xa, sft)), xb = max(xb, __shfl_xor(xb, sft));
                ya = min(ya, __shfl_xor(ya, sft)), yb = max(yb, __shfl_xor(yb, sft));
            }
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(J.area + d0, __popcll(act));
            if (mx > 0) atomicMax(J.score_bits + d0, mx);
            if (RLE) {
                atomicMin(R.x0 + d0, xa), atomicMax(R.x1 + d0, xb);
                atomicMin(R.y0 + d0, ya), atomicMax(R.y1 + d0, yb);
            }
        }
    } else if (fg) {
        atomicAdd(J.area + d, 1);
        if (bits > 0) atomicMax(J.score_bits + d, bits);
        if (RLE) {
            atomicMin(R.x0 + d, x), atomicMax(R.x1 + d, x);
            atomicMin(R.y0 + d, y), atomicMax(R.y1 + d, y);
        }
    }
}

// a detection below the area threshold keeps its place and scores 0; statistics are kept by FINAL id
__device__ __forceinline__ float final_score(int area, double min_area, int bits) {
    return ((double)area < min_area) ? 0.f : __int_as_float(bits);
}

__global__ __launch_bounds__(256) void det_final_kernel(const DetJob *__restrict__ jobs) {
    const DetJob J = jobs[blockIdx.y];
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= J.n_det) return;
    J.score[d] = final_score(J.area[d], J.min_area, J.score_bits[d]);
}

}  // namespace
}  // namespace irn

using namespace irn;

extern "C" int irn_find_centroids_batch(int n_images, const float *const *dp_dev, const int32_t *h, const int32_t *w,
                                        int iterations, int32_t *const *centroids_dev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_images < 1 || !dp_dev || !h || !w || !centroids_dev || iterations < 0)
        return fail(IRN_ERR_ARG, "irn_find_centroids_batch: bad argument");
    std::vector<CenJob> jobs(n_images);
    int max_n = 0;
    for (int i = 0; i < n_images; ++i) {
        if (!dp_dev[i] || !centroids_dev[i] || h[i] < 1 || w[i] < 1)
            return fail(IRN_ERR_ARG, "irn_find_centroids_batch: image %d: bad argument", i);
        jobs[i] = CenJob{dp_dev[i], centroids_dev[i], h[i], w[i]};
        max_n = std::max(max_n, h[i] * w[i]);
    }
    CenJob *jobs_dev = nullptr;
    int rc = scratch_upload(jobs.data(), sizeof(CenJob) * n_images, (void **)&jobs_dev, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(centroid_kernel, dim3(cdiv(max_n, 256), n_images), dim3(256), 0, stream, jobs_dev, iterations);
    IRN_LAUNCH_CHECK("centroid_kernel");
    return scratch_release(stream);
}

extern "C" size_t irn_ccl_scratch_bytes(int n, int h, int w) {
    if (n < 1 || h < 1 || w < 1) return 0;
    return round_up(sizeof(int) * 2 * (size_t)n * h * w, 256);
}

extern "C" int irn_label4(const uint8_t *mask_dev, int n, int h, int w, int32_t *labels_dev, int32_t *n_labels_dev,
                          void *scratch_dev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!mask_dev || !labels_dev || !scratch_dev || n < 1 || h < 1 || w < 1)
        return fail(IRN_ERR_ARG, "irn_label4: bad argument");
    if ((long)h * w > (1L << 30)) return fail(IRN_ERR_ARG, "irn_label4: image too large");
    if (n > 65535) return fail(IRN_ERR_ARG, "irn_label4: at most 65535 images per call");   // grid.y = image
    const int npx = h * w;
    int *parent = (int *)scratch_dev, *rank = parent + (size_t)n * npx;
    std::vector<CclJob> jobs(n);
    for (int i = 0; i < n; ++i) {
        const size_t at = (size_t)i * npx;
        jobs[i] = CclJob{mask_dev + at, parent + at, rank + at, labels_dev + at, n_labels_dev ? n_labels_dev + i : nullptr, h, w};
    }
    CclJob *jd = nullptr;
    int rc = scratch_upload(jobs.data(), sizeof(CclJob) * n, (void **)&jd, stream);
    if (rc) return rc;
    const dim3 px(cdiv(npx, 256), n);
    hipLaunchKernelGGL(ccl_init_kernel, px, dim3(256), 0, stream, jd);
    IRN_LAUNCH_CHECK("ccl_init_kernel");
    hipLaunchKernelGGL(forest_merge_kernel<CclJob>, px, dim3(256), 0, stream, jd);
    IRN_LAUNCH_CHECK("forest_merge_kernel<ccl>");
    hipLaunchKernelGGL(forest_flatten_kernel<CclJob>, px, dim3(256), 0, stream, jd);
    IRN_LAUNCH_CHECK("forest_flatten_kernel<ccl>");
    hipLaunchKernelGGL(ccl_rank_kernel, dim3(n), dim3(1024), 0, stream, jd);
    IRN_LAUNCH_CHECK("ccl_rank_kernel");
    hipLaunchKernelGGL(ccl_relabel_kernel, px, dim3(256), 0, stream, jd);
    IRN_LAUNCH_CHECK("ccl_relabel_kernel");
    return scratch_release(stream);
}

// scratch of one image in irn_cluster_centroids_batch:
//   [parent npx][rank npx] int32, [picked npx] int32, [present npx+2] int32, [one spare block]
//   (each 256-byte aligned)
static size_t cluster_scratch_bytes(int h, int w) {
    if (h < 1 || w < 1) return 0;
    const size_t npx = (size_t)h * w;
    return round_up(4 * npx, 256) * 3 + round_up(4 * (npx + 2), 256) + 256;
}

extern "C" size_t irn_cluster_batch_scratch_bytes(int n_images, const int32_t *h, const int32_t *w) {
    if (n_images < 1 || !h || !w) return 0;
    size_t total = 0;
    for (int i = 0; i < n_images; ++i) total += cluster_scratch_bytes(h[i], w[i]);
    return total;
}

extern "C" int irn_cluster_centroids_batch(int n_images, const int32_t *const *centroids_dev, const float *const *dp_dev,
                                           const int32_t *h, const int32_t *w, float thres,
                                           int32_t *const *cluster_map_dev, int32_t *k_dev, void *scratch_dev,
                                           void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n_images < 1 || !centroids_dev || !dp_dev || !h || !w || !cluster_map_dev || !k_dev || !scratch_dev)
        return fail(IRN_ERR_ARG, "irn_cluster_centroids_batch: bad argument");
    std::vector<ClusterJob> jobs(n_images);
    char *s = (char *)scratch_dev;
    int max_n = 0;
    for (int i = 0; i < n_images; ++i) {
        if (!centroids_dev[i] || !dp_dev[i] || !cluster_map_dev[i] || h[i] < 1 || w[i] < 1)
            return fail(IRN_ERR_ARG, "irn_cluster_centroids_batch: image %d: bad argument", i);
        if ((long)h[i] * w[i] > (1L << 30)) return fail(IRN_ERR_ARG, "irn_cluster_centroids_batch: image too large");
        const size_t npx = (size_t)h[i] * w[i];
        const size_t a = round_up(4 * npx, 256);
        ClusterJob &J = jobs[i];
        J.centroids = centroids_dev[i];
        J.dp = dp_dev[i];
        J.cluster_map = cluster_map_dev[i];
        J.parent = (int *)s;
        J.rank = (int *)(s + a);
        J.picked = (int32_t *)(s + 2 * a);
        J.present = (int *)(s + 3 * a);
        J.k_out = k_dev + i;
        J.h = h[i];
        J.w = w[i];
        s += cluster_scratch_bytes(h[i], w[i]);
        max_n = std::max(max_n, (int)npx);
    }
    ClusterJob *jd = nullptr;
    int rc = scratch_upload(jobs.data(), sizeof(ClusterJob) * n_images, (void **)&jd, stream);
    if (rc) return rc;
    const dim3 px(cdiv(max_n, 256), n_images);
    hipLaunchKernelGGL(cluster_init_kernel, px, dim3(256), 0, stream, jd, thres);
    IRN_LAUNCH_CHECK("cluster_init_kernel");
    hipLaunchKernelGGL(forest_merge_kernel<ClusterJob>, px, dim3(256), 0, stream, jd);
    IRN_LAUNCH_CHECK("forest_merge_kernel<cluster>");
    hipLaunchKernelGGL(forest_flatten_kernel<ClusterJob>, px, dim3(256), 0, stream, jd);
    IRN_LAUNCH_CHECK("forest_flatten_kernel<cluster>");
    hipLaunchKernelGGL(cluster_rank_kernel, dim3(n_images), dim3(1024), 0, stream, jd);
    IRN_LAUNCH_CHECK("cluster_rank_kernel");
    hipLaunchKernelGGL(cluster_pick_kernel, px, dim3(256), 0, stream, jd);
    IRN_LAUNCH_CHECK("cluster_pick_kernel");
    hipLaunchKernelGGL(cluster_compress_kernel, dim3(n_images), dim3(1024), 0, stream, jd);
    IRN_LAUNCH_CHECK("cluster_compress_kernel");
    hipLaunchKernelGGL(cluster_remap_kernel, px, dim3(256), 0, stream, jd);
    IRN_LAUNCH_CHECK("cluster_remap_kernel");
    return scratch_release(stream);
}

// scratch of one image in irn_detect_instance_*: [parent npx][prov npx][newid npx][area npx][score_bits npx] int32,
//                                                 [keys npx] int64, [counter]
static size_t detect_scratch_bytes(int n_channels, int h, int w) {
    if (n_channels < 1 || h < 1 || w < 1) return 0;
    const size_t npx = (size_t)h * w;
    return round_up(4 * npx, 256) * 5 + round_up(8 * npx, 256) + 256;
}

extern "C" size_t irn_detect_batch_scratch_bytes(int n_images, const int32_t *n_channels, const int32_t *h,
                                                 const int32_t *w) {
    if (n_images < 1 || !n_channels || !h || !w) return 0;
    size_t total = 0;
    for (int i = 0; i < n_images; ++i) total += detect_scratch_bytes(n_channels[i], h[i], w[i]);
    return total;
}

namespace {
// carve the per-image scratch; `counter` = the last 256-byte block unless the caller supplies one
void det_carve(DetJob &J, char *b, size_t npx) {
    const size_t a = round_up(4 * npx, 256);
    J.parent = (int *)b;
    J.prov = (int *)(b + a);
    J.newid = (int *)(b + 2 * a);
    J.area = (int *)(b + 3 * a);
    J.score_bits = (int *)(b + 4 * a);
    J.keys = (long long *)(b + 5 * a);
    J.counter = (int32_t *)(b + 5 * a + round_up(8 * npx, 256));
}

int det_fill_jobs(const char *who, int n_images, const float *const *rw_up_dev, const int32_t *const *argmax_dev,
                  const int32_t *n_channels, const int32_t *h, const int32_t *w, void *scratch_dev,
                  std::vector<DetJob> &jobs, int *max_n) {
    if (n_images < 1 || !rw_up_dev || !argmax_dev || !n_channels || !h || !w || !scratch_dev)
        return fail(IRN_ERR_ARG, "%s: bad argument", who);
    jobs.assign(n_images, DetJob{});
    char *s = (char *)scratch_dev;
    *max_n = 0;
    for (int i = 0; i < n_images; ++i) {
        if (!rw_up_dev[i] || !argmax_dev[i] || n_channels[i] < 1 || n_channels[i] > 65535 || h[i] < 1 || w[i] < 1)
            return fail(IRN_ERR_ARG, "%s: image %d: bad argument", who, i);
        if ((long)h[i] * w[i] > (1L << 30)) return fail(IRN_ERR_ARG, "%s: image too large", who);
        DetJob &J = jobs[i];
        J.rw_up = rw_up_dev[i];
        J.cls = argmax_dev[i];
        J.h = h[i];
        J.w = w[i];
        det_carve(J, s, (size_t)h[i] * w[i]);
        s += detect_scratch_bytes(n_channels[i], h[i], w[i]);
        *max_n = std::max(*max_n, h[i] * w[i]);
    }
    return IRN_OK;
}
}  // namespace

extern "C" int irn_detect_instance_batch_count(int n_images, const float *const *rw_up_dev,
                                               const int32_t *const *argmax_dev, const int32_t *n_channels,
                                               const int32_t *h, const int32_t *w, int32_t *n_det_dev,
                                               void *scratch_dev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    std::vector<DetJob> jobs;
    int max_n = 0;
    int rc = det_fill_jobs("irn_detect_instance_batch_count", n_images, rw_up_dev, argmax_dev, n_channels, h, w,
                           scratch_dev, jobs, &max_n);
    if (rc) return rc;
    if (!n_det_dev) return fail(IRN_ERR_ARG, "irn_detect_instance_batch_count: null n_det_dev");
    for (int i = 0; i < n_images; ++i) jobs[i].counter = n_det_dev + i;
    DetJob *jd = nullptr;
    rc = scratch_upload(jobs.data(), sizeof(DetJob) * n_images, (void **)&jd, stream);
    if (rc) return rc;
    IRN_HIP_TRY(hipMemsetAsync(n_det_dev, 0, sizeof(int32_t) * n_images, stream));
    const dim3 px(cdiv(max_n, 256), n_images);
    int max_tiles = 0, max_border = 0;
    for (int i = 0; i < n_images; ++i) {
        const int tx = cdiv(w[i], kDetTW), ty = cdiv(h[i], kDetTH);
        max_tiles = std::max(max_tiles, tx * ty);
        max_border = std::max(max_border, (ty - 1) * w[i] + (tx - 1) * h[i]);
    }
    hipLaunchKernelGGL(det_local_kernel, dim3(max_tiles, n_images), dim3(256), 0, stream, jd);
    IRN_LAUNCH_CHECK("det_local_kernel");
    if (max_border > 0) {
        hipLaunchKernelGGL(det_border_kernel, dim3(cdiv(max_border, 256), n_images), dim3(256), 0, stream, jd);
        IRN_LAUNCH_CHECK("det_border_kernel");
    }
    hipLaunchKernelGGL(forest_flatten_kernel<DetJob>, px, dim3(256), 0, stream, jd);
    IRN_LAUNCH_CHECK("forest_flatten_kernel<det>");
    hipLaunchKernelGGL(det_roots_kernel, px, dim3(256), 0, stream, jd);
    IRN_LAUNCH_CHECK("det_roots_kernel");
    return scratch_release(stream);
}

extern "C" int irn_detect_instance_batch_emit(int n_images, const float *const *rw_up_dev,
                                              const int32_t *const *argmax_dev, const int32_t *n_channels,
                                              const int32_t *h, const int32_t *w, const int32_t *n_det,
                                              const double *min_area, float *const *score_dev,
                                              int32_t *const *channel_dev, uint8_t *const *mask_dev, void *scratch_dev,
                                              void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    std::vector<DetJob> jobs;
    int max_n = 0;
    int rc = det_fill_jobs("irn_detect_instance_batch_emit", n_images, rw_up_dev, argmax_dev, n_channels, h, w,
                           scratch_dev, jobs, &max_n);
    if (rc) return rc;
    if (!n_det || !min_area || !score_dev || !channel_dev || !mask_dev)
        return fail(IRN_ERR_ARG, "irn_detect_instance_batch_emit: null argument");
    int max_det = 0;
    for (int i = 0; i < n_images; ++i) {
        DetJob &J = jobs[i];
        J.n_det = n_det[i];
        if (J.n_det < 0 || J.n_det > h[i] * w[i])
            return fail(IRN_ERR_ARG, "irn_detect_instance_batch_emit: image %d: n_det = %d", i, J.n_det);
        if (J.n_det == 0) continue;                       // nothing to write for this image
        if (!score_dev[i] || !channel_dev[i] || !mask_dev[i])
            return fail(IRN_ERR_ARG, "irn_detect_instance_batch_emit: image %d: null output", i);
        J.score = score_dev[i];
        J.channel = channel_dev[i];
        J.mask = mask_dev[i];
        J.min_area = min_area[i];
        max_det = std::max(max_det, J.n_det);
    }
    if (max_det == 0) return IRN_OK;
    DetJob *jd = nullptr;
    rc = scratch_upload(jobs.data(), sizeof(DetJob) * n_images, (void **)&jd, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(det_zero_masks_kernel, dim3(64, n_images), dim3(256), 0, stream, jd);
    IRN_LAUNCH_CHECK("det_zero_masks_kernel");
    hipLaunchKernelGGL(det_order_kernel, dim3(cdiv(max_det, 256), n_images), dim3(256), 0, stream, jd);
    IRN_LAUNCH_CHECK("det_order_kernel");
    hipLaunchKernelGGL(det_stats_kernel<false>, dim3(cdiv(max_n, 256), n_images), dim3(256), 0, stream, jd, (const RleJob *)nullptr);
    IRN_LAUNCH_CHECK("det_stats_kernel<dense>");
    hipLaunchKernelGGL(det_final_kernel, dim3(cdiv(max_det, 256), n_images), dim3(256), 0, stream, jd);
    IRN_LAUNCH_CHECK("det_final_kernel");
    return scratch_release(stream);
}

// ---------------------------------------------------------------------------------------------
// Detections as COCO run lengths, straight from the labelled map (step/make_ins_seg_labels.py:82-105 followed by the
// encoding of step/make_cocoann.py:38-46) — no dense mask plane anywhere.
//
// After irn_detect_instance_batch_count and det_order_kernel the detection of pixel p is newid[prov[parent[p]]]: ONE
// int32 map per image holds every mask.  In pycocotools' column-major order (j = x*h + y) a pixel whose id differs from
// its predecessor's is an EVENT: it ends a run of ones of the predecessor's detection and starts one of its own (the
// background, id -1, has no runs).  The events of one detection, ordered by j, alternate start / end, their positions are
// distinct, and with the map's end (j = h*w) appended as a last position the run lengths are the differences of
// neighbouring positions, the first taken from 0: the leading zero-run (0 when the detection owns pixel (0,0)), then ones
// and zeros in turn, and the last difference is the trailing zero-run or — when the detection owns the last pixel — the
// run of ones that reaches the end.  So n_runs = events + 1, always.
//
//   count:  det_order_kernel     final ids and channels (shared with the dense path)
//           rle_init_kernel      box and run counters of every detection
//           det_stats_kernel     <true>: the id map; area, maximum score and box per detection (integer atomics)
//           rle_events_kernel    <false>: events per detection (integer atomic adds)
//           rle_final_kernel     score, area, bbox, n_runs of every detection
//   emit:   rle_events_kernel    <true>: every event appends the key (batch-wide detection index << 32 | j) to its image's
//                                segment; every detection adds the key of the map's end
//           rocprim radix sort   ONE sort of the batch's keys: detections ascending, positions ascending inside each
//           rle_runs_kernel      counts[t] = position of key t - position of key t-1 (0 across a detection's start)
//
// Where a key lands before the sort depends on the order the atomics arrive in; the keys are distinct, so the sorted
// array does not, and everything else is an integer sum, minimum or maximum: the output is bit-reproducible and the
// same whatever batch an image is part of.  Nothing is sized per thread and per detection: a noisy map with tens of
// thousands of fragments costs two keys per fragment pixel run, like any other.
// ---------------------------------------------------------------------------------------------
namespace {

__global__ __launch_bounds__(256) void rle_init_kernel(const RleJob *__restrict__ jobs) {
    const RleJob R = jobs[blockIdx.y];
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= R.n_det) return;
    R.x0[d] = R.y0[d] = INT_MAX;
    R.x1[d] = R.y1[d] = -1;
    R.runs[d] = 1;                    // the map's end closes the last run
}

// one atomic add for the wave when all of its adders share a target (a component's upper edge), one each otherwise
__device__ __forceinline__ void add_one_per_lane(int *counter, bool on, int target) {
    const unsigned long long m = __ballot(on);
    if (m == 0) return;
    const int first = __ffsll((long long)m) - 1;
    const int t0 = __shfl(target, first);
    if (__all(!on || target == t0)) {
        if ((int)(threadIdx.x & 63) == first) atomicAdd(counter + t0, __popcll(m));
    } else if (on) {
        atomicAdd(counter + target, 1);
    }
}

// Pixel p = (y, x) follows (y-1, x) in column-major order, or the last pixel of column x-1; the first pixel follows the
// background.  Row-major threads: the map is read as whole rows, twice.
template <bool EMIT>
__global__ __launch_bounds__(256) void rle_events_kernel(const RleJob *__restrict__ jobs) {
    const RleJob R = jobs[blockIdx.y];
    if (R.n_det < 1) return;
    const int npx = R.h * R.w;
    const int p = blockIdx.x * 256 + threadIdx.x;
    int a = -1, b = -1, j = 0;
    if (p < npx) {
        const int y = p / R.w, x = p - y * R.w;
        b = R.idmap[p];
        a = y > 0 ? R.idmap[p - R.w] : (x > 0 ? R.idmap[(R.h - 1) * R.w + x - 1] : -1);
        j = x * R.h + y;
    }
    const bool ends = a != b && a >= 0, starts = a != b && b >= 0;
    if (!EMIT) {
        add_one_per_lane(R.runs, ends, a);
        add_one_per_lane(R.runs, starts, b);
        return;
    }
    if (p < R.n_det && p < R.room) R.keys[p] = ((unsigned long long)(R.g0 + p) << 32) | (unsigned)npx;   // the map's end
    const unsigned long long me = __ballot(ends), ms = __ballot(starts);
    const int total = __popcll(me) + __popcll(ms);
    if (total == 0) return;
    const int lane = threadIdx.x & 63;
    const unsigned long long below = lane ? ~0ull >> (64 - lane) : 0ull;
    unsigned base = 0;
    if (lane == 0) base = atomicAdd(R.cursor, (unsigned)total);
    base = (unsigned)__shfl((int)base, 0);
    long long slot = (long long)R.n_det + base + __popcll(me & below) + __popcll(ms & below);
    if (ends) {
        if (slot < R.room) R.keys[slot] = ((unsigned long long)(R.g0 + a) << 32) | (unsigned)j;
        ++slot;
    }
    if (starts && slot < R.room) R.keys[slot] = ((unsigned long long)(R.g0 + b) << 32) | (unsigned)j;
}

__global__ __launch_bounds__(256) void rle_final_kernel(const DetJob *__restrict__ jobs, const RleJob *__restrict__ rjobs) {
    const DetJob J = jobs[blockIdx.y];
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= J.n_det) return;
    const RleJob R = rjobs[blockIdx.y];
    const int area = J.area[d];
    J.score[d] = final_score(area, J.min_area, J.score_bits[d]);
    R.area_out[d] = area;
    R.n_runs_out[d] = R.runs[d];
    const int x0 = R.x0[d], y0 = R.y0[d];
    int32_t *b = R.bbox_out + 4 * (long)d;
    b[0] = x0, b[1] = y0, b[2] = R.x1[d] - x0 + 1, b[3] = R.y1[d] - y0 + 1;   // every detection has a pixel
}

__global__ __launch_bounds__(256) void rle_runs_kernel(const unsigned long long *__restrict__ keys, long long n,
                                                       uint32_t *__restrict__ counts) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const unsigned long long k = keys[t];
    unsigned prev = 0;
    if (t > 0) {
        const unsigned long long q = keys[t - 1];
        if ((q >> 32) == (k >> 32)) prev = (unsigned)q;
    }
    counts[t] = (unsigned)k - prev;
}

// scratch of the rle entries: [cursor int32 x n_images], then per image [idmap npx] and [x0 x1 y0 y1 runs] x n_det int32
// (each block 256-byte aligned)
size_t rle_image_bytes(int h, int w, int n_det) {
    return round_up(4 * (size_t)h * w, 256) + 5 * round_up(4 * (size_t)n_det, 256);
}

bool rle_shapes_ok(int n_images, const int32_t *h, const int32_t *w, const int32_t *n_det, long long *total_det) {
    if (n_images < 0 || (n_images > 0 && (!h || !w || !n_det))) return false;
    long long g = 0;
    for (int i = 0; i < n_images; ++i) {
        if (h[i] < 1 || w[i] < 1 || (long long)h[i] * w[i] > (1LL << 30)) return false;   // as irn_detect_instance_batch_count
        if (n_det[i] < 0 || n_det[i] > (long long)h[i] * w[i]) return false;
        g += n_det[i];
    }
    if (g > INT_MAX) return false;
    *total_det = g;
    return true;
}

void rle_carve(std::vector<RleJob> &jobs, void *scratch, int n_images, const int32_t *h, const int32_t *w,
               const int32_t *n_det) {
    jobs.assign(n_images, RleJob{});
    char *s = (char *)scratch + round_up(4 * (size_t)n_images, 256);
    int g = 0;
    for (int i = 0; i < n_images; ++i) {
        RleJob &R = jobs[i];
        const size_t a = round_up(4 * (size_t)n_det[i], 256);
        R.idmap = (int *)s;
        char *t = s + round_up(4 * (size_t)h[i] * w[i], 256);
        R.x0 = (int *)t, R.x1 = (int *)(t + a), R.y0 = (int *)(t + 2 * a), R.y1 = (int *)(t + 3 * a), R.runs = (int *)(t + 4 * a);
        R.cursor = (unsigned *)scratch + i;
        R.g0 = g;
        R.h = h[i], R.w = w[i], R.n_det = n_det[i];
        g += n_det[i];
        s += rle_image_bytes(h[i], w[i], n_det[i]);
    }
}

// the sort looks at the position's 32 bits and at as many bits above them as the batch's detection indices need
unsigned rle_key_bits(int total_det) {
    unsigned bits = 33;
    while (bits < 64 && ((long long)total_det - 1) >> (bits - 32)) ++bits;
    return bits;
}

}  // namespace

extern "C" size_t irn_detect_instance_batch_rle_scratch_bytes(int n_images, const int32_t *h, const int32_t *w,
                                                              const int32_t *n_det) {
    long long g = 0;
    if (!rle_shapes_ok(n_images, h, w, n_det, &g)) {
        fail(IRN_ERR_ARG, "irn_detect_instance_batch_rle_scratch_bytes: bad argument (n_images >= 0, 1 <= h*w <= 2^30, "
                          "0 <= n_det <= h*w, no null pointer)");
        return 0;
    }
    if (n_images == 0) return 0;
    size_t total = round_up(4 * (size_t)n_images, 256);
    for (int i = 0; i < n_images; ++i) total += rle_image_bytes(h[i], w[i], n_det[i]);
    return total;
}

extern "C" int irn_detect_instance_batch_rle_count(int n_images, const float *const *rw_up_dev,
                                                   const int32_t *const *argmax_dev, const int32_t *n_channels,
                                                   const int32_t *h, const int32_t *w, const int32_t *n_det,
                                                   const double *min_area, float *score_dev, int32_t *channel_dev,
                                                   int32_t *area_dev, int32_t *n_runs_dev, int32_t *bbox_dev,
                                                   void *scratch_dev, void *rle_scratch_dev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char *who = "irn_detect_instance_batch_rle_count";
    long long g = 0;
    if (!rle_shapes_ok(n_images, h, w, n_det, &g))
        return fail(IRN_ERR_ARG, "%s: bad argument (n_images >= 0, 1 <= h*w <= 2^30 < 2^31 - 1, 0 <= n_det <= h*w, no null pointer)", who);
    if (n_images == 0) return IRN_OK;
    if (!min_area || !rle_scratch_dev) return fail(IRN_ERR_ARG, "%s: null argument", who);
    std::vector<DetJob> jobs;
    int max_n = 0;
    int rc = det_fill_jobs(who, n_images, rw_up_dev, argmax_dev, n_channels, h, w, scratch_dev, jobs, &max_n);
    if (rc) return rc;
    if (g == 0) return IRN_OK;
    if (!score_dev || !channel_dev || !area_dev || !n_runs_dev || !bbox_dev) return fail(IRN_ERR_ARG, "%s: null output", who);
    std::vector<RleJob> rjobs;
    rle_carve(rjobs, rle_scratch_dev, n_images, h, w, n_det);
    int max_det = 0;
    for (int i = 0; i < n_images; ++i) {
        DetJob &J = jobs[i];
        RleJob &R = rjobs[i];
        J.n_det = n_det[i];
        J.min_area = min_area[i];
        J.score = score_dev + R.g0;
        J.channel = channel_dev + R.g0;
        R.area_out = area_dev + R.g0;
        R.n_runs_out = n_runs_dev + R.g0;
        R.bbox_out = bbox_dev + 4 * (size_t)R.g0;
        max_det = std::max(max_det, J.n_det);
    }
    // both job tables in ONE upload (a scratch slot is released once)
    const size_t det_bytes = round_up(sizeof(DetJob) * n_images, 16);
    std::vector<char> blob(det_bytes + sizeof(RleJob) * n_images);
    memcpy(blob.data(), jobs.data(), sizeof(DetJob) * n_images);
    memcpy(blob.data() + det_bytes, rjobs.data(), sizeof(RleJob) * n_images);
    char *bd = nullptr;
    rc = scratch_upload(blob.data(), blob.size(), (void **)&bd, stream);
    if (rc) return rc;
    const DetJob *jd = (const DetJob *)bd;
    const RleJob *rd = (const RleJob *)(bd + det_bytes);
    const dim3 per_det(cdiv(max_det, 256), n_images), per_px(cdiv(max_n, 256), n_images);
    hipLaunchKernelGGL(det_order_kernel, per_det, dim3(256), 0, stream, jd);
    IRN_LAUNCH_CHECK("det_order_kernel");
    hipLaunchKernelGGL(rle_init_kernel, per_det, dim3(256), 0, stream, rd);
    IRN_LAUNCH_CHECK("rle_init_kernel");
    hipLaunchKernelGGL(det_stats_kernel<true>, per_px, dim3(256), 0, stream, jd, rd);
    IRN_LAUNCH_CHECK("det_stats_kernel<rle>");
    hipLaunchKernelGGL(rle_events_kernel<false>, per_px, dim3(256), 0, stream, rd);
    IRN_LAUNCH_CHECK("rle_events_kernel<count>");
    hipLaunchKernelGGL(rle_final_kernel, per_det, dim3(256), 0, stream, jd, rd);
    IRN_LAUNCH_CHECK("rle_final_kernel");
    return scratch_release(stream);
}

extern "C" size_t irn_detect_instance_batch_rle_sort_bytes(int64_t total_runs, int total_det) {
    if (total_runs < 0 || total_runs >= (long long)UINT_MAX || total_det < 0 || total_det > total_runs) {
        fail(IRN_ERR_ARG, "irn_detect_instance_batch_rle_sort_bytes: bad argument (0 <= total_det <= total_runs < 2^32 - 1)");
        return 0;
    }
    if (total_runs == 0) return 0;
    size_t tmp = 0;
    (void)rocprim::radix_sort_keys(nullptr, tmp, (unsigned long long *)nullptr, (unsigned long long *)nullptr,
                                   (unsigned)total_runs, 0u, rle_key_bits(total_det), (hipStream_t)0);
    return 2 * round_up(8 * (size_t)total_runs, 256) + round_up(tmp, 256);
}

extern "C" int irn_detect_instance_batch_rle_emit(int n_images, const int32_t *h, const int32_t *w, const int32_t *n_det,
                                                  const int64_t *runs, uint32_t *counts_dev, void *rle_scratch_dev,
                                                  void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char *who = "irn_detect_instance_batch_rle_emit";
    long long g = 0;
    if (!rle_shapes_ok(n_images, h, w, n_det, &g))
        return fail(IRN_ERR_ARG, "%s: bad argument (n_images >= 0, 1 <= h*w <= 2^30 < 2^31 - 1, 0 <= n_det <= h*w, no null pointer)", who);
    if (n_images == 0) return IRN_OK;
    if (!runs) return fail(IRN_ERR_ARG, "%s: null runs", who);
    long long total = 0;
    int max_n = 0;
    for (int i = 0; i < n_images; ++i) {
        // every detection has at least its first event and the map's end; a map of npx pixels has at most 2*npx events
        if (runs[i] < 2LL * n_det[i] || runs[i] > 2LL * h[i] * w[i] + n_det[i])
            return fail(IRN_ERR_ARG, "%s: image %d: %lld runs for %d detections", who, i, (long long)runs[i], n_det[i]);
        total += runs[i];
        if (n_det[i] > 0) max_n = std::max(max_n, h[i] * w[i]);
    }
    if (total >= (long long)UINT_MAX) return fail(IRN_ERR_ARG, "%s: %lld runs in one batch", who, total);
    if (total == 0) return IRN_OK;
    if (!counts_dev || !rle_scratch_dev || !ws) return fail(IRN_ERR_ARG, "%s: null argument", who);
    const size_t need = irn_detect_instance_batch_rle_sort_bytes(total, (int)g);
    if (ws_bytes < need) return fail(IRN_ERR_ARG, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, need);
    const size_t kb = round_up(8 * (size_t)total, 256);
    unsigned long long *keys_in = (unsigned long long *)ws, *keys_out = (unsigned long long *)((char *)ws + kb);
    void *tmp = (char *)ws + 2 * kb;
    size_t tmp_bytes = need - 2 * kb;
    std::vector<RleJob> rjobs;
    rle_carve(rjobs, rle_scratch_dev, n_images, h, w, n_det);
    long long at = 0;
    for (int i = 0; i < n_images; ++i) {
        rjobs[i].keys = keys_in + at;
        rjobs[i].room = (int)std::min<long long>(runs[i], INT_MAX);
        at += runs[i];
    }
    RleJob *rd = nullptr;
    int rc = scratch_upload(rjobs.data(), sizeof(RleJob) * n_images, (void **)&rd, stream);
    if (rc) return rc;
    IRN_HIP_TRY(hipMemsetAsync(rle_scratch_dev, 0, sizeof(int) * n_images, stream));       // the cursors
    hipLaunchKernelGGL(rle_events_kernel<true>, dim3(cdiv(max_n, 256), n_images), dim3(256), 0, stream, rd);
    IRN_LAUNCH_CHECK("rle_events_kernel<emit>");
    IRN_HIP_TRY(rocprim::radix_sort_keys(tmp, tmp_bytes, keys_in, keys_out, (unsigned)total, 0u, rle_key_bits((int)g), stream));
    hipLaunchKernelGGL(rle_runs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, keys_out, total, counts_dev);
    IRN_LAUNCH_CHECK("rle_runs_kernel");
    return scratch_release(stream);
}

// ---------------------------------------------------------------------------------------------
// Overlap counts against the ground truth, straight from the labelled map (what irn_detect_instance_batch_emit followed by
// irn_mask_overlap count, eval.hip) — no dense mask plane anywhere.
//
// Pixel p lies in detection d = newid[prov[parent[p]]] (none: background) and in GT instance id = inst[p] (0: none; an id
// above g is counted in `bad` over the whole image and then reads as none, as k_mask_overlap's whole-image row does).  The
// pixel counts by (d + 1, id) form a table of (n_det + 1) x (g + 1) cells whose interior is `inter`, whose column sums are
// the GT areas (row 0, the background, included: an image without detections still has them) and whose row sums are the
// detections' areas (column 0 included).  Only the interior and the two margins are kept in memory: a cell's count goes to
// inter[d][id - 1], area_gt[id - 1] and the detection's int32 area of det_stats_kernel, by integer atomics.
//
// A workgroup counts 4096 consecutive pixels.  When the image's table has at most kOvlCells = 4096 cells the workgroup
// counts into a copy of it in LDS (uint32: a cell cannot exceed 4096) and flushes its non-zero cells once; a larger table
// (a noisy map with thousands of fragments) is counted with global atomics directly.  The budget: 16 KiB of LDS per
// workgroup lets ten workgroups share a CU's 160 KiB, more than the eight that its 32 wave slots hold, so the table
// never lowers the occupancy; and the flush scans at most 16 cells per thread, no more than the 16 pixels the thread has
// just counted.  A real image has tens of detections and a few GT instances: a few hundred cells.
// Either way a wave first looks whether its 64 consecutive pixels share ONE (detection, GT id) pair — nearly always —
// and then adds once for all of them; the maximum score is aggregated per detection as det_stats_kernel does.
// ---------------------------------------------------------------------------------------------
namespace {

constexpr int kOvlPPT = 16, kOvlPix = 256 * kOvlPPT, kOvlCells = 4096;

struct OvlJob {
    const uint8_t *inst;        // [h,w] GT instance of every pixel
    long long *inter;           // [n_det][g]
    long long *area_gt;         // [g]
    long long *area_pred;       // [n_det]
    int g;
    int in_lds;                 // the image's table fits kOvlCells
};

__device__ __forceinline__ void ovl_add64(long long *p, unsigned v) {
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
}

// v pixels of cell (r, c): r = detection + 1 (0 = background), c = GT id (0 = none)
__device__ __forceinline__ void ovl_cell(const DetJob &J, const OvlJob &O, int r, int c, unsigned v) {
    if (r > 0) atomicAdd(J.area + (r - 1), (int)v);
    if (c > 0) ovl_add64(O.area_gt + (c - 1), v);
    if (r > 0 && c > 0) ovl_add64(O.inter + (size_t)(r - 1) * O.g + (c - 1), v);
}

__global__ __launch_bounds__(256) void det_overlap_kernel(const DetJob *__restrict__ jobs, const OvlJob *__restrict__ ojobs,
                                                          long long *__restrict__ bad) {
    __shared__ unsigned tab[kOvlCells];
    __shared__ unsigned nbad;
    const DetJob J = jobs[blockIdx.y];
    const int npx = J.h * J.w;
    const int base = blockIdx.x * kOvlPix;
    if (base >= npx) return;
    const OvlJob O = ojobs[blockIdx.y];
    const int tid = threadIdx.x, lane = tid & 63;
    const int cols = O.g + 1, cells = O.in_lds ? (J.n_det + 1) * cols : 0;
    for (int i = tid; i < cells; i += 256) tab[i] = 0;
    if (tid == 0) nbad = 0;
    __syncthreads();
    unsigned my_bad = 0;
    for (int i = 0; i < kOvlPPT; ++i) {
        const int p = base + i * 256 + tid;           // a wave's 64 pixels are consecutive
        const bool in = p < npx;
        int d = -1, bits = 0, id = 0;
        if (in) {
            id = O.inst[p];
            if (id > O.g) {
                ++my_bad;
                id = 0;
            }
            const int c = J.cls[p];
            if (c > 0 && J.n_det > 0) {
                d = J.newid[J.prov[J.parent[p]]];
                if ((unsigned)d >= (unsigned)J.n_det) d = -1;          // a count that is not this map's: write nowhere
                const float sc = J.rw_up[(long)(c - 1) * npx + p];
                bits = sc > 0.f ? __float_as_int(sc) : 0;
            }
        }
        const bool fg = d >= 0;
        const unsigned long long act = __ballot(fg);
        if (act != 0) {
            const int d0 = __shfl(d, __ffsll((long long)act) - 1);
            if (__all(!fg || d == d0)) {
                int mx = bits;
                for (int sft = 32; sft > 0; sft >>= 1) mx = max(mx, __shfl_xor(mx, sft));
                if (lane == 0 && mx > 0) atomicMax(J.score_bits + d0, mx);
            } else if (fg && bits > 0) {
                atomicMax(J.score_bits + d, bits);
            }
        }
        const bool on = fg || id > 0;                 // cell (0, 0) is nobody's
        const unsigned long long m = __ballot(on);
        if (m == 0) continue;                         // (the whole wave)
        const int first = __ffsll((long long)m) - 1;
        const int d1 = __shfl(d, first), id1 = __shfl(id, first);
        const bool one = __all(!on || (d == d1 && id == id1));
        if (one ? lane == first : on) {
            const int r = d + 1;
            const unsigned v = one ? (unsigned)__popcll(m) : 1u;
            if (O.in_lds) atomicAdd(&tab[r * cols + id], v);
            else ovl_cell(J, O, r, id, v);
        }
    }
    if (my_bad) atomicAdd(&nbad, my_bad);
    __syncthreads();
    for (int i = tid; i < cells; i += 256) {
        const unsigned v = tab[i];
        if (v) ovl_cell(J, O, i / cols, i % cols, v);
    }
    if (tid == 0 && nbad) ovl_add64(bad, nbad);
}

__global__ __launch_bounds__(256) void det_overlap_final_kernel(const DetJob *__restrict__ jobs, const OvlJob *__restrict__ ojobs) {
    const DetJob J = jobs[blockIdx.y];
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= J.n_det) return;
    const int area = J.area[d];
    J.score[d] = final_score(area, J.min_area, J.score_bits[d]);
    ojobs[blockIdx.y].area_pred[d] = area;
}

struct RethresJob {
    const float *rw_up;         // [n_channels,h,w]
    const int32_t *argmax;      // [h,w]
    int32_t *out;               // [h,w]
    int n_channels, npx;
};

// The label epilogue's selection (label.hip, label_argmax_kernel) starts from the background plane and keeps the first NaN
// channel, else the first channel that reaches the maximum m when m > bg: which channel that is does not depend on bg, and
// the scores it compares are the ones it stores in rw_up.  So the map at a threshold T >= the map's own keeps a pixel's
// channel where that channel's stored score is NaN or > T, and reads 0 elsewhere.
__global__ __launch_bounds__(256) void argmax_rethreshold_kernel(const RethresJob *__restrict__ jobs, float thres) {
    const RethresJob J = jobs[blockIdx.y];
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= J.npx) return;
    int a = J.argmax[p];
    if (a > 0 && a <= J.n_channels) {
        const float s = J.rw_up[(long)(a - 1) * J.npx + p];
        if (!(s != s || s > thres)) a = 0;
    }
    J.out[p] = a;
}

}  // namespace

extern "C" int irn_detect_instance_batch_overlap(int n_images, const float *const *rw_up_dev, const int32_t *const *argmax_dev,
                                                 const int32_t *n_channels, const int32_t *h, const int32_t *w,
                                                 const int32_t *n_det, const double *min_area, const uint8_t *const *inst_dev,
                                                 const int32_t *g, float *score_dev, int32_t *channel_dev,
                                                 int64_t *area_pred_dev, int64_t *inter_dev, int64_t *area_gt_dev,
                                                 int64_t *bad_dev, void *scratch_dev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char *who = "irn_detect_instance_batch_overlap";
    long long G = 0;
    if (!rle_shapes_ok(n_images, h, w, n_det, &G))
        return fail(IRN_ERR_ARG, "%s: bad argument (n_images >= 0, 1 <= h*w <= 2^30, 0 <= n_det <= h*w, no null pointer)", who);
    if (n_images == 0) return IRN_OK;
    if (!min_area || !inst_dev || !g || !bad_dev) return fail(IRN_ERR_ARG, "%s: null argument", who);
    std::vector<DetJob> jobs;
    int max_n = 0;
    int rc = det_fill_jobs(who, n_images, rw_up_dev, argmax_dev, n_channels, h, w, scratch_dev, jobs, &max_n);
    if (rc) return rc;
    size_t n_gt = 0, n_inter = 0;
    for (int i = 0; i < n_images; ++i) {
        if (!inst_dev[i]) return fail(IRN_ERR_ARG, "%s: image %d: null instance map", who, i);
        if (g[i] < 0 || g[i] > 255) return fail(IRN_ERR_ARG, "%s: image %d: %d GT instances (0..255)", who, i, g[i]);
        n_gt += (size_t)g[i];
        n_inter += (size_t)n_det[i] * (size_t)g[i];
    }
    if ((G > 0 && (!score_dev || !channel_dev || !area_pred_dev)) || (n_gt > 0 && !area_gt_dev) || (n_inter > 0 && !inter_dev))
        return fail(IRN_ERR_ARG, "%s: null output", who);
    std::vector<OvlJob> ojobs(n_images);
    size_t at_det = 0, at_gt = 0, at_inter = 0;
    int max_det = 0;
    for (int i = 0; i < n_images; ++i) {
        DetJob &J = jobs[i];
        OvlJob &O = ojobs[i];
        J.n_det = n_det[i];
        J.min_area = min_area[i];
        J.score = score_dev + at_det;
        J.channel = channel_dev + at_det;
        O.inst = inst_dev[i];
        O.area_pred = (long long *)area_pred_dev + at_det;
        O.area_gt = (long long *)area_gt_dev + at_gt;
        O.inter = (long long *)inter_dev + at_inter;
        O.g = g[i];
        O.in_lds = ((long long)n_det[i] + 1) * (g[i] + 1) <= kOvlCells;
        at_det += (size_t)n_det[i];
        at_gt += (size_t)g[i];
        at_inter += (size_t)n_det[i] * (size_t)g[i];
        max_det = std::max(max_det, J.n_det);
    }
    // both job tables in ONE upload (a scratch slot is released once)
    const size_t det_bytes = round_up(sizeof(DetJob) * n_images, 16);
    std::vector<char> blob(det_bytes + sizeof(OvlJob) * n_images);
    memcpy(blob.data(), jobs.data(), sizeof(DetJob) * n_images);
    memcpy(blob.data() + det_bytes, ojobs.data(), sizeof(OvlJob) * n_images);
    char *bd = nullptr;
    rc = scratch_upload(blob.data(), blob.size(), (void **)&bd, stream);
    if (rc) return rc;
    const DetJob *jd = (const DetJob *)bd;
    const OvlJob *od = (const OvlJob *)(bd + det_bytes);
    if (n_gt) IRN_HIP_TRY(hipMemsetAsync(area_gt_dev, 0, sizeof(int64_t) * n_gt, stream));
    if (n_inter) IRN_HIP_TRY(hipMemsetAsync(inter_dev, 0, sizeof(int64_t) * n_inter, stream));
    const dim3 per_det(cdiv(max_det, 256), n_images);
    if (max_det > 0) {
        hipLaunchKernelGGL(det_order_kernel, per_det, dim3(256), 0, stream, jd);
        IRN_LAUNCH_CHECK("det_order_kernel");
    }
    hipLaunchKernelGGL(det_overlap_kernel, dim3(cdiv(max_n, kOvlPix), n_images), dim3(256), 0, stream, jd, od, (long long *)bad_dev);
    IRN_LAUNCH_CHECK("det_overlap_kernel");
    if (max_det > 0) {
        hipLaunchKernelGGL(det_overlap_final_kernel, per_det, dim3(256), 0, stream, jd, od);
        IRN_LAUNCH_CHECK("det_overlap_final_kernel");
    }
    return scratch_release(stream);
}

extern "C" int irn_argmax_rethreshold_batch(int n_images, const float *const *rw_up_dev, const int32_t *const *argmax_dev,
                                            const int32_t *n_channels, const int32_t *h, const int32_t *w, float thres,
                                            int32_t *const *out_dev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const char *who = "irn_argmax_rethreshold_batch";
    if (n_images < 0 || (n_images > 0 && (!rw_up_dev || !argmax_dev || !n_channels || !h || !w || !out_dev)) || thres != thres)
        return fail(IRN_ERR_ARG, "%s: bad argument (n_images >= 0, no null pointer, a threshold that is not NaN)", who);
    if (n_images == 0) return IRN_OK;
    if (n_images > 65535) return fail(IRN_ERR_ARG, "%s: at most 65535 images per call", who);   // grid.y = image
    std::vector<RethresJob> jobs(n_images);
    int max_n = 0;
    for (int i = 0; i < n_images; ++i) {
        if (!rw_up_dev[i] || !argmax_dev[i] || !out_dev[i] || n_channels[i] < 1 || h[i] < 1 || w[i] < 1)
            return fail(IRN_ERR_ARG, "%s: image %d: bad argument", who, i);
        if ((long)h[i] * w[i] > (1L << 30)) return fail(IRN_ERR_ARG, "%s: image too large", who);
        jobs[i] = RethresJob{rw_up_dev[i], argmax_dev[i], out_dev[i], n_channels[i], h[i] * w[i]};
        max_n = std::max(max_n, h[i] * w[i]);
    }
    RethresJob *jd = nullptr;
    int rc = scratch_upload(jobs.data(), sizeof(RethresJob) * n_images, (void **)&jd, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(argmax_rethreshold_kernel, dim3(cdiv(max_n, 256), n_images), dim3(256), 0, stream, jd, thres);
    IRN_LAUNCH_CHECK("argmax_rethreshold_kernel");
    return scratch_release(stream);
}
