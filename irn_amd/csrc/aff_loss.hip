// Fused affinity / displacement loss of IRNet training (gfx950).
//
// Replaces, for the training step, the chain reference net/resnet50_irn.py:198-213 + step/train_irn.py:58-64 +
// voc12/dataloader.py:80-106: `aff`, two log losses, `pair_disp`, two displacement losses and three label tensors,
// each [B, |S|, N] (255 MB at radius 10, 128x128, batch 32), only to be multiplied and summed to five numbers.  Here one
// workgroup owns a tile of source cells, stages the edge, label and displacement tiles with their radial halo in LDS
// once, and every thread walks the directions of its source cell: path maximum (LDS-issue bound, as in affinity.hip),
// then classification of the pair from the two label bytes and the loss terms on top of it, in registers.  Nothing of
// size [B, |S|, N] is ever written: the forward leaves five sums and three counts, the backward recomputes everything
// from the three maps and leaves the gradients of the two maps.
//
// Forward sums: per-element arithmetic in fp32 (as torch does it), accumulation in fp64, per-workgroup partials in the
// workspace, a second kernel adds them in a fixed order — no floating-point atomics, two calls give identical bits.
// Backward: gradients of a workgroup meet in LDS tiles (ds_add_f32) and are flushed with one global float atomic per
// touched cell, like affinity_backward_kernel: the order of those additions is not fixed, so the gradients are
// reproducible to rounding only, not bit for bit.
// Ordered backward (irn_aff_loss_backward_ordered): the same gradients as a gather.  One workgroup owns a tile of OUTPUT
// cells, stages the maps with a halo of radius - 1 on all four sides, and every thread adds what reaches its own cell in
// the path table's order in a register: no atomic, one plain store per cell, identical bits for identical inputs.
#include "path_unroll.hpp"

namespace irn {

namespace {

// ignore_from, a launch argument of the three kernels: labels >= ignore_from take no part (voc12/dataloader.py:94 has 21,
// the 20 VOC classes; a dataset of C classes passes C + 1).  Labels are bytes and 255 is always void: 1 <= ignore_from <= 255.
constexpr int kPartWords = 8;        // per workgroup: 5 fp64 sums, 3 int64 counts

struct PairAcc {
    // the source label is fixed per thread, so bg / fg is decided once at the end: positives and negatives are kept apart
    double pos = 0.0, neg = 0.0, disp = 0.0;
    int n_pos = 0, n_neg = 0;
};

struct Tiles {
    const float *edge, *dp0, *dp1;
    const unsigned char *lab;
};

// LDS layout for a tile with `cells` cells: edge, dp0, dp1 (fp32), [3 gradient tiles (fp32),] labels (bytes)
__host__ __device__ constexpr size_t lds_bytes(int cells, bool backward) {
    return (size_t)cells * 4 * (backward ? 6 : 3) + (size_t)((cells + 3) & ~3);
}

// Stage rows [ty0, ty0+LH), cols [tx0, tx0+LW) of the grid (tile column lx is grid column tx0 + lx: the source rectangle
// starts rf = halo columns in).  Cells outside the grid carry label 255, so no pair ever counts them.
__device__ __forceinline__ void stage(const float *__restrict__ edge, const float *__restrict__ dp,
                                      const unsigned char *__restrict__ label, int hp, int wp, int ty0, int tx0, int LH,
                                      int LW, float *t_edge, float *t_dp0, float *t_dp1, unsigned char *t_lab) {
    const long plane = (long)hp * wp;
    for (int i = threadIdx.x; i < LH * LW; i += 256) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gy = ty0 + ly, gx = tx0 + lx;
        float e = 1.0f, d0 = 0.f, d1 = 0.f;
        unsigned char l = 255;
        if (gy < hp && gx < wp) {
            const long g = (long)gy * wp + gx;
            e = edge[g];
            d0 = dp[g];
            d1 = dp[plane + g];
            l = label[g];
        }
        t_edge[i] = e;
        t_dp0[i] = d0;
        t_dp1[i] = d1;
        t_lab[i] = l;
    }
}

// Terms of the pair (source, source + (dy, dx)) whose path maximum is m.  a: the source label (255 for a thread outside the
// source rectangle), s0 / s1: displacement at the source, `o`: tile offset of the destination relative to the source.
__device__ __forceinline__ void pair_terms(PairAcc &acc, const Tiles &T, int src, int o, float m, int a, float s0, float s1,
                                           float dy, float dx, int ignore_from) {
    const int b = T.lab[src + o];
    const bool valid = a < ignore_from && b < ignore_from;
    const bool pos = valid && a == b, neg = valid && a != b;
    const float aff = 1.0f - m;
    // -log(aff + 1e-5) for an equal pair, -log(1 + 1e-5 - aff) for an unequal one: one logarithm per pair
    const float l = -logf(neg ? 1.00001f - aff : aff + 1e-5f);
    const float p0 = s0 - T.dp0[src + o], p1 = s1 - T.dp1[src + o];
    const float t0 = a > 0 ? fabsf(p0 - dy) : fabsf(p0), t1 = a > 0 ? fabsf(p1 - dx) : fabsf(p1);
    acc.pos += pos ? (double)l : 0.0;
    acc.neg += neg ? (double)l : 0.0;
    acc.disp += pos ? (double)t0 + (double)t1 : 0.0;
    acc.n_pos += pos;
    acc.n_neg += neg;
}

// R > 0: the directions and their paths are compile-time constants (radius 5 and 10, as affinity_wide_kernel);
// R == 0: the table-driven loop of affinity_kernel for any radius.
template <int R>
__global__ __launch_bounds__(256) void aff_loss_forward_kernel(const float *__restrict__ edge, const float *__restrict__ dp,
                                                               const unsigned char *__restrict__ label, int hp, int wp,
                                                               int radius, int n_dirs, const int *__restrict__ dir_start8,
                                                               const int *__restrict__ cell_off8,
                                                               const int *__restrict__ dir_dy, const int *__restrict__ dir_dx,
                                                               int ignore_from, double *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int halo = (R ? R : radius) - 1;
    const int LW = AFF_TW + 2 * halo, LH = AFF_TH + halo, cells = LH * LW;
    float *t_edge = lds, *t_dp0 = lds + cells, *t_dp1 = lds + 2 * cells;
    unsigned char *t_lab = reinterpret_cast<unsigned char *>(lds + 3 * cells);
    const int sh = hp - halo, sw = wp - 2 * halo;
    const int tiles_x = (sw + AFF_TW - 1) / AFF_TW;
    const int ty0 = ((int)blockIdx.x / tiles_x) * AFF_TH, tx0 = ((int)blockIdx.x % tiles_x) * AFF_TW;
    const long img = (long)blockIdx.y * hp * wp;
    stage(edge + img, dp + 2 * img, label + img, hp, wp, ty0, tx0, LH, LW, t_edge, t_dp0, t_dp1, t_lab);
    __syncthreads();

    const int ly = threadIdx.x / AFF_TW, lx = threadIdx.x % AFF_TW;
    const bool inside = ty0 + ly < sh && tx0 + lx < sw;
    const int src = ly * LW + lx + halo;
    const Tiles T{t_edge, t_dp0, t_dp1, t_lab};
    const int a = inside ? (int)t_lab[src] : 255;
    const float s0 = t_dp0[src], s1 = t_dp1[src];
    PairAcc acc;
    if constexpr (R > 0) {
        const float *tb = t_edge + ly * LW + lx;
        static_for<kPaths<R>.n_dirs>([&](auto id) __attribute__((always_inline)) {
            constexpr int d = decltype(id)::value;
            constexpr int dy = kPaths<R>.dy[d], dx = kPaths<R>.dx[d];
            pair_terms(acc, T, src, dy * LW + dx, path_max<R, d>(tb), a, s0, s1, (float)dy, (float)dx, ignore_from);
        });
    } else {
        const float *tb = t_edge + src;
        for (int d = 0; d < n_dirs; ++d) {
            const int k0 = dir_start8[d], k1 = dir_start8[d + 1];
            float m0 = -INFINITY, m1 = -INFINITY;
            for (int k = k0; k < k1; k += 8) {          // eight wave-uniform cell offsets per scalar load (affinity_kernel)
                const int4 oa = *reinterpret_cast<const int4 *>(cell_off8 + k);
                const int4 ob = *reinterpret_cast<const int4 *>(cell_off8 + k + 4);
                m0 = max3(max3(m0, tb[oa.x], tb[oa.y]), tb[oa.z], tb[oa.w]);
                m1 = max3(max3(m1, tb[ob.x], tb[ob.y]), tb[ob.z], tb[ob.w]);
            }
            const int dy = dir_dy[d], dx = dir_dx[d];
            pair_terms(acc, T, src, dy * LW + dx, max3(m0, m1, m1), a, s0, s1, (float)dy, (float)dx, ignore_from);
        }
    }

    // workgroup partial, in a fixed order: lanes by shuffle, then the four waves one after the other
    const bool bg = a == 0;
    double v[5] = {bg ? acc.pos : 0.0, bg ? 0.0 : acc.pos, acc.neg, bg ? 0.0 : acc.disp, bg ? acc.disp : 0.0};
    long long c[3] = {bg ? acc.n_pos : 0, bg ? 0 : acc.n_pos, acc.n_neg};
    for (int s = 32; s; s >>= 1) {
        for (int i = 0; i < 5; ++i) v[i] += __shfl_down(v[i], s, 64);
        for (int i = 0; i < 3; ++i) c[i] += __shfl_down(c[i], s, 64);
    }
    __shared__ double wave_part[4][kPartWords];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int i = 0; i < 5; ++i) wave_part[wave][i] = v[i];
        for (int i = 0; i < 3; ++i) wave_part[wave][5 + i] = __longlong_as_double(c[i]);
    }
    __syncthreads();
    if (threadIdx.x < kPartWords) {
        const int i = threadIdx.x;
        double *out = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kPartWords;
        if (i < 5) {
            out[i] = ((wave_part[0][i] + wave_part[1][i]) + wave_part[2][i]) + wave_part[3][i];
        } else {
            long long n = 0;
            for (int w = 0; w < 4; ++w) n += __double_as_longlong(wave_part[w][i]);
            out[i] = __longlong_as_double(n);
        }
    }
}

// One workgroup: thread t adds partials t, t+256, ... in ascending order, then a fixed tree over the 256 threads.
__global__ __launch_bounds__(256) void aff_loss_finish_kernel(const double *__restrict__ part, int n_parts,
                                                              double *__restrict__ sums, long long *__restrict__ counts) {
    __shared__ double red[256][kPartWords];
    double v[5] = {0, 0, 0, 0, 0};
    long long c[3] = {0, 0, 0};
    for (int p = threadIdx.x; p < n_parts; p += 256) {
        const double *q = part + (size_t)p * kPartWords;
        for (int i = 0; i < 5; ++i) v[i] += q[i];
        for (int i = 0; i < 3; ++i) c[i] += __double_as_longlong(q[5 + i]);
    }
    for (int i = 0; i < 5; ++i) red[threadIdx.x][i] = v[i];
    for (int i = 0; i < 3; ++i) red[threadIdx.x][5 + i] = __longlong_as_double(c[i]);
    __syncthreads();
    for (int s = 128; s; s >>= 1) {
        if ((int)threadIdx.x < s) {
            for (int i = 0; i < 5; ++i) red[threadIdx.x][i] += red[threadIdx.x + s][i];
            for (int i = 5; i < 8; ++i)
                red[threadIdx.x][i] = __longlong_as_double(__double_as_longlong(red[threadIdx.x][i]) +
                                                           __double_as_longlong(red[threadIdx.x + s][i]));
        }
        __syncthreads();
    }
    if (threadIdx.x < 5) sums[threadIdx.x] = red[0][threadIdx.x];
    else if (threadIdx.x < 8) counts[threadIdx.x - 5] = __double_as_longlong(red[0][threadIdx.x]);
}

__device__ __forceinline__ float sgn(float v) { return (float)((v > 0.f) - (v < 0.f)); }

// Backward.  Table-driven for every radius, over the path cells in the reference's order: the gradient of a path maximum
// goes to the FIRST cell that attains it (max_pool2d's rule, the same as affinity_backward_kernel), and that order is the
// path table's, not the raster order of the compile-time tables.
// IGN: the ignore threshold as a constant (the instantiation for 21, the default of every caller without a class list: with the
// threshold in a register this kernel measured 3 % slower), or 0 = the launch argument.
template <int IGN>
__global__ __launch_bounds__(256) void aff_loss_backward_kernel(const float *__restrict__ edge, const float *__restrict__ dp,
                                                                const unsigned char *__restrict__ label, int hp, int wp,
                                                                int radius, int n_dirs, const int *__restrict__ dir_start,
                                                                const int *__restrict__ cell_dy, const int *__restrict__ cell_dx,
                                                                const int *__restrict__ dir_dy, const int *__restrict__ dir_dx,
                                                                const float *__restrict__ coef, int ignore_arg,
                                                                float *__restrict__ grad_edge, float *__restrict__ grad_dp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int ignore_from = IGN ? IGN : ignore_arg;
    const int halo = radius - 1;
    const int LW = AFF_TW + 2 * halo, LH = AFF_TH + halo, cells = LH * LW;
    float *t_edge = lds, *t_dp0 = lds + cells, *t_dp1 = lds + 2 * cells;
    float *g_edge = lds + 3 * cells, *g_dp0 = lds + 4 * cells, *g_dp1 = lds + 5 * cells;
    unsigned char *t_lab = reinterpret_cast<unsigned char *>(lds + 6 * cells);
    const int sh = hp - halo, sw = wp - 2 * halo;
    const int tiles_x = (sw + AFF_TW - 1) / AFF_TW;
    const int ty0 = ((int)blockIdx.x / tiles_x) * AFF_TH, tx0 = ((int)blockIdx.x % tiles_x) * AFF_TW;
    const long img = (long)blockIdx.y * hp * wp;
    stage(edge + img, dp + 2 * img, label + img, hp, wp, ty0, tx0, LH, LW, t_edge, t_dp0, t_dp1, t_lab);
    for (int i = threadIdx.x; i < 3 * cells; i += 256) g_edge[i] = 0.f;
    __syncthreads();

    const int ly = threadIdx.x / AFF_TW, lx = threadIdx.x % AFF_TW;
    const bool inside = ty0 + ly < sh && tx0 + lx < sw;
    const int src = ly * LW + lx + halo;
    const int a = inside ? (int)t_lab[src] : 255;
    if (a < ignore_from) {
        const float c_pos = a == 0 ? coef[0] : coef[1], c_neg = coef[2];
        const float c_fg = coef[3], c_bg = coef[4];
        const float s0 = t_dp0[src], s1 = t_dp1[src];
        float acc0 = 0.f, acc1 = 0.f;
        for (int d = 0; d < n_dirs; ++d) {
            const int dy = dir_dy[d], dx = dir_dx[d];
            const int o = dy * LW + dx;
            const int b = t_lab[src + o];
            if (b >= ignore_from) continue;
            const int k0 = dir_start[d], k1 = dir_start[d + 1];
            float m = -INFINITY;
            int arg = 0;
            for (int k = k0; k < k1; ++k) {
                const int off = cell_dy[k] * LW + cell_dx[k];
                const float v = t_edge[src + off];
                if (v > m) {     // strict: the first maximum keeps the gradient
                    m = v;
                    arg = off;
                }
            }
            const float aff = 1.0f - m;
            if (a == b) {
                atomicAdd(&g_edge[src + arg], c_pos / (aff + 1e-5f));           // -g_aff, g_aff = -c / (aff + 1e-5)
                const float p0 = s0 - t_dp0[src + o], p1 = s1 - t_dp1[src + o];
                const float g0 = a > 0 ? c_fg * sgn(p0 - (float)dy) : c_bg * sgn(p0);
                const float g1 = a > 0 ? c_fg * sgn(p1 - (float)dx) : c_bg * sgn(p1);
                acc0 += g0;
                acc1 += g1;
                if (g0 != 0.f) atomicAdd(&g_dp0[src + o], -g0);
                if (g1 != 0.f) atomicAdd(&g_dp1[src + o], -g1);
            } else {
                atomicAdd(&g_edge[src + arg], -c_neg / (1.00001f - aff));
            }
        }
        if (acc0 != 0.f) atomicAdd(&g_dp0[src], acc0);
        if (acc1 != 0.f) atomicAdd(&g_dp1[src], acc1);
    }
    __syncthreads();
    const long plane = (long)hp * wp;
    float *ge = grad_edge + img, *gd = grad_dp + 2 * img;
    for (int i = threadIdx.x; i < cells; i += 256) {
        const int py = i / LW, px = i - py * LW;
        const int gy = ty0 + py, gx = tx0 + px;
        if (gy >= hp || gx >= wp) continue;
        const long g = (long)gy * wp + gx;
        if (g_edge[i] != 0.f) unsafeAtomicAdd(ge + g, g_edge[i]);
        if (g_dp0[i] != 0.f) unsafeAtomicAdd(gd + g, g_dp0[i]);
        if (g_dp1[i] != 0.f) unsafeAtomicAdd(gd + plane + g, g_dp1[i]);
    }
}

// Stage rows [ty0, ty0+LH), cols [tx0, tx0+LW) of the grid, ty0 / tx0 possibly negative (the halo above and to the left of
// an output tile).  Cells outside the grid carry label 255 and are never a source or a destination.
__device__ __forceinline__ void stage_around(const float *__restrict__ edge, const float *__restrict__ dp,
                                             const unsigned char *__restrict__ label, int hp, int wp, int ty0, int tx0,
                                             int LH, int LW, float *t_edge, float *t_dp0, float *t_dp1,
                                             unsigned char *t_lab) {
    const long plane = (long)hp * wp;
    for (int i = threadIdx.x; i < LH * LW; i += 256) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gy = ty0 + ly, gx = tx0 + lx;
        float e = 1.0f, d0 = 0.f, d1 = 0.f;
        unsigned char l = 255;
        if (gy >= 0 && gy < hp && gx >= 0 && gx < wp) {
            const long g = (long)gy * wp + gx;
            e = edge[g];
            d0 = dp[g];
            d1 = dp[plane + g];
            l = label[g];
        }
        t_edge[i] = e;
        t_dp0[i] = d0;
        t_dp1[i] = d1;
        t_lab[i] = l;
    }
}

// Ordered backward: the gather form of aff_loss_backward_kernel.  A thread owns the output cell c and walks the path table
// in its own order (direction d ascending, path cell k ascending).  Table cell (d, k) names the one source s = c - cell(k)
// whose path (s, d) has c as its k-th cell; it contributes iff s is a source, the pair (s, s + dir(d)) is counted, and c
// is the FIRST cell of that path attaining its maximum: every earlier cell < edge[c], every later one <= edge[c] (the
// strict `>` of the scatter).  The path cells of (s, d) lie within radius - 1 of c in both axes, hence the halo.  The
// displacement gradient of c: per direction, c as the source of (c, d), then c as the destination of (c - dir(d), d).
// (d, k) is wave-uniform, so the table is read with scalar loads; the walk of a candidate ends at its first refusal.
__global__ __launch_bounds__(256) void aff_loss_backward_ordered_kernel(
    const float *__restrict__ edge, const float *__restrict__ dp, const unsigned char *__restrict__ label, int hp, int wp,
    int radius, int n_dirs, const int *__restrict__ dir_start, const int *__restrict__ cell_dy,
    const int *__restrict__ cell_dx, const int *__restrict__ dir_dy, const int *__restrict__ dir_dx,
    const float *__restrict__ coef, int ignore_from, float *__restrict__ grad_edge, float *__restrict__ grad_dp) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int halo = radius - 1;
    const int LW = AFF_TW + 2 * halo, LH = AFF_TH + 2 * halo, cells = LH * LW;
    float *t_edge = lds, *t_dp0 = lds + cells, *t_dp1 = lds + 2 * cells;
    unsigned char *t_lab = reinterpret_cast<unsigned char *>(lds + 3 * cells);
    const int tiles_x = (wp + AFF_TW - 1) / AFF_TW;
    const int ty0 = ((int)blockIdx.x / tiles_x) * AFF_TH, tx0 = ((int)blockIdx.x % tiles_x) * AFF_TW;
    const long img = (long)blockIdx.y * hp * wp;
    stage_around(edge + img, dp + 2 * img, label + img, hp, wp, ty0 - halo, tx0 - halo, LH, LW, t_edge, t_dp0, t_dp1, t_lab);
    __syncthreads();

    const int ly = threadIdx.x / AFF_TW, lx = threadIdx.x % AFF_TW;
    const int cy = ty0 + ly, cx = tx0 + lx;
    if (cy >= hp || cx >= wp) return;
    const int ctr = (ly + halo) * LW + lx + halo;
    // the source rectangle: rows [0, sy1), columns [sx0, sx1)
    const int sy1 = hp - halo, sx0 = halo, sx1 = wp - halo;
    const float c_bgp = coef[0], c_fgp = coef[1], c_neg = coef[2], c_fg = coef[3], c_bg = coef[4];
    const float ec = t_edge[ctr], aff = 1.0f - ec;
    // what c receives as the first maximum of a path, by the kind of pair
    const float e_bg = c_bgp / (aff + 1e-5f), e_fg = c_fgp / (aff + 1e-5f), e_neg = -c_neg / (1.00001f - aff);
    const int lc = t_lab[ctr];
    const float q0 = t_dp0[ctr], q1 = t_dp1[ctr];
    const bool c_is_src = cy < sy1 && cx >= sx0 && cx < sx1 && lc < ignore_from;
    float acc_e = 0.f, acc0 = 0.f, acc1 = 0.f;
    for (int d = 0; d < n_dirs; ++d) {
        const int dy = dir_dy[d], dx = dir_dx[d];
        const int o = dy * LW + dx;
        const float fy = (float)dy, fx = (float)dx;
        if (c_is_src && (int)t_lab[ctr + o] == lc) {           // c the source of (c, d): + g
            const float p0 = q0 - t_dp0[ctr + o], p1 = q1 - t_dp1[ctr + o];
            acc0 += lc > 0 ? c_fg * sgn(p0 - fy) : c_bg * sgn(p0);
            acc1 += lc > 0 ? c_fg * sgn(p1 - fx) : c_bg * sgn(p1);
        }
        if (lc < ignore_from && cy - dy >= 0 && cy - dy < sy1 && cx - dx >= sx0 && cx - dx < sx1 && (int)t_lab[ctr - o] == lc) {
            // c the destination of (c - dir, d): - g, chosen by the source's label (equal to c's)
            const float p0 = t_dp0[ctr - o] - q0, p1 = t_dp1[ctr - o] - q1;
            acc0 -= lc > 0 ? c_fg * sgn(p0 - fy) : c_bg * sgn(p0);
            acc1 -= lc > 0 ? c_fg * sgn(p1 - fx) : c_bg * sgn(p1);
        }
        const int k0 = dir_start[d], k1 = dir_start[d + 1];
        for (int k = k0; k < k1; ++k) {
            const int ky = cell_dy[k], kx = cell_dx[k];
            const int sy = cy - ky, sx = cx - kx;
            if (sy < 0 || sy >= sy1 || sx < sx0 || sx >= sx1) continue;
            const int s = ctr - (ky * LW + kx);
            const int a = t_lab[s], b = t_lab[s + o];
            if (a >= ignore_from || b >= ignore_from) continue;
            bool first = true;
            for (int j = k0; j < k1 && first; ++j) {
                const float v = t_edge[s + cell_dy[j] * LW + cell_dx[j]];
                first = j < k ? v < ec : (j == k || v <= ec);
            }
            if (first) acc_e += a != b ? e_neg : (a == 0 ? e_bg : e_fg);
        }
    }
    const long g = (long)cy * wp + cx, plane = (long)hp * wp;
    grad_edge[img + g] = acc_e;
    grad_dp[2 * img + g] = acc0;
    grad_dp[2 * img + plane + g] = acc1;
}

int n_tiles(int hp, int wp, int radius) {
    const int rf = radius - 1;
    return cdiv(hp - rf, AFF_TH) * cdiv(wp - 2 * rf, AFF_TW);
}

// everything that can be refused before a device is touched
int check_args(const char *who, bool pointers, int batch, int hp, int wp, int radius, int ignore_from, const void *ws,
               size_t ws_bytes) {
    if (!pointers || !ws) return fail(IRN_ERR_ARG, "%s: null pointer", who);
    if (ignore_from < 1 || ignore_from > 255) return fail(IRN_ERR_ARG, "%s: ignore_from %d outside 1..255", who, ignore_from);
    if (batch < 1 || batch > 65535) return fail(IRN_ERR_ARG, "%s: batch must be in [1, 65535]", who);
    if (radius < 2 || radius > IRN_MAX_RADIUS) return fail(IRN_ERR_ARG, "%s: radius must be in [2,%d]", who, IRN_MAX_RADIUS);
    if (hp <= radius - 1 || wp <= 2 * (radius - 1))
        return fail(IRN_ERR_ARG, "%s: grid %dx%d too small for radius %d", who, hp, wp, radius);
    if ((long)batch * hp * wp > (1L << 30)) return fail(IRN_ERR_ARG, "%s: batch * hp * wp must be <= 2^30", who);
    if (ws_bytes < irn_aff_loss_workspace_bytes(batch, hp, wp, radius))
        return fail(IRN_ERR_STATE, "%s: workspace of %zu bytes, irn_aff_loss_workspace_bytes asks for %zu", who, ws_bytes,
                    irn_aff_loss_workspace_bytes(batch, hp, wp, radius));
    return IRN_OK;
}

}  // namespace

}  // namespace irn

using namespace irn;

extern "C" size_t irn_aff_loss_workspace_bytes(int batch, int hp, int wp, int radius) {
    if (batch < 1 || batch > 65535 || radius < 2 || radius > IRN_MAX_RADIUS || hp <= radius - 1 || wp <= 2 * (radius - 1))
        return 0;
    return (size_t)batch * n_tiles(hp, wp, radius) * kPartWords * sizeof(double);
}

extern "C" int irn_aff_loss_forward(const float *edge, const float *dp, const uint8_t *label, int batch, int hp, int wp,
                                    int radius, int ignore_from, double *sums, int64_t *counts, void *ws, size_t ws_bytes,
                                    void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_args("irn_aff_loss_forward", edge && dp && label && sums && counts, batch, hp, wp, radius, ignore_from, ws,
                            ws_bytes))
        return rc;
    const int tiles = n_tiles(hp, wp, radius), rf = radius - 1;
    const size_t lds = lds_bytes((AFF_TH + rf) * (AFF_TW + 2 * rf), false);
    const dim3 grid(tiles, batch);
    double *part = (double *)ws;
    if (radius == 10) {
        hipLaunchKernelGGL(aff_loss_forward_kernel<10>, grid, dim3(256), lds, stream, edge, dp, label, hp, wp, radius, 0,
                           nullptr, nullptr, nullptr, nullptr, ignore_from, part);
    } else if (radius == 5) {
        hipLaunchKernelGGL(aff_loss_forward_kernel<5>, grid, dim3(256), lds, stream, edge, dp, label, hp, wp, radius, 0,
                           nullptr, nullptr, nullptr, nullptr, ignore_from, part);
    } else {
        const DeviceTable *tab = nullptr;
        if (int rc = get_device_table(radius, 0, &tab)) return rc;
        hipLaunchKernelGGL(aff_loss_forward_kernel<0>, grid, dim3(256), lds, stream, edge, dp, label, hp, wp, radius,
                           tab->n_dirs, tab->dir_start8, tab->cell_off8, tab->dir_dy, tab->dir_dx, ignore_from, part);
    }
    IRN_LAUNCH_CHECK("aff_loss_forward_kernel");
    hipLaunchKernelGGL(aff_loss_finish_kernel, dim3(1), dim3(256), 0, stream, (const double *)part, tiles * batch, sums,
                       (long long *)counts);
    IRN_LAUNCH_CHECK("aff_loss_finish_kernel");
    return IRN_OK;
}

extern "C" int irn_aff_loss_backward(const float *edge, const float *dp, const uint8_t *label, int batch, int hp, int wp,
                                     int radius, int ignore_from, const float *coef, float *grad_edge, float *grad_dp,
                                     void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_args("irn_aff_loss_backward", edge && dp && label && coef && grad_edge && grad_dp, batch, hp, wp,
                            radius, ignore_from, ws, ws_bytes))
        return rc;
    const DeviceTable *tab = nullptr;
    if (int rc = get_device_table(radius, 0, &tab)) return rc;
    const int rf = radius - 1;
    const size_t n = (size_t)batch * hp * wp;
    IRN_HIP_TRY(hipMemsetAsync(grad_edge, 0, sizeof(float) * n, stream));
    IRN_HIP_TRY(hipMemsetAsync(grad_dp, 0, sizeof(float) * 2 * n, stream));
    const auto kernel = ignore_from == IRN_EVAL_CLASSES ? aff_loss_backward_kernel<IRN_EVAL_CLASSES> : aff_loss_backward_kernel<0>;
    hipLaunchKernelGGL(kernel, dim3(n_tiles(hp, wp, radius), batch), dim3(256),
                       lds_bytes((AFF_TH + rf) * (AFF_TW + 2 * rf), true), stream, edge, dp, label, hp, wp, radius, tab->n_dirs,
                       tab->dir_start, tab->cell_dy, tab->cell_dx, tab->dir_dy, tab->dir_dx, coef, ignore_from, grad_edge,
                       grad_dp);
    IRN_LAUNCH_CHECK("aff_loss_backward_kernel");
    return IRN_OK;
}

extern "C" int irn_aff_loss_backward_ordered(const float *edge, const float *dp, const uint8_t *label, int batch, int hp,
                                             int wp, int radius, int ignore_from, const float *coef, float *grad_edge,
                                             float *grad_dp, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = check_args("irn_aff_loss_backward_ordered", edge && dp && label && coef && grad_edge && grad_dp, batch, hp,
                            wp, radius, ignore_from, ws, ws_bytes))
        return rc;
    const DeviceTable *tab = nullptr;
    if (int rc = get_device_table(radius, 0, &tab)) return rc;
    const int rf = radius - 1;
    // tiles of output cells over the whole grid: every cell of both gradients is stored once, nothing is cleared first
    hipLaunchKernelGGL(aff_loss_backward_ordered_kernel, dim3(cdiv(hp, AFF_TH) * cdiv(wp, AFF_TW), batch), dim3(256),
                       lds_bytes((AFF_TH + 2 * rf) * (AFF_TW + 2 * rf), false), stream, edge, dp, label, hp, wp, radius,
                       tab->n_dirs, tab->dir_start, tab->cell_dy, tab->cell_dx, tab->dir_dy, tab->dir_dx, coef, ignore_from,
                       grad_edge, grad_dp);
    IRN_LAUNCH_CHECK("aff_loss_backward_ordered_kernel");
    return IRN_OK;
}
