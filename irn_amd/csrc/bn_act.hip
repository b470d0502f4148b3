// Inference batch norm (+ residual) (+ ReLU) of the ResNet-50 trunk as ONE pass over the convolution's output, in place:
//     x[n, c, :, :] = act(x[n, c, :, :] * scale[c] + shift[c] (+ res[n, c, :, :] (* res_scale[c] + res_shift[c])))
// with scale = weight / sqrt(running_var + eps), shift = bias - running_mean * scale folded by the caller; the residual may
// carry a batch norm of its own (the projection shortcut of a stage's first unit, net/resnet50.py:48-49, whose output then
// never exists as a tensor of its own).
//
// Replaces the elementwise tail of reference net/resnet50.py:34-54 (Bottleneck.forward: FixedBatchNorm :11-14 ->
// `out += residual` -> ReLU) and of the stem (:94-97): three kernels and seven tensor transfers at the end of a
// bottleneck (batch norm read + write, add two reads + write, ReLU read + write) become one kernel and three; after a
// plain convolution four transfers become two.  The convolutions stay on MIOpen / rocBLAS; measured on the CAM leg
// (profiles/r02_s13_cam_kernel_stats_composed.csv) the elementwise kernels were 28 % of the backbone's time.
//
// HBM-bound (12 or 8 bytes per element).  The tensor is walked flat in 16-byte pieces, so every load and store is a
// full-width coalesced access whatever H x W is (VOC planes are rarely a multiple of 4 wide); a piece that straddles
// a plane boundary takes the next channel's constants for its upper elements.  Plane and channel of a piece come from
// multiply-shift divisions by invariant divisors prepared on the host.
#include "common.hpp"
#include "upsample.hpp"

#pragma clang fp contract(off)

namespace irn {
namespace {

typedef float f4v __attribute__((ext_vector_type(4)));

// n / d for n < 2^31 as mulhi + shift (Granlund-Montgomery round-up multiplier)
struct Div {
    unsigned mul = 0, shr = 0, d = 1;
};

Div make_div(unsigned d) {
    Div r;
    r.d = d;
    if (d == 1) return r;
    unsigned l = 0;
    while ((1ull << l) < d) ++l;                 // ceil(log2 d)
    const unsigned p = 31 + l;
    r.mul = (unsigned)(((1ull << p) + d - 1) / d);
    r.shr = p - 32;
    return r;
}

__device__ __forceinline__ unsigned div_by(unsigned n, const Div dv) {
    return dv.d == 1 ? n : (__umulhi(n, dv.mul) >> dv.shr);
}

constexpr int kThreads = 256, kPieces = 4;       // 16-byte pieces per thread, a block-width apart

// (non-temporal loads of x / res were measured: faster for the one shape that exceeds the caches, 268 MB per tensor — 5.9 vs 5.3
// TB/s with a residual — and 10-20 % slower for every smaller one, whose lines the convolution has just left in L2 / MALL;
// profiles/r02_s19_epilogue_bench.txt)
__device__ __forceinline__ f4v load_piece(const float *p, unsigned i) { return reinterpret_cast<const f4v *>(p)[i]; }

// RES: 0 no residual, 1 residual added as it is, 2 residual through its own scale / shift first.  `out` is `x` itself (the
// inference pass, in place) or another tensor (irn_bn_act_forward, which keeps x for the backward).
template <int RES, bool RELU>
__device__ __forceinline__ void bn_act_pieces(const float *x, float *out, const float *__restrict__ res,
                                              const float *__restrict__ scale, const float *__restrict__ shift,
                                              const float *__restrict__ res_scale, const float *__restrict__ res_shift,
                                              unsigned n_pieces, unsigned hw, unsigned n_ch, Div by_hw, Div by_ch) {
    constexpr bool HAS_RES = RES != 0;
    const unsigned base = blockIdx.x * (unsigned)(kThreads * kPieces) + threadIdx.x;
    f4v v[kPieces], r[kPieces];
#pragma unroll
    for (int j = 0; j < kPieces; ++j) {
        const unsigned p = base + j * kThreads;
        if (p < n_pieces) {
            v[j] = load_piece(x, p);
            if (HAS_RES) r[j] = load_piece(res, p);
        }
    }
#pragma unroll
    for (int j = 0; j < kPieces; ++j) {
        const unsigned p = base + j * kThreads;
        if (p >= n_pieces) continue;
        const unsigned e = p * 4u;
        const unsigned plane = div_by(e, by_hw);
        const unsigned in_plane = e - plane * hw;
        const unsigned c0 = plane - div_by(plane, by_ch) * n_ch;
        const unsigned c1 = c0 + 1 == n_ch ? 0u : c0 + 1;
        const float s0 = scale[c0], b0 = shift[c0];
        float s1 = s0, b1 = b0;
        const unsigned left = hw - in_plane;      // elements of this piece that still belong to plane `plane` (if < 4)
        if (left < 4u) {
            s1 = scale[c1];
            b1 = shift[c1];
        }
        float rs0 = 1.f, rb0 = 0.f, rs1 = 1.f, rb1 = 0.f;
        if (RES == 2) {
            rs0 = rs1 = res_scale[c0];
            rb0 = rb1 = res_shift[c0];
            if (left < 4u) {
                rs1 = res_scale[c1];
                rb1 = res_shift[c1];
            }
        }
        f4v o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool upper = (unsigned)k >= left;
            float y = fmaf(v[j][k], upper ? s1 : s0, upper ? b1 : b0);
            if (RES == 1) y += r[j][k];
            if (RES == 2) y += fmaf(r[j][k], upper ? rs1 : rs0, upper ? rb1 : rb0);
            if (RELU) y = y < 0.f ? 0.f : y;      // NaN stays NaN, like torch.relu
            o[k] = y;
        }
        reinterpret_cast<f4v *>(out)[p] = o;
    }
}

template <int RES, bool RELU>
__global__ __launch_bounds__(kThreads) void bn_act_kernel(float *__restrict__ x, const float *__restrict__ res,
                                                          const float *__restrict__ scale, const float *__restrict__ shift,
                                                          const float *__restrict__ res_scale, const float *__restrict__ res_shift,
                                                          unsigned n_pieces, unsigned hw, unsigned n_ch, Div by_hw, Div by_ch) {
    bn_act_pieces<RES, RELU>(x, x, res, scale, shift, res_scale, res_shift, n_pieces, hw, n_ch, by_hw, by_ch);
}

template <int RES, bool RELU>
__global__ __launch_bounds__(kThreads) void bn_act_forward_kernel(const float *__restrict__ x, float *__restrict__ out,
                                                                  const float *__restrict__ res, const float *__restrict__ scale,
                                                                  const float *__restrict__ shift, const float *__restrict__ res_scale,
                                                                  const float *__restrict__ res_shift, unsigned n_pieces, unsigned hw,
                                                                  unsigned n_ch, Div by_hw, Div by_ch) {
    bn_act_pieces<RES, RELU>(x, out, res, scale, shift, res_scale, res_shift, n_pieces, hw, n_ch, by_hw, by_ch);
}

// one element per thread from `first` on: the last numel % 4 elements, and tensors whose planes are shorter than a piece
template <int RES, bool RELU>
__global__ void bn_act_tail_kernel(const float *x, float *out, const float *__restrict__ res, const float *__restrict__ scale,
                                   const float *__restrict__ shift, const float *__restrict__ res_scale,
                                   const float *__restrict__ res_shift, unsigned first, unsigned numel, unsigned hw, unsigned n_ch) {
    const unsigned e = first + blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= numel) return;
    const unsigned c = (e / hw) % n_ch;
    float y = fmaf(x[e], scale[c], shift[c]);
    if (RES == 1) y += res[e];
    if (RES == 2) y += fmaf(res[e], res_scale[c], res_shift[c]);
    if (RELU) y = y < 0.f ? 0.f : y;
    out[e] = y;
}

// The same pass over a channels-last tensor ([n_pixels, n_ch] in memory, n_ch a multiple of 4): the four elements of a
// 16-byte piece are four consecutive channels of one pixel, so the constants come as 16-byte loads too and no piece
// straddles anything.  (For the trunk run with `IRN_CHANNELS_LAST=1`: MIOpen's NHWC solvers.)
template <int RES, bool RELU>
__global__ __launch_bounds__(kThreads) void bn_act_nhwc_kernel(float *__restrict__ x, const float *__restrict__ res,
                                                               const float *__restrict__ scale, const float *__restrict__ shift,
                                                               const float *__restrict__ res_scale, const float *__restrict__ res_shift,
                                                               unsigned n_pieces, unsigned n_ch, Div by_ch) {
    constexpr bool HAS_RES = RES != 0;
    const unsigned base = blockIdx.x * (unsigned)(kThreads * kPieces) + threadIdx.x;
    f4v v[kPieces], r[kPieces];
#pragma unroll
    for (int j = 0; j < kPieces; ++j) {
        const unsigned p = base + j * kThreads;
        if (p < n_pieces) {
            v[j] = load_piece(x, p);
            if (HAS_RES) r[j] = load_piece(res, p);
        }
    }
#pragma unroll
    for (int j = 0; j < kPieces; ++j) {
        const unsigned p = base + j * kThreads;
        if (p >= n_pieces) continue;
        const unsigned e = p * 4u;
        const unsigned c0 = e - div_by(e, by_ch) * n_ch;          // multiple of 4
        const f4v s = load_piece(scale, c0 >> 2), b = load_piece(shift, c0 >> 2);
        f4v rs, rb;
        if (RES == 2) {
            rs = load_piece(res_scale, c0 >> 2);
            rb = load_piece(res_shift, c0 >> 2);
        }
        f4v o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float y = fmaf(v[j][k], s[k], b[k]);
            if (RES == 1) y += r[j][k];
            if (RES == 2) y += fmaf(r[j][k], rs[k], rb[k]);
            if (RELU) y = y < 0.f ? 0.f : y;
            o[k] = y;
        }
        reinterpret_cast<f4v *>(x)[p] = o;
    }
}

template <int RES, bool RELU>
int launch_nhwc(float *x, const float *res, const float *scale, const float *shift, const float *res_scale, const float *res_shift,
                unsigned numel, unsigned n_ch, hipStream_t stream) {
    const unsigned n_pieces = numel / 4u;
    const unsigned blocks = (n_pieces + kThreads * kPieces - 1) / (kThreads * kPieces);
    hipLaunchKernelGGL((bn_act_nhwc_kernel<RES, RELU>), dim3(blocks), dim3(kThreads), 0, stream, x, res, scale, shift, res_scale,
                       res_shift, n_pieces, n_ch, make_div(n_ch));
    IRN_LAUNCH_CHECK("bn_act_nhwc_kernel");
    return IRN_OK;
}

// out == x: the in-place pass; otherwise x is only read
template <int RES, bool RELU>
int launch(const float *x, float *out, const float *res, const float *scale, const float *shift, const float *res_scale,
           const float *res_shift, unsigned numel, unsigned hw, unsigned n_ch, hipStream_t stream) {
    // planes shorter than a piece (a piece would span more than two of them) go element by element; such maps carry no time
    const unsigned n_pieces = hw >= 4u ? numel / 4u : 0u;
    if (n_pieces) {
        const unsigned blocks = (n_pieces + kThreads * kPieces - 1) / (kThreads * kPieces);
        if (out == x)
            hipLaunchKernelGGL((bn_act_kernel<RES, RELU>), dim3(blocks), dim3(kThreads), 0, stream, out, res, scale, shift, res_scale,
                               res_shift, n_pieces, hw, n_ch, make_div(hw), make_div(n_ch));
        else
            hipLaunchKernelGGL((bn_act_forward_kernel<RES, RELU>), dim3(blocks), dim3(kThreads), 0, stream, x, out, res, scale, shift,
                               res_scale, res_shift, n_pieces, hw, n_ch, make_div(hw), make_div(n_ch));
        IRN_LAUNCH_CHECK("bn_act_kernel");
    }
    const unsigned rest = numel - n_pieces * 4u;
    if (rest) {
        hipLaunchKernelGGL((bn_act_tail_kernel<RES, RELU>), dim3((rest + 63u) / 64u), dim3(64), 0, stream, x, out, res, scale, shift,
                           res_scale, res_shift, n_pieces * 4u, numel, hw, n_ch);
        IRN_LAUNCH_CHECK("bn_act_tail_kernel");
    }
    return IRN_OK;
}

int launch_mode(const float *x, float *out, const float *res, const float *scale, const float *shift, const float *res_scale,
                const float *res_shift, unsigned numel, unsigned hw, unsigned n_ch, int relu, hipStream_t s) {
    const int mode = !res ? 0 : (res_scale ? 2 : 1);
#define IRN_BN_ACT_CASE(RES_MODE)                                                                                       \
    return relu ? launch<RES_MODE, true>(x, out, res, scale, shift, res_scale, res_shift, numel, hw, n_ch, s)          \
                : launch<RES_MODE, false>(x, out, res, scale, shift, res_scale, res_shift, numel, hw, n_ch, s)
    if (mode == 0) IRN_BN_ACT_CASE(0);
    if (mode == 1) IRN_BN_ACT_CASE(1);
    IRN_BN_ACT_CASE(2);
#undef IRN_BN_ACT_CASE
}

// ------------------------------------------------------------------------------------------------
// The training seam: the same tail as a differentiable operator (ops.bn_act).  irn_bn_fold makes scale / shift from the
// layer's parameters in one launch (the optimiser writes them every step), irn_bn_act_forward is the pass above out of
// place, irn_bn_act_backward is its vector-Jacobian product in one pass over the tensors plus a tiny second launch.
// ------------------------------------------------------------------------------------------------

// `FrozenBatchNorm._fold64().float()`: every operation a separate IEEE double operation (contraction is off in this file),
// one rounding to fp32 at the end
__global__ void bn_fold_kernel(const float *__restrict__ weight, const float *__restrict__ bias, const float *__restrict__ mean,
                               const float *__restrict__ var, double eps, int n_ch, float *__restrict__ scale,
                               float *__restrict__ shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_ch) return;
    const double s = (double)weight[c] / sqrt((double)var[c] + eps);
    const double m = (double)mean[c] * s;
    scale[c] = (float)s;
    shift[c] = (float)((double)bias[c] - m);
}

// Backward.  With z = x * scale[c] + shift[c] (+ r) and out = act(z):  dz = grad_out where out > 0 (or NaN), else 0 —
// torch's threshold_backward — and
//     grad_x = dz * scale[c],   grad_res = dz  or  dz * res_scale[c],
//     S0[c] = sum dz,   S1[c] = sum dz * x,   S2[c] = sum dz * res          (over images and plane, in double)
// from which the caller forms the parameter gradients.  A channel's N planes lie C planes apart, so a workgroup takes ONE
// channel and a share of its planes — kBwdShare elements: whole planes of consecutive images while a plane is at most a
// share long, else one kBwdShare-long chunk of one plane — and walks each plane range in 16-byte pieces of the flat tensor
// (a range's first and last piece may hold neighbours' elements: those go element by element, so no store ever touches
// an element of another workgroup).  Sums: per thread in double (the product of two floats is exact in double), a fixed
// shuffle tree per wave, the four waves added in ascending order by thread 0, one partial per (sum, channel, share) in the
// caller's workspace; bn_act_sums_kernel then adds a channel's partials in ascending share order.  No atomics: the same
// inputs give the same bits.  Blocks are numbered share-major, so that concurrent blocks read neighbouring planes.
constexpr int kBwdThreads = 256, kBwdShare = kBwdThreads * 4 * kPieces;      // 4096 elements

struct BwdSplit {
    unsigned chunks;       // shares per plane (1 when a plane fits a share)
    unsigned images;       // images per share (1 when chunks > 1)
    unsigned shares;       // per channel
};

BwdSplit bwd_split(unsigned n_img, unsigned hw) {
    BwdSplit sp;
    sp.chunks = hw > (unsigned)kBwdShare ? (hw + kBwdShare - 1) / kBwdShare : 1u;
    sp.images = sp.chunks > 1 ? 1u : (unsigned)kBwdShare / hw;                  // hw >= 1
    sp.shares = sp.chunks > 1 ? n_img * sp.chunks : (n_img + sp.images - 1) / sp.images;
    return sp;
}

template <bool RES_BN, bool RELU, bool SUMS>
__global__ __launch_bounds__(kBwdThreads) void bn_act_backward_kernel(
    const float *__restrict__ grad_out, const float *__restrict__ out, const float *__restrict__ x, const float *__restrict__ res,
    const float *__restrict__ scale, const float *__restrict__ res_scale, float *__restrict__ grad_x, float *__restrict__ grad_res,
    double *__restrict__ partial, unsigned n_img, unsigned hw, unsigned n_ch, BwdSplit sp) {
    constexpr int NQ = RES_BN ? 3 : 2;
    const unsigned share = blockIdx.x / n_ch, c = blockIdx.x - share * n_ch;
    unsigned n0, n1, first = 0, last = hw;                                      // images [n0, n1), plane range [first, last)
    if (sp.chunks > 1) {
        n0 = share / sp.chunks;
        n1 = n0 + 1;
        first = (share - n0 * sp.chunks) * (unsigned)kBwdShare;
        last = min(hw, first + (unsigned)kBwdShare);
    } else {
        n0 = share * sp.images;
        n1 = min(n_img, n0 + sp.images);
    }
    const float sc = grad_x ? scale[c] : 0.f;
    const float rsc = RES_BN ? res_scale[c] : 1.f;
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
    for (unsigned n = n0; n < n1; ++n) {
        const unsigned plane0 = (n * n_ch + c) * hw;
        const unsigned b = plane0 + first, e = plane0 + last;                  // flat element range of this plane, e < 2^31
        for (unsigned p = (b >> 2) + threadIdx.x; p * 4u < e; p += kBwdThreads) {
            const unsigned e0 = p * 4u;
            const bool whole = e0 >= b && e0 + 4u <= e;
            float g[4], o[4], xv[4], rv[4];
            if (whole) {
                const f4v gv = load_piece(grad_out, p);
#pragma unroll
                for (int k = 0; k < 4; ++k) g[k] = gv[k];
                if (RELU) {
                    const f4v ov = load_piece(out, p);
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[k] = ov[k];
                }
                if (SUMS) {
                    const f4v v = load_piece(x, p);
#pragma unroll
                    for (int k = 0; k < 4; ++k) xv[k] = v[k];
                    if (RES_BN) {
                        const f4v r = load_piece(res, p);
#pragma unroll
                        for (int k = 0; k < 4; ++k) rv[k] = r[k];
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned i = e0 + k;
                    const bool in = i >= b && i < e;
                    g[k] = in ? grad_out[i] : 0.f;                              // an element outside the range adds +0 to every sum
                    o[k] = (RELU && in) ? out[i] : 1.f;
                    xv[k] = (SUMS && in) ? x[i] : 0.f;
                    rv[k] = (SUMS && RES_BN && in) ? res[i] : 0.f;
                }
            }
            float gx[4], gr[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float dz = g[k];
                if (RELU) dz = o[k] <= 0.f ? 0.f : dz;                          // a NaN output lets the gradient pass, as in torch
                gx[k] = dz * sc;
                gr[k] = RES_BN ? dz * rsc : dz;
                if (SUMS) {
                    acc[0] += (double)dz;
                    acc[1] += (double)dz * (double)xv[k];
                    if (RES_BN) acc[2] += (double)dz * (double)rv[k];
                }
            }
            if (whole) {
                if (grad_x) reinterpret_cast<f4v *>(grad_x)[p] = f4v{gx[0], gx[1], gx[2], gx[3]};
                if (grad_res) reinterpret_cast<f4v *>(grad_res)[p] = f4v{gr[0], gr[1], gr[2], gr[3]};
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned i = e0 + k;
                    if (i < b || i >= e) continue;
                    if (grad_x) grad_x[i] = gx[k];
                    if (grad_res) grad_res[i] = gr[k];
                }
            }
        }
    }
    if (!SUMS) return;
    __shared__ double wave_sum[kBwdThreads / 64][NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        double v = acc[q];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
        if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < NQ) {
        double v = wave_sum[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kBwdThreads / 64; ++w) v += wave_sum[w][threadIdx.x];
        partial[((size_t)threadIdx.x * n_ch + c) * sp.shares + share] = v;
    }
}

// sums[q * n_ch + c] = partial[q][c][0] + partial[q][c][1] + ... in that order; one thread per (q, c)
__global__ void bn_act_sums_kernel(const double *__restrict__ partial, double *__restrict__ sums, unsigned n_rows, unsigned shares) {
    const unsigned row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n_rows) return;
    const double *p = partial + (size_t)row * shares;
    double v = p[0];
    for (unsigned s = 1; s < shares; ++s) v += p[s];
    sums[row] = v;
}

template <bool RES_BN, bool RELU, bool SUMS>
int launch_backward(const float *grad_out, const float *out, const float *x, const float *res, const float *scale,
                    const float *res_scale, float *grad_x, float *grad_res, double *sums, double *partial, unsigned n_img,
                    unsigned hw, unsigned n_ch, hipStream_t s) {
    const BwdSplit sp = bwd_split(n_img, hw);
    hipLaunchKernelGGL((bn_act_backward_kernel<RES_BN, RELU, SUMS>), dim3(sp.shares * n_ch), dim3(kBwdThreads), 0, s, grad_out, out, x,
                       res, scale, res_scale, grad_x, grad_res, partial, n_img, hw, n_ch, sp);
    IRN_LAUNCH_CHECK("bn_act_backward_kernel");
    if (SUMS) {
        const unsigned rows = (RES_BN ? 3u : 2u) * n_ch;
        hipLaunchKernelGGL(bn_act_sums_kernel, dim3((rows + 63u) / 64u), dim3(64), 0, s, partial, sums, rows, sp.shares);
        IRN_LAUNCH_CHECK("bn_act_sums_kernel");
    }
    return IRN_OK;
}

}  // namespace
}  // namespace irn

extern "C" int irn_bn_fold(const float *weight_dev, const float *bias_dev, const float *mean_dev, const float *var_dev, double eps,
                           int n_channels, float *scale_dev, float *shift_dev, void *stream) {
    using namespace irn;
    if (!weight_dev || !bias_dev || !mean_dev || !var_dev || !scale_dev || !shift_dev) return fail(IRN_ERR_ARG, "irn_bn_fold: null pointer");
    if (n_channels <= 0) return fail(IRN_ERR_ARG, "irn_bn_fold: %d channels", n_channels);
    hipLaunchKernelGGL(bn_fold_kernel, dim3((unsigned)cdiv(n_channels, 256)), dim3(256), 0, (hipStream_t)stream, weight_dev, bias_dev,
                       mean_dev, var_dev, eps, n_channels, scale_dev, shift_dev);
    IRN_LAUNCH_CHECK("bn_fold_kernel");
    return IRN_OK;
}

extern "C" int irn_bn_act_forward(const float *x_dev, const float *res_dev, const float *scale_dev, const float *shift_dev,
                                  const float *res_scale_dev, const float *res_shift_dev, float *out_dev, int64_t n_images,
                                  int n_channels, int64_t plane_elems, int relu, void *stream) {
    using namespace irn;
    if (!x_dev || !out_dev || !scale_dev || !shift_dev) return fail(IRN_ERR_ARG, "irn_bn_act_forward: null pointer");
    if ((res_scale_dev != nullptr) != (res_shift_dev != nullptr) || (res_scale_dev && !res_dev))
        return fail(IRN_ERR_ARG, "irn_bn_act_forward: res_scale and res_shift come together, and only with a residual");
    if (n_images < 0 || n_channels <= 0 || plane_elems < 0) return fail(IRN_ERR_ARG, "irn_bn_act_forward: negative size");
    if (((uintptr_t)x_dev | (uintptr_t)res_dev | (uintptr_t)out_dev) & 15u)
        return fail(IRN_ERR_ARG, "irn_bn_act_forward: tensors must be 16-byte aligned");
    const int64_t numel = n_images * n_channels * plane_elems;
    if (numel == 0) return IRN_OK;
    if (numel >= (1ll << 31)) return fail(IRN_ERR_ARG, "irn_bn_act_forward: %lld elements; at most 2^31 - 1 per call", (long long)numel);
    if (out_dev < x_dev + numel && x_dev < out_dev + numel) return fail(IRN_ERR_ARG, "irn_bn_act_forward: out overlaps x (in place: irn_bn_act)");
    return launch_mode(x_dev, out_dev, res_dev, scale_dev, shift_dev, res_scale_dev, res_shift_dev, (unsigned)numel, (unsigned)plane_elems,
                       (unsigned)n_channels, relu, (hipStream_t)stream);
}

extern "C" size_t irn_bn_act_backward_workspace_bytes(int64_t n_images, int n_channels, int64_t plane_elems) {
    if (n_images <= 0 || n_channels <= 0 || plane_elems <= 0 || n_images * n_channels * plane_elems >= (1ll << 31)) return 0;
    return (size_t)3 * (size_t)n_channels * irn::bwd_split((unsigned)n_images, (unsigned)plane_elems).shares * sizeof(double);
}

extern "C" int irn_bn_act_backward(const float *grad_out_dev, const float *out_dev, const float *x_dev, const float *res_dev,
                                   const float *scale_dev, const float *res_scale_dev, float *grad_x_dev, float *grad_res_dev,
                                   double *sums_dev, int64_t n_images, int n_channels, int64_t plane_elems, int relu,
                                   void *workspace_dev, size_t workspace_bytes, void *stream) {
    using namespace irn;
    if (!grad_out_dev) return fail(IRN_ERR_ARG, "irn_bn_act_backward: null pointer");
    if (relu && !out_dev) return fail(IRN_ERR_ARG, "irn_bn_act_backward: the ReLU mask needs the forward's output");
    if (grad_x_dev && !scale_dev) return fail(IRN_ERR_ARG, "irn_bn_act_backward: grad_x needs scale");
    if (sums_dev && (!x_dev || (res_scale_dev && !res_dev)))
        return fail(IRN_ERR_ARG, "irn_bn_act_backward: the sums need x, and res when the residual has a batch norm of its own");
    if (n_images < 0 || n_channels <= 0 || plane_elems < 0) return fail(IRN_ERR_ARG, "irn_bn_act_backward: negative size");
    if (((uintptr_t)grad_out_dev | (uintptr_t)out_dev | (uintptr_t)x_dev | (uintptr_t)res_dev | (uintptr_t)grad_x_dev |
         (uintptr_t)grad_res_dev) & 15u)
        return fail(IRN_ERR_ARG, "irn_bn_act_backward: tensors must be 16-byte aligned");
    const int64_t numel = n_images * n_channels * plane_elems;
    if (numel >= (1ll << 31)) return fail(IRN_ERR_ARG, "irn_bn_act_backward: %lld elements; at most 2^31 - 1 per call", (long long)numel);
    hipStream_t s = (hipStream_t)stream;
    const int n_sums = res_scale_dev ? 3 : 2;
    if (numel == 0) {
        if (sums_dev) IRN_HIP_TRY(hipMemsetAsync(sums_dev, 0, sizeof(double) * n_sums * n_channels, s));
        return IRN_OK;
    }
    if (!sums_dev && !grad_x_dev && !grad_res_dev) return IRN_OK;
    if (sums_dev) {
        const size_t need = (size_t)n_sums * n_channels * bwd_split((unsigned)n_images, (unsigned)plane_elems).shares * sizeof(double);
        if (!workspace_dev || workspace_bytes < need || ((uintptr_t)workspace_dev & 7u))
            return fail(IRN_ERR_ARG, "irn_bn_act_backward: workspace of %zu bytes, %zu needed (irn_bn_act_backward_workspace_bytes)",
                        workspace_bytes, need);
    }
    const unsigned ni = (unsigned)n_images, hw = (unsigned)plane_elems, nc = (unsigned)n_channels;
    double *ws = (double *)workspace_dev;
#define IRN_BN_BWD_CASE(RES_BN, SUMS)                                                                                                \
    return relu ? launch_backward<RES_BN, true, SUMS>(grad_out_dev, out_dev, x_dev, res_dev, scale_dev, res_scale_dev, grad_x_dev,   \
                                                      grad_res_dev, sums_dev, ws, ni, hw, nc, s)                                     \
                : launch_backward<RES_BN, false, SUMS>(grad_out_dev, out_dev, x_dev, res_dev, scale_dev, res_scale_dev, grad_x_dev,  \
                                                       grad_res_dev, sums_dev, ws, ni, hw, nc, s)
    if (res_scale_dev) {
        if (sums_dev) IRN_BN_BWD_CASE(true, true);
        IRN_BN_BWD_CASE(true, false);
    }
    if (sums_dev) IRN_BN_BWD_CASE(false, true);
    IRN_BN_BWD_CASE(false, false);
#undef IRN_BN_BWD_CASE
}

extern "C" int irn_bn_act(float *x_dev, const float *res_dev, const float *scale_dev, const float *shift_dev,
                          const float *res_scale_dev, const float *res_shift_dev, int64_t n_images, int n_channels,
                          int64_t plane_elems, int relu, void *stream) {
    using namespace irn;
    if (!x_dev || !scale_dev || !shift_dev) return fail(IRN_ERR_ARG, "irn_bn_act: null pointer");
    if ((res_scale_dev != nullptr) != (res_shift_dev != nullptr) || (res_scale_dev && !res_dev))
        return fail(IRN_ERR_ARG, "irn_bn_act: res_scale and res_shift come together, and only with a residual");
    if (n_images < 0 || n_channels <= 0 || plane_elems < 0) return fail(IRN_ERR_ARG, "irn_bn_act: negative size");
    if (((uintptr_t)x_dev | (uintptr_t)res_dev) & 15u) return fail(IRN_ERR_ARG, "irn_bn_act: tensors must be 16-byte aligned");
    const int64_t numel = n_images * n_channels * plane_elems;
    if (numel == 0) return IRN_OK;
    if (numel >= (1ll << 31)) return fail(IRN_ERR_ARG, "irn_bn_act: %lld elements; at most 2^31 - 1 per call", (long long)numel);
    const unsigned hw = (unsigned)plane_elems, n_ch = (unsigned)n_channels, n = (unsigned)numel;
    hipStream_t s = (hipStream_t)stream;
    return irn::launch_mode(x_dev, x_dev, res_dev, scale_dev, shift_dev, res_scale_dev, res_shift_dev, n, hw, n_ch, relu, s);
}

extern "C" int irn_bn_act_nhwc(float *x_dev, const float *res_dev, const float *scale_dev, const float *shift_dev,
                               const float *res_scale_dev, const float *res_shift_dev, int64_t n_pixels, int n_channels, int relu,
                               void *stream) {
    using namespace irn;
    if (!x_dev || !scale_dev || !shift_dev) return fail(IRN_ERR_ARG, "irn_bn_act_nhwc: null pointer");
    if ((res_scale_dev != nullptr) != (res_shift_dev != nullptr) || (res_scale_dev && !res_dev))
        return fail(IRN_ERR_ARG, "irn_bn_act_nhwc: res_scale and res_shift come together, and only with a residual");
    if (n_pixels < 0 || n_channels <= 0 || (n_channels & 3)) return fail(IRN_ERR_ARG, "irn_bn_act_nhwc: n_channels must be a positive multiple of 4");
    if (((uintptr_t)x_dev | (uintptr_t)res_dev | (uintptr_t)scale_dev | (uintptr_t)shift_dev | (uintptr_t)res_scale_dev |
         (uintptr_t)res_shift_dev) & 15u)
        return fail(IRN_ERR_ARG, "irn_bn_act_nhwc: tensors and constants must be 16-byte aligned");
    const int64_t numel = n_pixels * n_channels;
    if (numel == 0) return IRN_OK;
    if (numel >= (1ll << 31)) return fail(IRN_ERR_ARG, "irn_bn_act_nhwc: %lld elements; at most 2^31 - 1 per call", (long long)numel);
    const unsigned n_ch = (unsigned)n_channels, n = (unsigned)numel;
    hipStream_t s = (hipStream_t)stream;
    const int mode = !res_dev ? 0 : (res_scale_dev ? 2 : 1);
#define IRN_BN_ACT_CASE(RES_MODE)                                                                                                   \
    return relu ? launch_nhwc<RES_MODE, true>(x_dev, res_dev, scale_dev, shift_dev, res_scale_dev, res_shift_dev, n, n_ch, s)      \
                : launch_nhwc<RES_MODE, false>(x_dev, res_dev, scale_dev, shift_dev, res_scale_dev, res_shift_dev, n, n_ch, s)
    if (mode == 0) IRN_BN_ACT_CASE(0);
    if (mode == 1) IRN_BN_ACT_CASE(1);
    IRN_BN_ACT_CASE(2);
#undef IRN_BN_ACT_CASE
}

// ------------------------------------------------------------------------------------------------
// Stem: batch norm + ReLU + 3x3 / stride 2 / pad 1 max pool of reference net/resnet50.py:94-97 (the nets' stage1,
// net/resnet50_cam.py:14, net/resnet50_irn.py:15) in one pass: the largest activation of the trunk (64 x H/2 x W/2) is
// read once and a quarter of it written, instead of read + written by the epilogue and read again by the pool.
// ------------------------------------------------------------------------------------------------
namespace irn {
namespace {

// A workgroup produces a 4 x 64 tile of outputs from a 9 x 129 tile of inputs: the inputs are read once, row-contiguous
// (consecutive lanes = consecutive floats), pass through batch norm + ReLU on their way into LDS (out-of-image taps
// become 0, the ReLU's floor), and every thread takes its 3 x 3 window from there as 8-byte reads (one output = columns
// 2x-1 .. 2x+1 of the tile; lanes a pair of columns apart never share a bank).
constexpr int kPoolW = 64, kPoolH = 4, kPoolInW = 2 * kPoolW + 1, kPoolInH = 2 * kPoolH + 1, kPoolLdsW = 132;

__global__ __launch_bounds__(256) void stem_pool_kernel(const float *__restrict__ x, const float *__restrict__ scale,
                                                        const float *__restrict__ shift, float *__restrict__ out, int n_ch, int h,
                                                        int w, int ho, int wo) {
    __shared__ __attribute__((aligned(16))) float tile[kPoolInH][kPoolLdsW];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int xo0 = blockIdx.x * kPoolW, yo0 = blockIdx.y * kPoolH;
    const unsigned plane = blockIdx.z;
    const float s = scale[plane % (unsigned)n_ch], b = shift[plane % (unsigned)n_ch];
    const float *src = x + (size_t)plane * h * w;
    const int x_in0 = 2 * xo0 - 1, y_in0 = 2 * yo0 - 1;
    // tile[r][c + 1] holds input (y_in0 + r, x_in0 + c); column 0 is padding so that a thread's window starts 8-byte aligned
#pragma unroll
    for (int i = threadIdx.x; i < kPoolInH * kPoolInW; i += 256) {
        const int r = i / kPoolInW, c = i - r * kPoolInW;
        const int yy = y_in0 + r, xx = x_in0 + c;
        float v = 0.f;
        if (yy >= 0 && yy < h && xx >= 0 && xx < w) {
            v = fmaf(src[(size_t)yy * w + xx], s, b);
            v = v < 0.f ? 0.f : v;                                    // NaN stays NaN
        }
        tile[r][c + 1] = v;
    }
    __syncthreads();
    const int xo = xo0 + tx, yo = yo0 + ty;
    if (xo >= wo || yo >= ho) return;
    float m = 0.f;
    bool nan = false;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        // columns 2tx .. 2tx+3 of the LDS row = inputs x_in0 + 2tx - 1 .. + 2: the window is the last three
        const float2 lo = *reinterpret_cast<const float2 *>(&tile[2 * ty + ky][2 * tx]);
        const float2 hi = *reinterpret_cast<const float2 *>(&tile[2 * ty + ky][2 * tx + 2]);
        const float v0 = lo.y, v1 = hi.x, v2 = hi.y;
        nan |= (v0 != v0) | (v1 != v1) | (v2 != v2);
        m = v0 > m ? v0 : m;
        m = v1 > m ? v1 : m;
        m = v2 > m ? v2 : m;
    }
    out[((size_t)plane * ho + yo) * wo + xo] = nan ? __builtin_nanf("") : m;      // torch's max pool propagates NaN
}

// Bilinear x`factor` upsampling (align_corners = False, the scale factor handed to the kernel as nn.Upsample does) + ReLU of
// the IRNet heads, reference net/resnet50_irn.py:36,42,48,72,78,84 followed by nn.ReLU.  Source index and weights as in
// ATen's upsample_bilinear2d: src = (dst + 0.5) / factor - 0.5 clamped at 0, lambda = src - floor(src), and
//     out = (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * c + lx * d)      in fp32, no contraction.
// Bound by the output write (4 or 16 times the input); V consecutive outputs of a row per thread leave as one store.
template <int V, bool RELU>
__global__ __launch_bounds__(256) void upsample_kernel(const float *__restrict__ x, float *__restrict__ out, int h, int w, int ho,
                                                       int wo, float rscale) {
    const int xg = blockIdx.x * 64 + (threadIdx.x & 63);         // group of V outputs
    const int yo = blockIdx.y * 4 + (threadIdx.x >> 6);
    const unsigned plane = blockIdx.z;
    if (xg * V >= wo || yo >= ho) return;
    const UpsampleTap ty = upsample_tap(yo, h, rscale);
    const float ly = ty.l, ly0 = 1.f - ly;
    const float *r0 = x + ((size_t)plane * h + ty.i0) * w, *r1 = x + ((size_t)plane * h + ty.i1) * w;
    float o[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const UpsampleTap tx = upsample_tap(xg * V + v, w, rscale);
        const float lx = tx.l, lx0 = 1.f - lx;
        float val = upsample_blend(r0[tx.i0], r0[tx.i1], r1[tx.i0], r1[tx.i1], lx0, lx, ly0, ly);
        if (RELU) val = val < 0.f ? 0.f : val;
        o[v] = val;
    }
    float *dst = out + ((size_t)plane * ho + yo) * wo + (size_t)xg * V;
    if constexpr (V == 4) *reinterpret_cast<f4v *>(dst) = f4v{o[0], o[1], o[2], o[3]};
    else if constexpr (V == 2) *reinterpret_cast<float2 *>(dst) = float2{o[0], o[1]};
    else dst[0] = o[0];
}

template <int V>
int launch_upsample(const float *x, float *out, unsigned n_planes, int h, int w, int ho, int wo, float rscale, int relu,
                    hipStream_t s) {
    const dim3 grid((unsigned)cdiv(cdiv(wo, V), 64), (unsigned)cdiv(ho, 4), n_planes);
    if (relu) hipLaunchKernelGGL((upsample_kernel<V, true>), grid, dim3(256), 0, s, x, out, h, w, ho, wo, rscale);
    else hipLaunchKernelGGL((upsample_kernel<V, false>), grid, dim3(256), 0, s, x, out, h, w, ho, wo, rscale);
    IRN_LAUNCH_CHECK("upsample_kernel");
    return IRN_OK;
}

// Backward of upsample_kernel, as a gather: one thread owns the input cell (y, x) and adds, rows ascending and columns
// ascending within a row, grad_out (masked by out > 0 behind the ReLU) times the weight the forward gave the cell; one store.
// Which outputs touch input index i: those whose first tap i0 is i - 1 or i.  In exact arithmetic i0 = floor((o + 0.5) / f
// - 0.5) lies in [i - 1, i] for f*i - f/2 - 0.5 <= o < f*i + 3f/2 - 0.5 (the clamp at 0 only moves outputs onto i = 0 that
// the range already holds; the clamp of the second tap adds none).  The loop runs over that range widened by one output on
// each side (upsample_below / upsample_above), which covers the rounding of the fp32 mapping, and takes the weights from the
// forward's own expressions (upsample_weight, upsample.hpp): an output outside the true support weighs exactly 0 and is skipped.
template <bool RELU>
__global__ __launch_bounds__(256) void upsample_backward_kernel(const float *__restrict__ grad_out, const float *__restrict__ out,
                                                                float *__restrict__ grad_in, int h, int w, int ho, int wo,
                                                                int factor, float rscale) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const unsigned plane = blockIdx.z;
    if (x >= w || y >= h) return;
    const int below = upsample_below(factor), above = upsample_above(factor);
    const int yo0 = max(0, factor * y - below), yo1 = min(ho, factor * y + above);
    const int xo0 = max(0, factor * x - below), xo1 = min(wo, factor * x + above);
    const float *g = grad_out + (size_t)plane * ho * wo;
    const float *o = RELU ? out + (size_t)plane * ho * wo : nullptr;
    float acc = 0.f;
    for (int yo = yo0; yo < yo1; ++yo) {
        const float wy = upsample_weight(yo, y, h, rscale);
        if (wy == 0.f) continue;
        for (int xo = xo0; xo < xo1; ++xo) {
            const float wx = upsample_weight(xo, x, w, rscale);
            if (wx == 0.f) continue;
            const size_t at = (size_t)yo * wo + xo;
            float v = g[at];
            if (RELU) v = o[at] > 0.f ? v : 0.f;
            acc += v * (wy * wx);
        }
    }
    grad_in[((size_t)plane * h + y) * w + x] = acc;
}

}  // namespace
}  // namespace irn

extern "C" int irn_stem_pool(const float *x_dev, const float *scale_dev, const float *shift_dev, int64_t n_images, int n_channels,
                             int h, int w, float *out_dev, void *stream) {
    using namespace irn;
    if (!x_dev || !scale_dev || !shift_dev || !out_dev) return fail(IRN_ERR_ARG, "irn_stem_pool: null pointer");
    if (n_images < 0 || n_channels <= 0 || h <= 0 || w <= 0) return fail(IRN_ERR_ARG, "irn_stem_pool: non-positive size");
    const int64_t n_planes = n_images * n_channels;
    if (n_planes == 0) return IRN_OK;
    const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
    if (cdiv(ho, 4) > 65535) return fail(IRN_ERR_ARG, "irn_stem_pool: %d rows; at most 524280", h);
    if (n_channels > 65535) return fail(IRN_ERR_ARG, "irn_stem_pool: %d channels; at most 65535", n_channels);
    // the plane index rides on grid.z (at most 65535 per launch); launches start at whole images so that plane % n_channels holds
    const int64_t step = (int64_t)(65535 / n_channels) * n_channels;
    for (int64_t p0 = 0; p0 < n_planes; p0 += step) {
        const unsigned np = (unsigned)((n_planes - p0) < step ? (n_planes - p0) : step);
        hipLaunchKernelGGL(stem_pool_kernel, dim3((unsigned)cdiv(wo, 64), (unsigned)cdiv(ho, 4), np), dim3(256), 0, (hipStream_t)stream,
                           x_dev + (size_t)p0 * h * w, scale_dev, shift_dev, out_dev + (size_t)p0 * ho * wo, n_channels, h, w, ho, wo);
        IRN_LAUNCH_CHECK("stem_pool_kernel");
    }
    return IRN_OK;
}

extern "C" int irn_upsample_bilinear(const float *x_dev, int64_t n_planes, int h, int w, int factor, int relu, float *out_dev,
                                     void *stream) {
    using namespace irn;
    if (!x_dev || !out_dev) return fail(IRN_ERR_ARG, "irn_upsample_bilinear: null pointer");
    if (n_planes < 0 || h <= 0 || w <= 0 || factor < 1 || factor > 64)
        return fail(IRN_ERR_ARG, "irn_upsample_bilinear: non-positive size or factor outside 1..64");
    if ((uintptr_t)out_dev & 15u) return fail(IRN_ERR_ARG, "irn_upsample_bilinear: output must be 16-byte aligned");
    if (n_planes == 0) return IRN_OK;
    const int ho = h * factor, wo = w * factor;
    if (cdiv(ho, 4) > 65535) return fail(IRN_ERR_ARG, "irn_upsample_bilinear: %d output rows; at most 262140", ho);
    const float rscale = (float)(1.0 / (double)factor);
    for (int64_t p0 = 0; p0 < n_planes; p0 += 65535) {
        const unsigned np = (unsigned)((n_planes - p0) < 65535 ? (n_planes - p0) : 65535);
        const float *xs = x_dev + (size_t)p0 * h * w;
        float *os = out_dev + (size_t)p0 * ho * wo;
        int rc;
        // rows start at multiples of wo elements: a 16-byte store needs wo % 4 == 0 (plane and row starts then stay aligned)
        if (wo % 4 == 0) rc = launch_upsample<4>(xs, os, np, h, w, ho, wo, rscale, relu, (hipStream_t)stream);
        else if (wo % 2 == 0) rc = launch_upsample<2>(xs, os, np, h, w, ho, wo, rscale, relu, (hipStream_t)stream);
        else rc = launch_upsample<1>(xs, os, np, h, w, ho, wo, rscale, relu, (hipStream_t)stream);
        if (rc != IRN_OK) return rc;
    }
    return IRN_OK;
}

extern "C" int irn_upsample_bilinear_backward(const float *grad_out_dev, const float *out_dev, int64_t n_planes, int h, int w,
                                              int factor, int relu, float *grad_in_dev, void *stream) {
    using namespace irn;
    if (!grad_out_dev || !grad_in_dev) return fail(IRN_ERR_ARG, "irn_upsample_bilinear_backward: null pointer");
    if (relu && !out_dev) return fail(IRN_ERR_ARG, "irn_upsample_bilinear_backward: the ReLU mask needs the forward's output");
    if (n_planes < 0 || h <= 0 || w <= 0 || factor < 1 || factor > 64)
        return fail(IRN_ERR_ARG, "irn_upsample_bilinear_backward: non-positive size or factor outside 1..64");
    if (n_planes == 0) return IRN_OK;
    const int ho = h * factor, wo = w * factor;
    if (cdiv(ho, 4) > 65535) return fail(IRN_ERR_ARG, "irn_upsample_bilinear_backward: %d output rows; at most 262140", ho);
    const float rscale = (float)(1.0 / (double)factor);
    for (int64_t p0 = 0; p0 < n_planes; p0 += 65535) {
        const unsigned np = (unsigned)((n_planes - p0) < 65535 ? (n_planes - p0) : 65535);
        const float *gs = grad_out_dev + (size_t)p0 * ho * wo;
        const float *os = out_dev ? out_dev + (size_t)p0 * ho * wo : nullptr;
        float *gi = grad_in_dev + (size_t)p0 * h * w;
        const dim3 grid((unsigned)cdiv(w, 64), (unsigned)cdiv(h, 4), np);
        if (relu)
            hipLaunchKernelGGL(upsample_backward_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, gs, os, gi, h, w, ho, wo,
                               factor, rscale);
        else
            hipLaunchKernelGGL(upsample_backward_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, gs, os, gi, h, w, ho, wo,
                               factor, rscale);
        IRN_LAUNCH_CHECK("upsample_backward_kernel");
    }
    return IRN_OK;
}
