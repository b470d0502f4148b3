// Path-max affinity kernel (gfx950).
//
// Replaces reference misc/indexing.py:91-109 (`edge_to_affinity`: 9-20 index_select + max_pool2d
// launches over int64 index tensors) by one kernel that stages an edge tile with its radial halo in
// LDS and walks the (dy,dx) path table itself.  Two instantiations:
//   POW=false : aff = 1 - max(edge over path)          (API form, reference channel order)
//   POW=true  : w   = fp32(aff ** beta)                (walk weight table, raster plane order;
//               fuses the Hadamard power of misc/indexing.py:133)
//
// Roofline: per source pixel the kernel reads n_cells LDS words (242 at r=5, 2134 at r=10) and writes n_dirs floats
// (34 / 152) in one pass; it runs once per image against 2^exp_times sweeps of the walk, so it is <5 % of the path
// (DESIGN.md §kernels).  Measured on the default workload (192 images of 128x128, radius 10, 1.87 GB of planes;
// profiles/affinity_wide_ab.txt): the one-pixel-per-lane form with 4-byte reads took 0.50 ms + 0.03 ms for the pads;
// two pixels per lane with 8-byte reads, the power loop cut to the products that reach the result, 8-byte stores and the
// pads in the same launch take 0.12 ms less.  Of that, 0.08 ms came with the 8-byte reads and stores and 0.04 ms with
// the shorter power loop: the LDS array and the vector pipe both bound the old form; what is left writes at ~4.5 TB/s.
#include "path_unroll.hpp"

namespace irn {

namespace {

__device__ __forceinline__ float pow_beta(float a, float beta, int beta_int) {
    // torch.pow(fp32, beta) is a <=1-ulp powf; the fp64 power rounded once to fp32 is the
    // correctly rounded value and so agrees with it to 1 ulp.
    double b = (double)a;
    if (beta_int > 0) {
        double r = 1.0;
        int e = beta_int;
        while (e) {
            if (e & 1) r *= b;
            b *= b;
            e >>= 1;
        }
        return (float)r;
    }
    return (float)pow(b, (double)beta);
}

template <bool POW>
__global__ __launch_bounds__(256) void affinity_kernel(const AffJob *__restrict__ jobs,
                                                       const int *__restrict__ dir_start8,
                                                       const int *__restrict__ cell_off8, int n_dirs,
                                                       int radius, float beta, int beta_int) {
    extern __shared__ float tile[];
    const AffJob J = jobs[blockIdx.y];
    const int tiles_x = (J.sw + AFF_TW - 1) / AFF_TW;
    const int tiles_y = (J.sh + AFF_TH - 1) / AFF_TH;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;
    const int halo = radius - 1;
    const int LW = AFF_TW + 2 * halo;
    const int LH = AFF_TH + halo;
    const int ty0 = ((int)blockIdx.x / tiles_x) * AFF_TH;
    const int tx0 = ((int)blockIdx.x % tiles_x) * AFF_TW;

    // stage the edge tile: rows [ty0, ty0+TH+halo), cols [tx0-halo, tx0+TW+halo) of the source
    // rectangle, translated into the grid; anything outside the grid is a boundary (edge = 1),
    // which is what the reference's F.pad(..., value=1.0) supplies (misc/indexing.py:150).
    for (int i = threadIdx.x; i < LH * LW; i += 256) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gy = J.oy + ty0 + ly;
        const int gx = J.ox + tx0 + lx - halo;
        float v = 1.0f;
        if (gy < J.gh && gx >= 0 && gx < J.gw) v = J.edge[(long)gy * J.gw + gx];
        tile[i] = v;
    }
    __syncthreads();

    const int ly = threadIdx.x / AFF_TW, lx = threadIdx.x % AFF_TW;
    const int sy = ty0 + ly, sx = tx0 + lx;
    const bool valid = sy < J.sh && sx < J.sw;
    const int base = ly * LW + lx + halo;
    float *out = J.out + (long)sy * J.sw + sx;

    // Eight path cells per scalar load of their (wave-uniform) LDS offsets.  The first version
    // fetched dy and dx of one cell at a time: two scalar loads, a multiply and a wait that also
    // drained the LDS reads per cell — latency-bound, ~10x off the LDS/VALU bound of the kernel.
    const float *tb = tile + base;
    for (int d = 0; d < n_dirs; ++d) {
        const int k0 = dir_start8[d], k1 = dir_start8[d + 1];
        float m0 = -INFINITY, m1 = -INFINITY;
        for (int k = k0; k < k1; k += 8) {
            const int4 oa = *reinterpret_cast<const int4 *>(cell_off8 + k);
            const int4 ob = *reinterpret_cast<const int4 *>(cell_off8 + k + 4);
            const float a0 = tb[oa.x], a1 = tb[oa.y], a2 = tb[oa.z], a3 = tb[oa.w];
            const float b0 = tb[ob.x], b1 = tb[ob.y], b2 = tb[ob.z], b3 = tb[ob.w];
            // v_max3_f32 directly: fmaxf() on values fresh from memory is preceded by a canonicalising v_max_f32 v, v, v
            // each (8 extra vector instructions per 8 cells in a loop the vector pipe bounds)
            m0 = max3(max3(m0, a0, a1), a2, a3);
            m1 = max3(max3(m1, b0, b1), b2, b3);
        }
        const float m = max3(m0, m1, m1);
        float a = 1.0f - m;
        if (POW) a = pow_beta(a, beta, beta_int);
        if (valid) out[(long)d * J.plane_stride] = a;
    }
}

// ------------------------------------------------------------------------------------------------
// The same kernel with the path table as a compile-time constant (radius 5 and 10, raster plane order: the walk's
// weight table).  In the table-driven loop above every LDS read costs a vector add for its address (the cell's offset
// arrives in a scalar register) and the loop is bound by the vector pipe (profiles/r02_s27_affinity_counters.txt: 11.5 k
// vector instructions per wave for 2.6 k LDS reads).  Unrolled, the cell offsets are the immediate offsets of the
// ds_read instructions, and a lane computes AFF_P horizontally adjacent pixels: every path cell is one aligned
// 4*AFF_P-byte read (path_unroll.hpp: WideTile, path_max_wide) that serves AFF_P v_max3 chains.
// The blocks behind the tiles of an image zero what no tile writes: every plane's front pad and tail (AffJob).
// ------------------------------------------------------------------------------------------------
constexpr int AFF_P = 2;           // pixels per lane
constexpr int AFF_PAD_BLOCKS = 8;  // blocks per image that zero the pads

typedef __attribute__((address_space(1))) float global_float;   // the planes are global memory: no flat stores, whose
template <int P>                                                // LDS-side counter the tile reads would wait on
using global_floatP = __attribute__((address_space(1))) floatP<P>;

template <int R, int P>
__global__ __launch_bounds__(256) void affinity_wide_kernel(const AffJob *__restrict__ jobs, int beta_int, int max_tiles) {
    using T = WideTile<R, P>;
    constexpr int ND = kPaths<R>.n_dirs;
    __shared__ __attribute__((aligned(16))) float tile[P * T::COPY];
    const AffJob J = jobs[blockIdx.y];
    if ((int)blockIdx.x >= max_tiles) {
        // [out - pad_front, out) and [out + sh*sw, out + sh*sw + pad_tail) of every plane
        const long n = (long)J.sh * J.sw;
        for (int d = (int)blockIdx.x - max_tiles; d < ND; d += AFF_PAD_BLOCKS) {
            float *plane = J.out + (long)d * J.plane_stride;
            for (int i = threadIdx.x; i < J.pad_front; i += 256) plane[i - J.pad_front] = 0.f;
            for (int i = threadIdx.x; i < J.pad_tail; i += 256) plane[n + i] = 0.f;
        }
        return;
    }
    const int tiles_x = (J.sw + T::TW - 1) / T::TW;
    const int tiles_y = (J.sh + T::TH - 1) / T::TH;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;
    const int ty0 = ((int)blockIdx.x / tiles_x) * T::TH;
    const int tx0 = ((int)blockIdx.x % tiles_x) * T::TW;
    for (int i = threadIdx.x; i < T::LH * T::LW; i += 256) {          // staging as in affinity_kernel, once per copy
        const int ly = i / T::LW, lx = i - ly * T::LW;
        const int gy = J.oy + ty0 + ly;
        const int gx = J.ox + tx0 + lx - T::HALO;
        float v = 1.0f;
        if (gy < J.gh && gx >= 0 && gx < J.gw) v = J.edge[(long)gy * J.gw + gx];
#pragma unroll
        for (int s = 0; s < P; ++s)
            if (lx >= s) tile[s * T::COPY + ly * T::STRIDE + lx - s] = v;   // copy s, shifted left by s floats
    }
    __syncthreads();
    const int ly = threadIdx.x / T::LANES_X, lx = (threadIdx.x % T::LANES_X) * P;
    const int sy = ty0 + ly, sx = tx0 + lx;
    // cell (cy, cx) of pixel sx + p sits at float cy * STRIDE + cx + HALO + p of copy 0 from here
    const unsigned tb = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)tile + 4 * (ly * T::STRIDE + lx);
    global_float *out = (global_float *)J.out + (long)sy * J.sw + sx;
    const int n_valid = sy < J.sh ? min(P, J.sw - sx) : 0;        // pixels of this lane inside the source rectangle
    // one 4P-byte store where the lane's pixels are all inside and the address is aligned in every plane
    const bool vec = n_valid == P && ((uintptr_t)out & (4 * P - 1)) == 0 && J.plane_stride % P == 0;
    auto planes = [&](auto wide) __attribute__((always_inline)) {
        static_for<ND>([&](auto id) __attribute__((always_inline)) {
            constexpr int d = decltype(id)::value;
            const floatP<P> m = path_max_wide<R, P, d>(tb);
            // integer beta only (the launch sends any other beta to the table-driven kernel): the general fp64 pow()
            // inlined once per direction would be 300 KB of code
            // The square-and-multiply loop of affinity_kernel's pow_beta without what does not reach the result: the
            // multiplications of 1.0 by the first factor (exact) and the squarings behind the top bit.  Same products,
            // same roundings.  beta_int is uniform: the empty asm keeps `if (e & 1)` a scalar branch, not a select.
            double b[P], r[P];
            static_for<P>([&](auto ip) __attribute__((always_inline)) { b[decltype(ip)::value] = (double)(1.0f - m[decltype(ip)::value]); });
            int e = beta_int;
            for (; e > 1 && !(e & 1); e >>= 1)   // (e >= 1 by the launch; bounded whatever arrives)
                static_for<P>([&](auto ip) __attribute__((always_inline)) { b[decltype(ip)::value] *= b[decltype(ip)::value]; });
            static_for<P>([&](auto ip) __attribute__((always_inline)) { r[decltype(ip)::value] = b[decltype(ip)::value]; });
            for (e >>= 1; e; e >>= 1) {
                static_for<P>([&](auto ip) __attribute__((always_inline)) { b[decltype(ip)::value] *= b[decltype(ip)::value]; });
                if (e & 1) {
                    asm volatile("");
                    static_for<P>([&](auto ip) __attribute__((always_inline)) { r[decltype(ip)::value] *= b[decltype(ip)::value]; });
                }
            }
            floatP<P> w;
            static_for<P>([&](auto ip) __attribute__((always_inline)) { w[decltype(ip)::value] = (float)r[decltype(ip)::value]; });
            if constexpr (decltype(wide)::value) {
                *reinterpret_cast<global_floatP<P> *>(out) = w;
            } else {
                static_for<P>([&](auto ip) __attribute__((always_inline)) {
                    constexpr int p = decltype(ip)::value;
                    if (p < n_valid) out[p] = w[p];
                });
            }
            out += J.plane_stride;
        });
    };
    // Two copies of the stream, chosen per wave: the one with the wide stores carries no per-plane predicates (its lanes
    // are switched off once, here) and is the one every wave of an even-width, aligned grid runs; a wave with a ragged
    // or unaligned lane stores pixel by pixel, all of its lanes.  67 KB and 74 KB of straight-line code at radius 10
    // (the one-pixel stream was ~40 KB); a wave runs one of them, and the times in the header are with that fetch.
    if (__builtin_amdgcn_ballot_w64(n_valid > 0 && !vec) == 0) {
        if (vec) planes(std::true_type{});
    } else {
        planes(std::false_type{});
    }
}

// Backward of edge_to_affinity for the training seam (reference net/resnet50_irn.py:162-175: index_select
// + max_pool2d over the path axis; autograd sends the gradient of aff[d,s] to the FIRST path cell that
// attains the maximum, negated because aff = 1 - max).  The forward's edge tile is rebuilt in LDS and the
// arg-max is recomputed (nothing is saved by the forward); gradients of a workgroup are gathered in an
// LDS tile with ds_add_f32 and flushed with one global atomic per touched cell, so overlapping halos of
// neighbouring workgroups meet in HBM only once per cell instead of once per (pixel, direction).
__global__ __launch_bounds__(256) void affinity_backward_kernel(const AffJob *__restrict__ jobs,
                                                                const float *const *__restrict__ grad_aff,
                                                                float *const *__restrict__ grad_edge,
                                                                const int *__restrict__ dir_start,
                                                                const int *__restrict__ cell_dy,
                                                                const int *__restrict__ cell_dx, int n_dirs, int radius) {
    extern __shared__ float tile[];
    const AffJob J = jobs[blockIdx.y];
    const int tiles_x = (J.sw + AFF_TW - 1) / AFF_TW;
    const int tiles_y = (J.sh + AFF_TH - 1) / AFF_TH;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;
    const int halo = radius - 1;
    const int LW = AFF_TW + 2 * halo;
    const int LH = AFF_TH + halo;
    float *gtile = tile + LH * LW;
    const int ty0 = ((int)blockIdx.x / tiles_x) * AFF_TH;
    const int tx0 = ((int)blockIdx.x % tiles_x) * AFF_TW;
    for (int i = threadIdx.x; i < LH * LW; i += 256) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gy = J.oy + ty0 + ly;
        const int gx = J.ox + tx0 + lx - halo;
        float v = 1.0f;
        if (gy < J.gh && gx >= 0 && gx < J.gw) v = J.edge[(long)gy * J.gw + gx];
        tile[i] = v;
        gtile[i] = 0.f;
    }
    __syncthreads();
    const int ly = threadIdx.x / AFF_TW, lx = threadIdx.x % AFF_TW;
    const int sy = ty0 + ly, sx = tx0 + lx;
    const bool valid = sy < J.sh && sx < J.sw;
    const int base = ly * LW + lx + halo;
    const float *ga = grad_aff[blockIdx.y] + (long)sy * J.sw + sx;
    if (valid) {
        for (int d = 0; d < n_dirs; ++d) {
            const int k0 = dir_start[d], k1 = dir_start[d + 1];
            float m = -INFINITY;
            int arg = 0;
            for (int k = k0; k < k1; ++k) {
                const int off = cell_dy[k] * LW + cell_dx[k];
                const float v = tile[base + off];
                if (v > m) {     // strict: the first maximum keeps the gradient, like max_pool2d
                    m = v;
                    arg = off;
                }
            }
            atomicAdd(&gtile[base + arg], -ga[(long)d * J.plane_stride]);
        }
    }
    __syncthreads();
    float *ge = grad_edge[blockIdx.y];
    for (int i = threadIdx.x; i < LH * LW; i += 256) {
        const float g = gtile[i];
        if (g == 0.f) continue;
        const int py = i / LW, px = i - py * LW;
        const int gy = J.oy + ty0 + py;
        const int gx = J.ox + tx0 + px - halo;
        if (gy < J.gh && gx >= 0 && gx < J.gw) unsafeAtomicAdd(ge + (long)gy * J.gw + gx, g);
    }
}

}  // namespace

bool affinity_writes_pads(const DeviceTable &tab, bool with_pow, float beta) {
    return with_pow && tab.order == 1 && (tab.radius == 10 || tab.radius == 5) && beta == (float)(int)beta &&
           beta >= 1.0f && beta <= 64.0f;
}

int launch_affinity(const AffJob *jobs_dev, int n_jobs, int max_sh, int max_sw, const DeviceTable &tab,
                    bool with_pow, float beta, hipStream_t stream) {
    const int halo = tab.radius - 1;
    const size_t lds = sizeof(float) * (AFF_TH + halo) * (AFF_TW + 2 * halo);
    int beta_int = 0;
    if (with_pow && beta == (float)(int)beta && beta >= 1.0f && beta <= 64.0f) beta_int = (int)beta;
    if (affinity_writes_pads(tab, with_pow, beta)) {
        using T = WideTile<10, AFF_P>;
        static_assert(T::TW == WideTile<5, AFF_P>::TW && T::TH == WideTile<5, AFF_P>::TH, "one tile for both radii");
        const int tiles = cdiv(max_sh, T::TH) * cdiv(max_sw, T::TW);
        dim3 grid(tiles + AFF_PAD_BLOCKS, n_jobs);
        if (tab.radius == 10)
            hipLaunchKernelGGL((affinity_wide_kernel<10, AFF_P>), grid, dim3(256), 0, stream, jobs_dev, beta_int, tiles);
        else
            hipLaunchKernelGGL((affinity_wide_kernel<5, AFF_P>), grid, dim3(256), 0, stream, jobs_dev, beta_int, tiles);
        IRN_LAUNCH_CHECK("affinity_wide_kernel");
        return IRN_OK;
    }
    dim3 grid(cdiv(max_sh, AFF_TH) * cdiv(max_sw, AFF_TW), n_jobs);
    if (with_pow)
        hipLaunchKernelGGL(affinity_kernel<true>, grid, dim3(256), lds, stream, jobs_dev, tab.dir_start8,
                           tab.cell_off8, tab.n_dirs, tab.radius, beta, beta_int);
    else
        hipLaunchKernelGGL(affinity_kernel<false>, grid, dim3(256), lds, stream, jobs_dev, tab.dir_start8,
                           tab.cell_off8, tab.n_dirs, tab.radius, beta, beta_int);
    IRN_LAUNCH_CHECK("affinity_kernel");
    return IRN_OK;
}

}  // namespace irn

// ------------------------------------------------------------------------------------------------
// C ABI: path table + edge_to_affinity
// ------------------------------------------------------------------------------------------------
using namespace irn;

extern "C" int irn_version(void) { return IRN_ABI_VERSION; }

extern "C" const char *irn_last_error(void) { return last_error_slot().c_str(); }

extern "C" int irn_path_count(int radius, int *n_dirs, int *n_cells) {
    if (radius < 2 || radius > IRN_MAX_RADIUS || !n_dirs || !n_cells)
        return fail(IRN_ERR_ARG, "irn_path_count: radius must be in [2,%d]", IRN_MAX_RADIUS);
    PathTable t = build_path_table(radius, 0);
    *n_dirs = t.n_dirs();
    *n_cells = t.n_cells();
    return IRN_OK;
}

extern "C" int irn_path_table(int radius, int order, int32_t *dst_dydx, int32_t *path_start,
                              int32_t *cells_dydx) {
    if (radius < 2 || radius > IRN_MAX_RADIUS || (order != 0 && order != 1) || !dst_dydx || !path_start ||
        !cells_dydx)
        return fail(IRN_ERR_ARG, "irn_path_table: bad argument");
    PathTable t = build_path_table(radius, order);
    for (int i = 0; i < t.n_dirs(); ++i) {
        dst_dydx[2 * i] = t.dy[i];
        dst_dydx[2 * i + 1] = t.dx[i];
    }
    for (int i = 0; i <= t.n_dirs(); ++i) path_start[i] = t.start[i];
    for (int i = 0; i < t.n_cells(); ++i) {
        cells_dydx[2 * i] = t.cy[i];
        cells_dydx[2 * i + 1] = t.cx[i];
    }
    return IRN_OK;
}

extern "C" int irn_edge_to_affinity(const float *edge_dev, int batch, int hp, int wp, int radius,
                                    float *aff_dev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!edge_dev || !aff_dev || batch < 1 || radius < 2 || radius > IRN_MAX_RADIUS)
        return fail(IRN_ERR_ARG, "irn_edge_to_affinity: bad argument");
    const int rf = radius - 1;
    const int sh = hp - rf, sw = wp - 2 * rf;
    if (sh < 1 || sw < 1)
        return fail(IRN_ERR_ARG, "irn_edge_to_affinity: grid %dx%d too small for radius %d", hp, wp, radius);
    const DeviceTable *tab = nullptr;
    int rc = get_device_table(radius, 0, &tab);
    if (rc) return rc;
    // job descriptors live in a small device buffer owned by the table cache (library-private)
    std::vector<AffJob> jobs(batch);
    const long ns = (long)sh * sw;
    for (int b = 0; b < batch; ++b) {
        AffJob &j = jobs[b];
        j.edge = edge_dev + (long)b * hp * wp;
        j.out = aff_dev + (long)b * tab->n_dirs * ns;
        j.gh = hp; j.gw = wp; j.oy = 0; j.ox = rf; j.sh = sh; j.sw = sw;
        j.plane_stride = ns;
    }
    AffJob *jobs_dev = nullptr;
    rc = scratch_upload(jobs.data(), sizeof(AffJob) * batch, (void **)&jobs_dev, stream);
    if (rc) return rc;
    rc = launch_affinity(jobs_dev, batch, sh, sw, *tab, false, 0.f, stream);
    if (rc) return rc;
    return scratch_release(stream);
}

extern "C" int irn_edge_to_affinity_backward(const float *edge_dev, const float *grad_aff_dev, int batch, int hp, int wp,
                                             int radius, float *grad_edge_dev, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!edge_dev || !grad_aff_dev || !grad_edge_dev || batch < 1 || radius < 2 || radius > IRN_MAX_RADIUS)
        return fail(IRN_ERR_ARG, "irn_edge_to_affinity_backward: bad argument");
    const int rf = radius - 1;
    const int sh = hp - rf, sw = wp - 2 * rf;
    if (sh < 1 || sw < 1)
        return fail(IRN_ERR_ARG, "irn_edge_to_affinity_backward: grid %dx%d too small for radius %d", hp, wp, radius);
    const DeviceTable *tab = nullptr;
    int rc = get_device_table(radius, 0, &tab);
    if (rc) return rc;
    const long ns = (long)sh * sw;
    // descriptors + the two pointer arrays in one upload
    std::vector<char> host(sizeof(AffJob) * batch + 2 * sizeof(void *) * batch);
    AffJob *jobs = (AffJob *)host.data();
    const float **gas = (const float **)(host.data() + sizeof(AffJob) * batch);
    float **ges = (float **)(host.data() + sizeof(AffJob) * batch + sizeof(void *) * batch);
    for (int b = 0; b < batch; ++b) {
        AffJob &j = jobs[b];
        j.edge = edge_dev + (long)b * hp * wp;
        j.out = nullptr;
        j.gh = hp; j.gw = wp; j.oy = 0; j.ox = rf; j.sh = sh; j.sw = sw;
        j.plane_stride = ns;
        gas[b] = grad_aff_dev + (long)b * tab->n_dirs * ns;
        ges[b] = grad_edge_dev + (long)b * hp * wp;
    }
    char *dev = nullptr;
    rc = scratch_upload(host.data(), host.size(), (void **)&dev, stream);
    if (rc) return rc;
    IRN_HIP_TRY(hipMemsetAsync(grad_edge_dev, 0, sizeof(float) * (size_t)batch * hp * wp, stream));
    const int tiles = cdiv(sh, AFF_TH) * cdiv(sw, AFF_TW);
    const size_t lds = 2 * sizeof(float) * (AFF_TH + rf) * (AFF_TW + 2 * rf);
    hipLaunchKernelGGL(affinity_backward_kernel, dim3(tiles, batch), dim3(256), lds, stream, (const AffJob *)dev,
                       (const float *const *)(dev + sizeof(AffJob) * batch),
                       (float *const *)(dev + sizeof(AffJob) * batch + sizeof(void *) * batch), tab->dir_start, tab->cell_dy,
                       tab->cell_dx, tab->n_dirs, radius);
    IRN_LAUNCH_CHECK("affinity_backward_kernel");
    return scratch_release(stream);
}

namespace {
// ---------------------------------------------------------------------------------------------
// Pair displacement of the training seam (AffinityDisplacementLoss.to_pair_displacement,
// net/resnet50_irn.py:177-193): out[b,c,d,y,x] = disp[b,c,y,rf+x] - disp[b,c,y+dy_d,rf+x+dx_d] over the
// cropped grid — |S| shifted slices, a stack and a subtraction in the reference; one pass here, exact.
// Backward as a gather (no atomics): the gradient of a cell is the sum over d of what it received as a
// source minus what it received as the destination of the cell at (-dy_d, -dx_d).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pair_disp_kernel(const float *__restrict__ disp, float *__restrict__ out, int hp,
                                                        int wp, int rf, int n_dirs, const int *__restrict__ dir_dy,
                                                        const int *__restrict__ dir_dx) {
    const int ch = hp - rf, cw = wp - 2 * rf;
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= ch * cw) return;
    const int y = s / cw, x = s - y * cw;
    const float *plane = disp + (size_t)blockIdx.y * hp * wp;
    float *o = out + (size_t)blockIdx.y * n_dirs * ch * cw + s;
    const float src = plane[y * wp + rf + x];
    for (int d = 0; d < n_dirs; ++d)
        o[(size_t)d * ch * cw] = src - plane[(y + dir_dy[d]) * wp + rf + x + dir_dx[d]];
}

__global__ __launch_bounds__(256) void pair_disp_backward_kernel(const float *__restrict__ gout, float *__restrict__ gdisp,
                                                                 int hp, int wp, int rf, int n_dirs,
                                                                 const int *__restrict__ dir_dy, const int *__restrict__ dir_dx) {
    const int ch = hp - rf, cw = wp - 2 * rf;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= hp * wp) return;
    const int Y = p / wp, X = p - Y * wp;
    const float *g = gout + (size_t)blockIdx.y * n_dirs * ch * cw;
    const int xs = X - rf;
    float acc = 0.f;
    if (Y < ch && xs >= 0 && xs < cw)
        for (int d = 0; d < n_dirs; ++d) acc += g[(size_t)d * ch * cw + Y * cw + xs];
    for (int d = 0; d < n_dirs; ++d) {
        const int yy = Y - dir_dy[d], xx = xs - dir_dx[d];
        if (yy >= 0 && yy < ch && xx >= 0 && xx < cw) acc -= g[(size_t)d * ch * cw + yy * cw + xx];
    }
    gdisp[(size_t)blockIdx.y * hp * wp + p] = acc;
}

int pair_disp_args(const char *who, const void *a, const void *b, int batch, int channels, int hp, int wp, int radius,
                   const DeviceTable **tab) {
    if (!a || !b || batch < 1 || channels < 1 || radius < 2 || radius > IRN_MAX_RADIUS)
        return fail(IRN_ERR_ARG, "%s: bad argument", who);
    if (hp - (radius - 1) < 1 || wp - 2 * (radius - 1) < 1)
        return fail(IRN_ERR_ARG, "%s: grid %dx%d too small for radius %d", who, hp, wp, radius);
    if ((long)batch * channels > 65535) return fail(IRN_ERR_ARG, "%s: batch * channels must be <= 65535", who);
    return get_device_table(radius, 0, tab);
}
}  // namespace

extern "C" int irn_pair_displacement(const float *disp_dev, int batch, int channels, int hp, int wp, int radius,
                                     float *out_dev, void *stream) {
    const DeviceTable *tab = nullptr;
    if (int rc = pair_disp_args("irn_pair_displacement", disp_dev, out_dev, batch, channels, hp, wp, radius, &tab)) return rc;
    const int rf = radius - 1;
    hipLaunchKernelGGL(pair_disp_kernel, dim3(cdiv((hp - rf) * (wp - 2 * rf), 256), batch * channels), dim3(256), 0,
                       (hipStream_t)stream, disp_dev, out_dev, hp, wp, rf, tab->n_dirs, tab->dir_dy, tab->dir_dx);
    IRN_LAUNCH_CHECK("pair_disp_kernel");
    return IRN_OK;
}

extern "C" int irn_pair_displacement_backward(const float *grad_out_dev, int batch, int channels, int hp, int wp,
                                              int radius, float *grad_disp_dev, void *stream) {
    const DeviceTable *tab = nullptr;
    if (int rc = pair_disp_args("irn_pair_displacement_backward", grad_out_dev, grad_disp_dev, batch, channels, hp, wp,
                                radius, &tab))
        return rc;
    hipLaunchKernelGGL(pair_disp_backward_kernel, dim3(cdiv(hp * wp, 256), batch * channels), dim3(256), 0,
                       (hipStream_t)stream, grad_out_dev, grad_disp_dev, hp, wp, radius - 1, tab->n_dirs, tab->dir_dy,
                       tab->dir_dx);
    IRN_LAUNCH_CHECK("pair_disp_backward_kernel");
    return IRN_OK;
}
