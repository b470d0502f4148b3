// Dense CRF with a permutohedral lattice (reference misc/imutils.py:156-170, crf_inference_label, and
// step/cam_to_ir_label.py:26-42): the densecrf numerics that pydensecrf wraps — float32, DIAG_KERNEL,
// NORMALIZE_SYMMETRIC, Potts compatibility — restated in tests/_densecrf_ref.py.
//
// A lattice (Adams et al. 2010, densecrf Permutohedral::init) is built once per image and feature set:
//   points    one thread per pixel: elevate, round, rank, barycentric weights, the d+1 vertex keys
//   sort      (packed key, entry) pairs by rocPRIM radix sort; the sort is stable, so the entries of one vertex stay in
//             (pixel, vertex-of-simplex) order, the order densecrf splats in
//   unique    head flags + an integer scan number the vertices in ascending key order; the sorted entry list IS the
//             vertex -> (pixel, weight) CSR that splat reduces over in a fixed order
//   neighbours binary search of the two blur neighbours along each of the d+1 axes
// The filter (Permutohedral::compute) is then splat (gather over the CSR), d+1 blur passes (ping-pong) and slice.
// Nothing accumulates through atomics: every result is a fixed-order reduction, bit-reproducible run to run.
// The file is compiled with -ffp-contract=off: the lattice's integer decisions (rounding, ranks) follow float32
// arithmetic op for op, as the restatement does.
#include "common.hpp"

#include <cmath>
#include <rocprim/rocprim.hpp>

using namespace irn;

namespace {

constexpr int TPB = 256;
constexpr int MAX_D = 5;
constexpr int MAX_LABELS = 32;
constexpr int MAX_BLOCKS = 2048;          // grid-stride beyond this (256 CUs x 8)

struct LatParams {
    float scale[MAX_D];
    float down, alpha;
    int bits;                           // bits per packed key component
};

// Bits per component of the packed 64-bit key: component 0 in the highest bits, so ascending packed order is the
// lexicographic order of the (signed) keys, the order np.unique(axis=0) numbers vertices in.
inline int key_bits(int d) { return d * 21 <= 64 ? 21 : 64 / d; }

LatParams lat_params(int d) {
    LatParams p{};
    // densecrf: float inv_std_dev = sqrt(2.0/3.0)*(d+1); scale_factor[i] = 1.0/sqrt(double((i+2)*(i+1)))*inv_std_dev
    const float inv_std_dev = (float)(std::sqrt(2.0 / 3.0) * (d + 1));
    for (int i = 0; i < d; i++) p.scale[i] = (float)(1.0 / std::sqrt((double)((i + 2) * (i + 1))) * inv_std_dev);
    p.down = 1.0f / (float)(d + 1);
    p.alpha = 1.0f / (1.0f + std::pow(2.0f, (float)-d));
    p.bits = key_bits(d);
    return p;
}

// Workspace of one lattice over n points with c channels; every array sized for the worst case M = n*(d+1).
struct Lattice {
    int n = 0, d = 0, e = 0, c = 0;
    uint64_t *key_in, *key_out, *ukey;
    uint32_t *idx_in, *idx_out, *head, *vid;
    uint32_t *vstart;
    int32_t *csr_pix;
    float *csr_w;
    int32_t *offset;
    float *bary;
    int2 *nbr;
    float *val0, *val1;
    float *norm;
    int32_t *meta;                      // [0] = vertices M, [1] = key overflow flag
    void *sort_tmp, *scan_tmp;
    size_t sort_bytes = 0, scan_bytes = 0;
    LatParams prm;
};

struct Carver {
    char *base;
    size_t off = 0;
    explicit Carver(void *b) : base((char *)b) {}
    template <class T> T *take(size_t count) {
        T *p = base ? (T *)(base + off) : nullptr;
        off += round_up(count * sizeof(T) + 1, 256);
        return p;
    }
};

size_t sort_tmp_bytes(int e, int bits_total) {
    size_t b = 0;
    (void)rocprim::radix_sort_pairs(nullptr, b, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                    (uint32_t *)nullptr, (unsigned)e, 0u, (unsigned)bits_total, (hipStream_t)0);
    return b;
}

size_t scan_tmp_bytes(int e) {
    size_t b = 0;
    (void)rocprim::inclusive_scan(nullptr, b, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)e, rocprim::plus<uint32_t>(),
                                  (hipStream_t)0);
    return b;
}

// Lays a lattice out from `cv` (a null base only counts bytes).
void carve(Carver &cv, Lattice &L, int n, int d, int c) {
    L.n = n; L.d = d; L.e = n * (d + 1); L.c = c;
    L.prm = lat_params(d);
    const size_t e = L.e;
    L.key_in = cv.take<uint64_t>(e); L.key_out = cv.take<uint64_t>(e); L.ukey = cv.take<uint64_t>(e);
    L.idx_in = cv.take<uint32_t>(e); L.idx_out = cv.take<uint32_t>(e);
    L.head = cv.take<uint32_t>(e); L.vid = cv.take<uint32_t>(e);
    L.vstart = cv.take<uint32_t>(e + 1);
    L.csr_pix = cv.take<int32_t>(e); L.csr_w = cv.take<float>(e);
    L.offset = cv.take<int32_t>(e); L.bary = cv.take<float>(e);
    L.nbr = cv.take<int2>(e * (d + 1));
    L.val0 = cv.take<float>(e * c); L.val1 = cv.take<float>(e * c);
    L.norm = cv.take<float>(n);
    L.meta = cv.take<int32_t>(4);
    L.sort_bytes = sort_tmp_bytes(L.e, d * L.prm.bits);
    L.scan_bytes = scan_tmp_bytes(L.e);
    L.sort_tmp = cv.take<char>(L.sort_bytes);
    L.scan_tmp = cv.take<char>(L.scan_bytes);
}

inline int grid_for(long work) { return (int)std::max(1L, std::min((long)MAX_BLOCKS, (work + TPB - 1) / TPB)); }

// ---------------------------------------------------------------------------------------------------------------------
// lattice construction
// ---------------------------------------------------------------------------------------------------------------------

__device__ inline bool pack_key(const int *k, int d, int bits, uint64_t &out) {
    const int bias = 1 << (bits - 1);
    uint64_t v = 0;
    for (int i = 0; i < d; i++) {
        const int b = k[i] + bias;
        if (b < 0 || b >= 2 * bias) return false;
        v = (v << bits) | (uint64_t)b;
    }
    out = v;
    return true;
}

template <int D>
__global__ void __launch_bounds__(TPB) k_points(const float *__restrict__ feat, int n, LatParams prm,
                                                uint64_t *__restrict__ key_in, uint32_t *__restrict__ idx_in,
                                                float *__restrict__ bary_out, int32_t *__restrict__ meta) {
    const int p = blockIdx.x * TPB + threadIdx.x;
    if (p >= n) return;
    const float *f = feat + (size_t)p * D;
    float elevated[D + 1], rem0[D + 1], bary[D + 2];
    int rank[D + 1];
    // elevate (y = E p, Adams et al. p.5)
    float sm = 0.0f;
#pragma unroll
    for (int j = D; j > 0; j--) {
        const float cf = f[j - 1] * prm.scale[j - 1];
        elevated[j] = sm - (float)j * cf;
        sm += cf;
    }
    elevated[0] = sm;
    // closest 0-coloured lattice point
    int sum = 0;
#pragma unroll
    for (int i = 0; i <= D; i++) {
        const int rd = (int)roundf(prm.down * elevated[i]);
        rem0[i] = (float)rd * (float)(D + 1);
        sum += rd;
    }
    // ranks of the remainders
#pragma unroll
    for (int i = 0; i <= D; i++) rank[i] = 0;
#pragma unroll
    for (int i = 0; i < D; i++) {
        const float di = elevated[i] - rem0[i];
#pragma unroll
        for (int j = i + 1; j <= D; j++) {
            if (di < elevated[j] - rem0[j]) rank[i]++;
            else rank[j]++;
        }
    }
    // back onto the plane
#pragma unroll
    for (int i = 0; i <= D; i++) {
        rank[i] += sum;
        if (rank[i] < 0) { rank[i] += D + 1; rem0[i] += (float)(D + 1); }
        else if (rank[i] > D) { rank[i] -= D + 1; rem0[i] -= (float)(D + 1); }
    }
    // barycentric weights (p.10)
#pragma unroll
    for (int i = 0; i <= D + 1; i++) bary[i] = 0.0f;
#pragma unroll
    for (int i = 0; i <= D; i++) {
        const float v = (elevated[i] - rem0[i]) * prm.down;
        // rank is a permutation: each slot receives one + and at most one -, so the order of these adds is immaterial
        bary[D - rank[i]] += v;
        bary[D - rank[i] + 1] -= v;
    }
    bary[0] = (float)((double)bary[0] + (1.0 + (double)bary[D + 1]));      // densecrf: barycentric[0] += 1.0 + b[d+1]
    // the d+1 vertices: key[i] = rem0[i] + canonical[remainder][rank[i]]
    bool ok = true;
#pragma unroll
    for (int r = 0; r <= D; r++) {
        int key[D];
#pragma unroll
        for (int i = 0; i < D; i++) key[i] = (int)rem0[i] + (rank[i] <= D - r ? r : r - (D + 1));
        uint64_t packed = 0;
        ok = pack_key(key, D, prm.bits, packed) && ok;
        const size_t e = (size_t)p * (D + 1) + r;
        key_in[e] = packed;
        idx_in[e] = (uint32_t)e;
        bary_out[e] = bary[r];
    }
    if (!ok) meta[1] = 1;               // a key component outside the packed range (same value from every writer)
}

__global__ void __launch_bounds__(TPB) k_heads(const uint64_t *__restrict__ key, int e, uint32_t *__restrict__ head) {
    for (int i = blockIdx.x * TPB + threadIdx.x; i < e; i += gridDim.x * TPB)
        head[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
}

__global__ void __launch_bounds__(TPB) k_vertices(const uint64_t *__restrict__ key, const uint32_t *__restrict__ idx,
                                                  const uint32_t *__restrict__ vid1, const float *__restrict__ bary,
                                                  int e, int dp1, uint64_t *__restrict__ ukey,
                                                  uint32_t *__restrict__ vstart, int32_t *__restrict__ csr_pix,
                                                  float *__restrict__ csr_w, int32_t *__restrict__ offset,
                                                  int32_t *__restrict__ meta) {
    for (int i = blockIdx.x * TPB + threadIdx.x; i < e; i += gridDim.x * TPB) {
        const int v = (int)vid1[i] - 1;
        const uint32_t en = idx[i];
        offset[en] = v;
        csr_pix[i] = (int32_t)(en / dp1);
        csr_w[i] = bary[en];
        if (i == 0 || key[i] != key[i - 1]) {
            vstart[v] = (uint32_t)i;
            ukey[v] = key[i];
        }
        if (i == e - 1) {
            vstart[v + 1] = (uint32_t)e;
            meta[0] = v + 1;
        }
    }
}

__device__ inline int find_key(const uint64_t *__restrict__ ukey, int m, uint64_t k) {
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ukey[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return (lo < m && ukey[lo] == k) ? lo : -1;
}

template <int D>
__global__ void __launch_bounds__(TPB) k_neighbours(const uint64_t *__restrict__ ukey, const int32_t *__restrict__ meta,
                                                    int stride, int bits, int2 *__restrict__ nbr) {
    const int m = meta[0];
    const int bias = 1 << (bits - 1);
    const uint64_t mask = (bits >= 64) ? ~0ull : ((1ull << bits) - 1);
    for (int v = blockIdx.x * TPB + threadIdx.x; v < m; v += gridDim.x * TPB) {
        int key[D];
        const uint64_t u = ukey[v];
#pragma unroll
        for (int i = 0; i < D; i++) key[i] = (int)((u >> (bits * (D - 1 - i))) & mask) - bias;
#pragma unroll
        for (int j = 0; j <= D; j++) {
            int k1[D], k2[D];
#pragma unroll
            for (int i = 0; i < D; i++) {
                k1[i] = key[i] - 1;
                k2[i] = key[i] + 1;
            }
            if (j < D) {            // axis d moves only the (implicit) last component
                k1[j] = key[j] + D;
                k2[j] = key[j] - D;
            }
            uint64_t p1, p2;
            const int n1 = pack_key(k1, D, bits, p1) ? find_key(ukey, m, p1) : -1;
            const int n2 = pack_key(k2, D, bits, p2) ? find_key(ukey, m, p2) : -1;
            nbr[(size_t)j * stride + v] = make_int2(n1, n2);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// filter: splat / blur / slice over c channels, values [vertex][channel]
// ---------------------------------------------------------------------------------------------------------------------

// values[v][ch] = sum over the vertex's CSR entries, in (pixel, r) order, of w * (in[pixel][ch] * norm[pixel]);
// in == nullptr splats ones (the normalisation pass)
__global__ void __launch_bounds__(TPB) k_splat(const float *__restrict__ in, const float *__restrict__ norm, int c,
                                               const uint32_t *__restrict__ vstart, const int32_t *__restrict__ csr_pix,
                                               const float *__restrict__ csr_w, const int32_t *__restrict__ meta,
                                               float *__restrict__ val) {
    const long total = (long)meta[0] * c;
    for (long t = (long)blockIdx.x * TPB + threadIdx.x; t < total; t += (long)gridDim.x * TPB) {
        const int v = (int)(t / c), ch = (int)(t - (long)v * c);
        const uint32_t b = vstart[v], e = vstart[v + 1];
        float s = 0.0f;
        for (uint32_t i = b; i < e; i++) {
            const int p = csr_pix[i];
            float x = in ? in[(size_t)p * c + ch] : 1.0f;
            if (norm) x = x * norm[p];
            s += csr_w[i] * x;
        }
        val[t] = s;
    }
}

__global__ void __launch_bounds__(TPB) k_blur(const float *__restrict__ src, const int2 *__restrict__ nbr, int c,
                                              const int32_t *__restrict__ meta, float *__restrict__ dst) {
    const long total = (long)meta[0] * c;
    for (long t = (long)blockIdx.x * TPB + threadIdx.x; t < total; t += (long)gridDim.x * TPB) {
        const int v = (int)(t / c), ch = (int)(t - (long)v * c);
        const int2 nb = nbr[v];
        const float a = nb.x >= 0 ? src[(size_t)nb.x * c + ch] : 0.0f;
        const float b = nb.y >= 0 ? src[(size_t)nb.y * c + ch] : 0.0f;
        dst[t] = src[t] + 0.5f * (a + b);
    }
}

// splat + d+1 blur passes; returns the buffer that holds the blurred values
float *splat_blur(const Lattice &L, const float *in, const float *norm, int c, hipStream_t s) {
    const int g = grid_for((long)L.e * c);
    k_splat<<<g, TPB, 0, s>>>(in, norm, c, L.vstart, L.csr_pix, L.csr_w, L.meta, L.val0);
    float *a = L.val0, *b = L.val1;
    for (int j = 0; j <= L.d; j++) {
        k_blur<<<g, TPB, 0, s>>>(a, L.nbr + (size_t)j * L.e, c, L.meta, b);
        std::swap(a, b);
    }
    return a;
}

__global__ void __launch_bounds__(TPB) k_slice(const float *__restrict__ val, const int32_t *__restrict__ offset,
                                               const float *__restrict__ bary, int n, int dp1, int c, float alpha,
                                               float *__restrict__ out) {
    const long total = (long)n * c;
    for (long t = (long)blockIdx.x * TPB + threadIdx.x; t < total; t += (long)gridDim.x * TPB) {
        const int p = (int)(t / c), ch = (int)(t - (long)p * c);
        float s = 0.0f;
        for (int r = 0; r < dp1; r++) {
            const size_t e = (size_t)p * dp1 + r;
            s += bary[e] * val[(size_t)offset[e] * c + ch] * alpha;
        }
        out[t] = s;
    }
}

// norm = 1 / sqrt(compute(ones) + 1e-20)   (densecrf DenseKernel::initLattice, NORMALIZE_SYMMETRIC)
__global__ void __launch_bounds__(TPB) k_norm(const float *__restrict__ val, const int32_t *__restrict__ offset,
                                              const float *__restrict__ bary, int n, int dp1, float alpha,
                                              float *__restrict__ norm) {
    for (int p = blockIdx.x * TPB + threadIdx.x; p < n; p += gridDim.x * TPB) {
        float s = 0.0f;
        for (int r = 0; r < dp1; r++) {
            const size_t e = (size_t)p * dp1 + r;
            s += bary[e] * val[offset[e]] * alpha;
        }
        norm[p] = (float)(1.0 / sqrt((double)s + 1e-20));
    }
}

template <int D>
int build_lattice_d(Lattice &L, const float *feat, hipStream_t s) {
    IRN_HIP_TRY(hipMemsetAsync(L.meta, 0, 4 * sizeof(int32_t), s));
    k_points<D><<<cdiv(L.n, TPB), TPB, 0, s>>>(feat, L.n, L.prm, L.key_in, L.idx_in, L.bary, L.meta);
    IRN_LAUNCH_CHECK("k_points");
    size_t sb = L.sort_bytes;
    IRN_HIP_TRY(rocprim::radix_sort_pairs(L.sort_tmp, sb, L.key_in, L.key_out, L.idx_in, L.idx_out, (unsigned)L.e, 0u,
                                          (unsigned)(D * L.prm.bits), s));
    const int g = grid_for(L.e);
    k_heads<<<g, TPB, 0, s>>>(L.key_out, L.e, L.head);
    size_t cb = L.scan_bytes;
    IRN_HIP_TRY(rocprim::inclusive_scan(L.scan_tmp, cb, L.head, L.vid, (size_t)L.e, rocprim::plus<uint32_t>(), s));
    k_vertices<<<g, TPB, 0, s>>>(L.key_out, L.idx_out, L.vid, L.bary, L.e, D + 1, L.ukey, L.vstart, L.csr_pix, L.csr_w,
                                 L.offset, L.meta);
    k_neighbours<D><<<g, TPB, 0, s>>>(L.ukey, L.meta, L.e, L.prm.bits, L.nbr);
    IRN_LAUNCH_CHECK("k_neighbours");
    return IRN_OK;
}

int build_lattice(Lattice &L, const float *feat, hipStream_t s) {
    switch (L.d) {
    case 1: return build_lattice_d<1>(L, feat, s);
    case 2: return build_lattice_d<2>(L, feat, s);
    case 3: return build_lattice_d<3>(L, feat, s);
    case 4: return build_lattice_d<4>(L, feat, s);
    case 5: return build_lattice_d<5>(L, feat, s);
    }
    return fail(IRN_ERR_ARG, "crf: lattice dimension %d outside 1..%d", L.d, MAX_D);
}

int compute_norm(Lattice &L, hipStream_t s) {
    const float *v = splat_blur(L, nullptr, nullptr, 1, s);
    k_norm<<<grid_for(L.n), TPB, 0, s>>>(v, L.offset, L.bary, L.n, L.d + 1, L.prm.alpha, L.norm);
    IRN_LAUNCH_CHECK("k_norm");
    return IRN_OK;
}

// Largest |key component| a feature set bounded by fmax[] can produce (elevation, rounding, wrap, canonical offset):
// the host-side check that the packed key cannot alias for the CRF entries.
bool keys_fit(int d, const double *fmax) {
    const LatParams p = lat_params(d);
    double worst = 0.0;
    for (int j = 0; j <= d; j++) {
        double e = 0.0;
        for (int k = j; k < d; k++) e += fmax[k] * p.scale[k];
        if (j > 0) e += j * fmax[j - 1] * p.scale[j - 1];
        worst = std::max(worst, e);
    }
    return worst + 3.0 * (d + 1) + 2 < (double)(1 << (p.bits - 1));
}

// ---------------------------------------------------------------------------------------------------------------------
// mean field
// ---------------------------------------------------------------------------------------------------------------------

constexpr float GAUSS_SXY = 3.0f, GAUSS_COMPAT = 3.0f;
constexpr float BILAT_SXY = 50.0f, BILAT_SRGB = 5.0f, BILAT_COMPAT = 10.0f;

// features of DenseCRF2D::addPairwiseGaussian / addPairwiseBilateral: (x/3, y/3) and (x/50, y/50, R/5, G/5, B/5)
__global__ void __launch_bounds__(TPB) k_features(const uint8_t *__restrict__ rgb, int h, int w,
                                                  float *__restrict__ fg, float *__restrict__ fb) {
    const int p = blockIdx.x * TPB + threadIdx.x;
    if (p >= h * w) return;
    const int y = p / w, x = p - y * w;
    fg[2 * p + 0] = __fdiv_rn((float)x, GAUSS_SXY);
    fg[2 * p + 1] = __fdiv_rn((float)y, GAUSS_SXY);
    fb[5 * p + 0] = __fdiv_rn((float)x, BILAT_SXY);
    fb[5 * p + 1] = __fdiv_rn((float)y, BILAT_SXY);
    fb[5 * p + 2] = __fdiv_rn((float)rgb[3 * p + 0], BILAT_SRGB);
    fb[5 * p + 3] = __fdiv_rn((float)rgb[3 * p + 1], BILAT_SRGB);
    fb[5 * p + 4] = __fdiv_rn((float)rgb[3 * p + 2], BILAT_SRGB);
}

// thresholds of one launch, by value (the entries take them from the host)
struct Thresholds {
    float v[IRN_CRF_MAX_SWEEP];
};

// step/cam_to_ir_label.py:26-28 / 32-34: argmax over [thr, cam_0 .. cam_{k-1}], the first maximum winning, for each of
// the ncrf thresholds; lab is [crf][pixel]
__global__ void __launch_bounds__(TPB) k_prologue(const float *__restrict__ cams, int k, int n, Thresholds th, int ncrf,
                                                  int32_t *__restrict__ lab) {
    const int p = blockIdx.x * TPB + threadIdx.x;
    if (p >= n) return;
    float best[IRN_CRF_MAX_SWEEP];
    int lb[IRN_CRF_MAX_SWEEP];
#pragma unroll
    for (int i = 0; i < IRN_CRF_MAX_SWEEP; i++) {
        best[i] = th.v[i];
        lb[i] = 0;
    }
    for (int c = 0; c < k; c++) {
        const float v = cams[(size_t)c * n + p];
#pragma unroll
        for (int i = 0; i < IRN_CRF_MAX_SWEEP; i++)
            if (i < ncrf && v > best[i]) { best[i] = v; lb[i] = c + 1; }
    }
#pragma unroll
    for (int i = 0; i < IRN_CRF_MAX_SWEEP; i++)
        if (i < ncrf) lab[(size_t)i * n + p] = lb[i];
}

struct Unary {
    float neg_p, neg_n;                 // -p_energy, -n_energy
};

// softmax over the l labels of a row, as densecrf expAndNormalize: subtract the maximum, exp, multiply by 1/sum
__device__ inline void softmax_row(float (&t)[MAX_LABELS], int l, float *__restrict__ q) {
    float mx = t[0];
#pragma unroll
    for (int i = 1; i < MAX_LABELS; i++)
        if (i < l) mx = fmaxf(mx, t[i]);
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < MAX_LABELS; i++)
        if (i < l) {
            t[i] = expf(t[i] - mx);
            sum += t[i];
        }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int i = 0; i < MAX_LABELS; i++)
        if (i < l) q[i] = t[i] * inv;
}

// Where a mean-field kernel takes -U from.  A source hands out one row per (crf, pixel); row(i, l) is -U of label i.
// SeedUnary: unary_from_labels over lab [crf][pixel] (two values per row).  DenseUnary: the rows k_score_unary wrote,
// fp32 [pixel][crf * l + label].
struct SeedUnary {
    const int32_t *lab;
    Unary u;
    struct Row {
        int lp;
        Unary u;
        __device__ float operator()(int i, int) const { return (i == lp) ? u.neg_p : u.neg_n; }
    };
    __device__ Row row(int n, int, int, int crf, int p) const { return Row{lab[(size_t)crf * n + p], u}; }
};

struct DenseUnary {
    const float *neg_u;
    struct Row {
        const float *r;
        __device__ float operator()(int i, int l) const { return i < l ? r[i] : 0.0f; }
    };
    __device__ Row row(int, int ncrf, int l, int crf, int p) const { return Row{neg_u + ((size_t)p * ncrf + crf) * l}; }
};

// Q = softmax(-U) for every (pixel, crf); Q is [pixel][crf * l + label]
template <class Src>
__global__ void __launch_bounds__(TPB) k_q_init(Src src, int n, int ncrf, int l, float *__restrict__ q) {
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= n * ncrf) return;
    const int crf = t / n, p = t - crf * n;
    const typename Src::Row un = src.row(n, ncrf, l, crf, p);
    float row[MAX_LABELS];
#pragma unroll
    for (int i = 0; i < MAX_LABELS; i++) row[i] = un(i, l);
    softmax_row(row, l, q + (size_t)p * ncrf * l + (size_t)crf * l);
}

// one mean-field update: tmp = -U; tmp -= -3 K_gauss(Q); tmp -= -10 K_bilat(Q); Q = softmax(tmp)
template <int DG, int DB, class Src>
__global__ void __launch_bounds__(TPB) k_update(Src src, int n, int ncrf, int l,
                                                const float *__restrict__ vg, const int32_t *__restrict__ og,
                                                const float *__restrict__ bg, const float *__restrict__ ng, float ag,
                                                const float *__restrict__ vb, const int32_t *__restrict__ ob,
                                                const float *__restrict__ bb, const float *__restrict__ nb, float ab,
                                                float *__restrict__ q) {
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= n * ncrf) return;
    const int crf = t / n, p = t - crf * n;
    const int c = ncrf * l, ch0 = crf * l;
    float kg[MAX_LABELS], kb[MAX_LABELS];
#pragma unroll
    for (int i = 0; i < MAX_LABELS; i++) kg[i] = kb[i] = 0.0f;
#pragma unroll
    for (int r = 0; r <= DG; r++) {
        const size_t e = (size_t)p * (DG + 1) + r;
        const float w = bg[e];
        const float *v = vg + (size_t)og[e] * c + ch0;
#pragma unroll
        for (int i = 0; i < MAX_LABELS; i++)
            if (i < l) kg[i] += w * v[i] * ag;
    }
#pragma unroll
    for (int r = 0; r <= DB; r++) {
        const size_t e = (size_t)p * (DB + 1) + r;
        const float w = bb[e];
        const float *v = vb + (size_t)ob[e] * c + ch0;
#pragma unroll
        for (int i = 0; i < MAX_LABELS; i++)
            if (i < l) kb[i] += w * v[i] * ab;
    }
    const float sg = ng[p], sb = nb[p];
    const typename Src::Row un = src.row(n, ncrf, l, crf, p);
#pragma unroll
    for (int i = 0; i < MAX_LABELS; i++) {
        float x = un(i, l);
        x = x - (-GAUSS_COMPAT * (kg[i] * sg));
        x = x - (-BILAT_COMPAT * (kb[i] * sb));
        kg[i] = x;
    }
    softmax_row(kg, l, q + (size_t)p * c + ch0);
}

constexpr float SCORE_EPS = 1e-5f;     // the clip of pydensecrf's unary_from_softmax (a definition)

// -U of the score-seeded CRFs of one chunk: s_0 = the CRF's threshold, s_i = scores[i-1]; -U_i =
// log(max(s_i, eps)).  A pixel with a NaN score has s' = 1 at its first NaN channel and eps at every other label, the
// background included.  neg_u is [pixel][crf * l + label]; only column 0 differs between the CRFs of a chunk.
__global__ void __launch_bounds__(TPB) k_score_unary(const float *__restrict__ scores, int c, int n, Thresholds th, int ncrf,
                                                     float *__restrict__ neg_u) {
    const int p = blockIdx.x * TPB + threadIdx.x;
    if (p >= n) return;
    const int l = c + 1;
    float *row = neg_u + (size_t)p * ncrf * l;
    int first_nan = -1;
    for (int i = 0; i < c; i++) {
        const float v = scores[(size_t)i * n + p];
        if (v != v && first_nan < 0) first_nan = i;
        const float lg = logf(v != v ? SCORE_EPS : fmaxf(v, SCORE_EPS));
        for (int crf = 0; crf < ncrf; crf++) row[crf * l + 1 + i] = lg;
    }
#pragma unroll
    for (int crf = 0; crf < IRN_CRF_MAX_SWEEP; crf++)
        if (crf < ncrf) row[crf * l] = logf(first_nan >= 0 ? SCORE_EPS : fmaxf(th.v[crf], SCORE_EPS));
    if (first_nan >= 0) {               // the whole row again: eps at every label but the first NaN channel's
        const float le = logf(SCORE_EPS);
        for (int crf = 0; crf < ncrf; crf++)
            for (int i = 0; i < c; i++) row[crf * l + 1 + i] = (i == first_nan) ? 0.0f : le;      // log(1) : log(eps)
    }
}

// -U of the probability-seeded CRF: -U_i = log(max(p_i, eps)), k_score_unary's rule without the threshold
// column: a pixel with a NaN has s' = 1 at its first NaN channel and eps at every other one.  neg_u is [pixel][label].
__global__ void __launch_bounds__(TPB) k_prob_unary(const float *__restrict__ prob, int l, int n, float *__restrict__ neg_u) {
    const int p = blockIdx.x * TPB + threadIdx.x;
    if (p >= n) return;
    float *row = neg_u + (size_t)p * l;
    int first_nan = -1;
    for (int i = 0; i < l; i++) {
        const float v = prob[(size_t)i * n + p];
        if (v != v && first_nan < 0) first_nan = i;
        row[i] = logf(v != v ? SCORE_EPS : fmaxf(v, SCORE_EPS));
    }
    if (first_nan >= 0) {
        const float le = logf(SCORE_EPS);
        for (int i = 0; i < l; i++) row[i] = (i == first_nan) ? 0.0f : le;      // log(1) : log(eps)
    }
}

// Q of every CRF of a chunk as planes: out [crf][label][pixel] (the tests' view of the sweep)
__global__ void __launch_bounds__(TPB) k_q_planes(const float *__restrict__ q, int n, int c, float *__restrict__ out) {
    const long total = (long)n * c;
    for (long t = (long)blockIdx.x * TPB + threadIdx.x; t < total; t += (long)gridDim.x * TPB) {
        const int p = (int)(t / c), ch = (int)(t - (long)p * c);
        out[(size_t)ch * n + p] = q[t];
    }
}

__global__ void __launch_bounds__(TPB) k_fill(float *__restrict__ out, long total, float v) {
    for (long t = (long)blockIdx.x * TPB + threadIdx.x; t < total; t += (long)gridDim.x * TPB) out[t] = v;
}

// argmax of each crf's Q (first maximum), then any of: the labels (+ Q as [label][pixel]) of the first CRF, the
// combination of step/cam_to_ir_label.py:36-39 over the first two (fg, bg), or every CRF's label through the keys as
// one uint8 plane each (planes is [crf][pixel])
__global__ void __launch_bounds__(TPB) k_finish(const float *__restrict__ q, int n, int ncrf, int l,
                                                const int64_t *__restrict__ keys, int32_t *__restrict__ labels,
                                                float *__restrict__ q_out, uint8_t *__restrict__ conf,
                                                uint8_t *__restrict__ planes) {
    const int p = blockIdx.x * TPB + threadIdx.x;
    if (p >= n) return;
    const float *row = q + (size_t)p * ncrf * l;
    long fg = 0, bgc = 0;
    for (int crf = 0; crf < ncrf; crf++) {
        float best = row[crf * l];
        int pred = 0;
        for (int i = 1; i < l; i++)
            if (row[crf * l + i] > best) { best = row[crf * l + i]; pred = i; }
        const long v = (keys && pred) ? keys[pred - 1] + 1 : pred;
        if (crf == 0) fg = v;
        if (crf == 1) bgc = v;
        if (planes) planes[(size_t)crf * n + p] = (uint8_t)v;
    }
    if (labels) labels[p] = (int32_t)fg;
    if (q_out)
        for (int i = 0; i < l; i++) q_out[(size_t)i * n + p] = row[i];
    if (conf) {
        long v = fg;
        if (fg == 0) v = 255;
        if (fg + bgc == 0) v = 0;
        conf[p] = (uint8_t)v;
    }
}

// Everything one image needs, carved from the caller's workspace: seeds for `nseed` CRFs, Q and the lattice values for
// the `ncrf` of them that share a filter pass (c = ncrf * l channels)
struct CrfWs {
    float *feat_g, *feat_b, *q;
    int32_t *lab;
    float *neg_u = nullptr;             // the dense unary of a score-seeded chunk, [pixel][ncrf * l]
    Lattice g, b;
};

size_t carve_crf(void *base, CrfWs &W, int h, int w, int l, int nseed = 2, int ncrf = 2, bool dense = false) {
    Carver cv(base);
    const int n = h * w, c = ncrf * l;
    W.feat_g = cv.take<float>((size_t)n * 2);
    W.feat_b = cv.take<float>((size_t)n * 5);
    W.lab = cv.take<int32_t>((size_t)n * nseed);
    W.q = cv.take<float>((size_t)n * c);
    if (dense) W.neg_u = cv.take<float>((size_t)n * c);
    carve(cv, W.g, n, 2, c);
    carve(cv, W.b, n, 5, c);
    return cv.off;
}

// CRFs of one filter pass of the sweep: never more than 2 * MAX_LABELS channels, what irn_crf_ir_label carries at most
inline int sweep_chunk(int l, int t_count) { return std::min(t_count, std::max(1, 2 * MAX_LABELS / l)); }

bool crf_args_ok(int h, int w, int l, const char *who) {
    if (h < 1 || w < 1 || (long)h * w > (1L << 26) / 6) return fail(IRN_ERR_ARG, "%s: bad image size %dx%d", who, h, w), false;
    if (l < 1 || l > MAX_LABELS) return fail(IRN_ERR_ARG, "%s: n_labels %d outside 1..%d", who, l, MAX_LABELS), false;
    const double fg[2] = {(w - 1) / 3.0, (h - 1) / 3.0};
    const double fb[5] = {(w - 1) / 50.0, (h - 1) / 50.0, 51.0, 51.0, 51.0};
    if (!keys_fit(2, fg) || !keys_fit(5, fb))
        return fail(IRN_ERR_ARG, "%s: image %dx%d too large for the 64-bit lattice keys", who, h, w), false;
    return true;
}

inline Unary unary_of(int l, float gt_prob) {
    const double n_energy = l > 1 ? -std::log((1.0 - gt_prob) / (l - 1)) : 0.0;
    const double p_energy = -std::log((double)gt_prob);
    return Unary{-(float)p_energy, -(float)n_energy};
}

// The mean field in two halves.  An image's pairwise kernels: features, both lattices and their normalisations, once per
// image whatever runs over them (nothing to build without iterations, or with one label: Q = 1 whatever the pairwise terms)
int build_kernels(CrfWs &W, const uint8_t *rgb, int h, int w, int l, int t, hipStream_t s) {
    if (t <= 0 || l == 1) return IRN_OK;
    k_features<<<cdiv(h * w, TPB), TPB, 0, s>>>(rgb, h, w, W.feat_g, W.feat_b);
    IRN_LAUNCH_CHECK("k_features");
    int rc;
    if ((rc = build_lattice(W.g, W.feat_g, s)) || (rc = build_lattice(W.b, W.feat_b, s))) return rc;
    if ((rc = compute_norm(W.g, s)) || (rc = compute_norm(W.b, s))) return rc;
    return IRN_OK;
}

// ... and the iterations of one chunk: ncrf CRFs whose unary comes from `src` (seeds lab [ncrf][n], or the dense rows of
// k_score_unary) as one filter over ncrf * l channels, into W.q.
// A channel's values never meet another's, so a CRF's Q does not depend on which others share its chunk.
template <class Src>
int iterate_chunk(CrfWs &W, Src src, int n, int ncrf, int l, int t, hipStream_t s) {
    const int c = ncrf * l;
    k_q_init<Src><<<cdiv(n * ncrf, TPB), TPB, 0, s>>>(src, n, ncrf, l, W.q);
    IRN_LAUNCH_CHECK("k_q_init");
    if (t <= 0 || l == 1) return IRN_OK;
    for (int it = 0; it < t; it++) {
        const float *vg = splat_blur(W.g, W.q, W.g.norm, c, s);
        const float *vb = splat_blur(W.b, W.q, W.b.norm, c, s);
        k_update<2, 5, Src><<<cdiv(n * ncrf, TPB), TPB, 0, s>>>(src, n, ncrf, l, vg, W.g.offset, W.g.bary, W.g.norm,
                                                                 W.g.prm.alpha, vb, W.b.offset, W.b.bary, W.b.norm,
                                                                 W.b.prm.alpha, W.q);
        IRN_LAUNCH_CHECK("k_update");
    }
    return IRN_OK;
}

inline SeedUnary seeds(const int32_t *lab, int l, float gt_prob) { return SeedUnary{lab, unary_of(l, gt_prob)}; }

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------

extern "C" size_t irn_crf_filter_workspace_bytes(int n, int d, int channels) {
    if (n < 1 || d < 1 || d > MAX_D || channels < 1 || (long)n * (d + 1) > (1L << 26)) return 0;
    Carver cv(nullptr);
    Lattice L;
    carve(cv, L, n, d, channels);
    return cv.off;
}

extern "C" int irn_crf_filter(const float *feat_dev, int n, int d, const float *in_dev, int channels, float *out_dev,
                              int32_t *n_vertices, int32_t *keys_dev, int32_t *nbr_dev, void *ws, size_t ws_bytes,
                              void *stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (!feat_dev || !in_dev || !out_dev || !ws || n < 1 || d < 1 || d > MAX_D || channels < 1)
        return fail(IRN_ERR_ARG, "irn_crf_filter: bad argument");
    const size_t need = irn_crf_filter_workspace_bytes(n, d, channels);
    if (need == 0) return fail(IRN_ERR_ARG, "irn_crf_filter: %d points x %d dims too large", n, d);
    if (ws_bytes < need) return fail(IRN_ERR_STATE, "irn_crf_filter: workspace %zu < %zu bytes", ws_bytes, need);
    Carver cv(ws);
    Lattice L;
    carve(cv, L, n, d, channels);
    int rc = build_lattice(L, feat_dev, s);
    if (rc) return rc;
    int32_t meta[2];
    IRN_HIP_TRY(hipMemcpyAsync(meta, L.meta, sizeof meta, hipMemcpyDeviceToHost, s));
    IRN_HIP_TRY(hipStreamSynchronize(s));
    if (meta[1]) return fail(IRN_ERR_ARG, "irn_crf_filter: a lattice key exceeds %d bits per component", L.prm.bits);
    const int m = meta[0];
    if (n_vertices) *n_vertices = m;
    const float *v = splat_blur(L, in_dev, nullptr, channels, s);
    k_slice<<<grid_for((long)n * channels), TPB, 0, s>>>(v, L.offset, L.bary, n, d + 1, channels, L.prm.alpha, out_dev);
    IRN_LAUNCH_CHECK("k_slice");
    // vertex keys (int32 [M][d], ascending lexicographic) and neighbours (int32 [d+1][M][2]) for inspection
    if (keys_dev || nbr_dev) {
        std::vector<uint64_t> uk(m);
        std::vector<int2> nb((size_t)(d + 1) * m);
        IRN_HIP_TRY(hipMemcpyAsync(uk.data(), L.ukey, m * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        for (int j = 0; j <= d; j++)
            IRN_HIP_TRY(hipMemcpyAsync(nb.data() + (size_t)j * m, L.nbr + (size_t)j * L.e, m * sizeof(int2),
                                       hipMemcpyDeviceToHost, s));
        IRN_HIP_TRY(hipStreamSynchronize(s));
        if (keys_dev) {
            std::vector<int32_t> k((size_t)m * d);
            const int bits = L.prm.bits, bias = 1 << (bits - 1);
            const uint64_t mask = (bits >= 64) ? ~0ull : ((1ull << bits) - 1);
            for (int v2 = 0; v2 < m; v2++)
                for (int i = 0; i < d; i++) k[(size_t)v2 * d + i] = (int)((uk[v2] >> (bits * (d - 1 - i))) & mask) - bias;
            IRN_HIP_TRY(hipMemcpy(keys_dev, k.data(), k.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        if (nbr_dev) IRN_HIP_TRY(hipMemcpy(nbr_dev, nb.data(), nb.size() * sizeof(int2), hipMemcpyHostToDevice));
    }
    return IRN_OK;
}

extern "C" size_t irn_crf_workspace_bytes(int h, int w, int n_labels) {
    if (h < 1 || w < 1 || n_labels < 1 || n_labels > MAX_LABELS || (long)h * w > (1L << 26) / 6) return 0;
    CrfWs W;
    return carve_crf(nullptr, W, h, w, n_labels);
}

extern "C" int irn_crf_inference_label(const uint8_t *rgb_dev, const int32_t *labels_dev, int h, int w, int n_labels,
                                       int t, float gt_prob, float *q_dev, int32_t *labels_out_dev, void *ws,
                                       size_t ws_bytes, void *stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (!rgb_dev || !labels_dev || !labels_out_dev || !ws || t < 0 || !(gt_prob > 0.0f && gt_prob < 1.0f))
        return fail(IRN_ERR_ARG, "irn_crf_inference_label: bad argument");
    if (!crf_args_ok(h, w, n_labels, "irn_crf_inference_label")) return IRN_ERR_ARG;
    const size_t need = irn_crf_workspace_bytes(h, w, n_labels);
    if (ws_bytes < need) return fail(IRN_ERR_STATE, "irn_crf_inference_label: workspace %zu < %zu bytes", ws_bytes, need);
    CrfWs W;
    carve_crf(ws, W, h, w, n_labels);
    const int n = h * w;
    int rc;
    if ((rc = build_kernels(W, rgb_dev, h, w, n_labels, t, s)) ||
        (rc = iterate_chunk(W, seeds(labels_dev, n_labels, gt_prob), n, 1, n_labels, t, s)))
        return rc;
    k_finish<<<cdiv(n, TPB), TPB, 0, s>>>(W.q, n, 1, n_labels, nullptr, labels_out_dev, q_dev, nullptr, nullptr);
    IRN_LAUNCH_CHECK("k_finish");
    return IRN_OK;
}

extern "C" int irn_crf_ir_label(const uint8_t *rgb_dev, const float *high_res_dev, const int64_t *keys_dev, int k, int h,
                                int w, float fg_thres, float bg_thres, int t, float gt_prob, uint8_t *conf_dev, void *ws,
                                size_t ws_bytes, void *stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (!rgb_dev || !conf_dev || k < 0 || (k > 0 && (!high_res_dev || !keys_dev || !ws)) || t < 0 ||
        !(gt_prob > 0.0f && gt_prob < 1.0f) || h < 1 || w < 1)
        return fail(IRN_ERR_ARG, "irn_crf_ir_label: bad argument");
    const int n = h * w, l = k + 1;
    if (k == 0) {                       // no class keys: the reference writes an all-zero map
        IRN_HIP_TRY(hipMemsetAsync(conf_dev, 0, (size_t)n, s));
        return IRN_OK;
    }
    if (!crf_args_ok(h, w, l, "irn_crf_ir_label")) return IRN_ERR_ARG;
    const size_t need = irn_crf_workspace_bytes(h, w, l);
    if (ws_bytes < need) return fail(IRN_ERR_STATE, "irn_crf_ir_label: workspace %zu < %zu bytes", ws_bytes, need);
    CrfWs W;
    carve_crf(ws, W, h, w, l);
    Thresholds th{};
    th.v[0] = fg_thres;
    th.v[1] = bg_thres;
    k_prologue<<<cdiv(n, TPB), TPB, 0, s>>>(high_res_dev, k, n, th, 2, W.lab);
    IRN_LAUNCH_CHECK("k_prologue");
    int rc;
    if ((rc = build_kernels(W, rgb_dev, h, w, l, t, s)) || (rc = iterate_chunk(W, seeds(W.lab, l, gt_prob), n, 2, l, t, s))) return rc;
    k_finish<<<cdiv(n, TPB), TPB, 0, s>>>(W.q, n, 2, l, keys_dev, nullptr, nullptr, conf_dev, nullptr);
    IRN_LAUNCH_CHECK("k_finish");
    return IRN_OK;
}

extern "C" size_t irn_crf_sweep_workspace_bytes(int h, int w, int n_labels, int t_count) {
    if (t_count < 1 || t_count > IRN_CRF_MAX_SWEEP || irn_crf_workspace_bytes(h, w, n_labels) == 0) return 0;
    CrfWs W;
    return carve_crf(nullptr, W, h, w, n_labels, t_count, sweep_chunk(n_labels, t_count));
}

extern "C" int irn_crf_label_sweep(const uint8_t *rgb_dev, const float *high_res_dev, const int64_t *keys_dev, int k, int h,
                                   int w, const float *thres, int t_count, int t, float gt_prob, uint8_t *planes_dev,
                                   void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (t_count < 1 || t_count > IRN_CRF_MAX_SWEEP)
        return fail(IRN_ERR_ARG, "irn_crf_label_sweep: t_count %d outside 1..%d", t_count, IRN_CRF_MAX_SWEEP);
    if (!thres) return fail(IRN_ERR_ARG, "irn_crf_label_sweep: thres is a null pointer");
    Thresholds th{};
    for (int i = 0; i < t_count; i++) {
        if (thres[i] != thres[i]) return fail(IRN_ERR_ARG, "irn_crf_label_sweep: threshold %d is NaN", i);
        if (i > 0 && !(thres[i - 1] < thres[i]))
            return fail(IRN_ERR_ARG, "irn_crf_label_sweep: thresholds not strictly ascending (%g then %g at %d)",
                        (double)thres[i - 1], (double)thres[i], i);
        th.v[i] = thres[i];
    }
    if (k < 0 || t < 0 || !(gt_prob > 0.0f && gt_prob < 1.0f))
        return fail(IRN_ERR_ARG, "irn_crf_label_sweep: bad argument (k=%d, t=%d, gt_prob=%g)", k, t, (double)gt_prob);
    const int l = k + 1;
    if (!crf_args_ok(h, w, l, "irn_crf_label_sweep")) return IRN_ERR_ARG;
    if (!rgb_dev || !planes_dev || (k > 0 && (!high_res_dev || !keys_dev || !ws)))
        return fail(IRN_ERR_ARG, "irn_crf_label_sweep: a null pointer (rgb, planes, or with k > 0 high_res, keys, ws)");
    const int n = h * w;
    if (k == 0) {                       // no class keys: every plane is the all-zero map irn_crf_ir_label writes
        IRN_HIP_TRY(hipMemsetAsync(planes_dev, 0, (size_t)t_count * n, s));
        return IRN_OK;
    }
    const size_t need = irn_crf_sweep_workspace_bytes(h, w, l, t_count);
    if (ws_bytes < need) return fail(IRN_ERR_STATE, "irn_crf_label_sweep: workspace %zu < %zu bytes", ws_bytes, need);
    const int chunk = sweep_chunk(l, t_count);
    CrfWs W;
    carve_crf(ws, W, h, w, l, t_count, chunk);
    k_prologue<<<cdiv(n, TPB), TPB, 0, s>>>(high_res_dev, k, n, th, t_count, W.lab);
    IRN_LAUNCH_CHECK("k_prologue");
    int rc = build_kernels(W, rgb_dev, h, w, l, t, s);
    if (rc) return rc;
    for (int c0 = 0; c0 < t_count; c0 += chunk) {
        const int ncrf = std::min(chunk, t_count - c0);
        const int32_t *lab = W.lab + (size_t)c0 * n;
        if ((rc = iterate_chunk(W, seeds(lab, l, gt_prob), n, ncrf, l, t, s))) return rc;
        k_finish<<<cdiv(n, TPB), TPB, 0, s>>>(W.q, n, ncrf, l, keys_dev, nullptr, nullptr, nullptr,
                                              planes_dev + (size_t)c0 * n);
        IRN_LAUNCH_CHECK("k_finish");
    }
    return IRN_OK;
}

extern "C" size_t irn_crf_score_sweep_workspace_bytes(int h, int w, int n_labels, int t_count) {
    if (t_count < 1 || t_count > IRN_CRF_MAX_SWEEP || irn_crf_workspace_bytes(h, w, n_labels) == 0) return 0;
    CrfWs W;
    return carve_crf(nullptr, W, h, w, n_labels, 0, sweep_chunk(n_labels, t_count), true);
}

extern "C" int irn_crf_score_sweep(const uint8_t *rgb_dev, const float *scores_dev, const int64_t *keys_dev, int c, int h,
                                   int w, const float *thres, int t_count, int t, uint8_t *planes_dev, float *q_dev, void *ws,
                                   size_t ws_bytes, void *stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (t_count < 1 || t_count > IRN_CRF_MAX_SWEEP)
        return fail(IRN_ERR_ARG, "irn_crf_score_sweep: t_count %d outside 1..%d", t_count, IRN_CRF_MAX_SWEEP);
    if (!thres) return fail(IRN_ERR_ARG, "irn_crf_score_sweep: thres is a null pointer");
    Thresholds th{};
    for (int i = 0; i < t_count; i++) {
        if (thres[i] != thres[i]) return fail(IRN_ERR_ARG, "irn_crf_score_sweep: threshold %d is NaN", i);
        if (!(thres[i] >= SCORE_EPS))
            return fail(IRN_ERR_ARG, "irn_crf_score_sweep: threshold %d is %g, below the unary's clip %g", i, (double)thres[i],
                        (double)SCORE_EPS);
        if (i > 0 && !(thres[i - 1] < thres[i]))
            return fail(IRN_ERR_ARG, "irn_crf_score_sweep: thresholds not strictly ascending (%g then %g at %d)",
                        (double)thres[i - 1], (double)thres[i], i);
        th.v[i] = thres[i];
    }
    if (c < 0 || t < 0) return fail(IRN_ERR_ARG, "irn_crf_score_sweep: bad argument (c=%d, t=%d)", c, t);
    const int l = c + 1;
    if (!crf_args_ok(h, w, l, "irn_crf_score_sweep")) return IRN_ERR_ARG;
    if (!rgb_dev || !planes_dev || (c > 0 && (!scores_dev || !keys_dev || !ws)))
        return fail(IRN_ERR_ARG, "irn_crf_score_sweep: a null pointer (rgb, planes, or with c > 0 scores, keys, ws)");
    const int n = h * w;
    if (c == 0) {                       // no class keys: background everywhere, Q = 1
        IRN_HIP_TRY(hipMemsetAsync(planes_dev, 0, (size_t)t_count * n, s));
        if (q_dev) {
            k_fill<<<grid_for((long)t_count * n), TPB, 0, s>>>(q_dev, (long)t_count * n, 1.0f);
            IRN_LAUNCH_CHECK("k_fill");
        }
        return IRN_OK;
    }
    const size_t need = irn_crf_score_sweep_workspace_bytes(h, w, l, t_count);
    if (ws_bytes < need) return fail(IRN_ERR_STATE, "irn_crf_score_sweep: workspace %zu < %zu bytes", ws_bytes, need);
    const int chunk = sweep_chunk(l, t_count);
    CrfWs W;
    carve_crf(ws, W, h, w, l, 0, chunk, true);
    int rc = build_kernels(W, rgb_dev, h, w, l, t, s);
    if (rc) return rc;
    for (int c0 = 0; c0 < t_count; c0 += chunk) {
        const int ncrf = std::min(chunk, t_count - c0);
        Thresholds tc{};
        for (int i = 0; i < ncrf; i++) tc.v[i] = th.v[c0 + i];
        k_score_unary<<<cdiv(n, TPB), TPB, 0, s>>>(scores_dev, c, n, tc, ncrf, W.neg_u);
        IRN_LAUNCH_CHECK("k_score_unary");
        if ((rc = iterate_chunk(W, DenseUnary{W.neg_u}, n, ncrf, l, t, s))) return rc;
        k_finish<<<cdiv(n, TPB), TPB, 0, s>>>(W.q, n, ncrf, l, keys_dev, nullptr, nullptr, nullptr,
                                              planes_dev + (size_t)c0 * n);
        IRN_LAUNCH_CHECK("k_finish");
        if (q_dev) {
            k_q_planes<<<grid_for((long)n * ncrf * l), TPB, 0, s>>>(W.q, n, ncrf * l, q_dev + (size_t)c0 * l * n);
            IRN_LAUNCH_CHECK("k_q_planes");
        }
    }
    return IRN_OK;
}

extern "C" size_t irn_crf_prob_workspace_bytes(int h, int w, int l) {
    if (l < 2 || irn_crf_workspace_bytes(h, w, l) == 0) return 0;
    CrfWs W;
    return carve_crf(nullptr, W, h, w, l, 0, 1, true);
}

extern "C" int irn_crf_prob(const uint8_t *rgb_dev, const float *prob_dev, int l, int h, int w, int t, uint8_t *labels_dev,
                            float *q_dev, void *ws, size_t ws_bytes, void *stream_) {
    hipStream_t s = (hipStream_t)stream_;
    if (l < 2) return fail(IRN_ERR_ARG, "irn_crf_prob: l %d outside 2..%d", l, MAX_LABELS);
    if (t < 0) return fail(IRN_ERR_ARG, "irn_crf_prob: t %d iterations", t);
    if (!crf_args_ok(h, w, l, "irn_crf_prob")) return IRN_ERR_ARG;
    if (!rgb_dev || !prob_dev || !labels_dev || !ws) return fail(IRN_ERR_ARG, "irn_crf_prob: a null pointer (rgb, prob, labels or ws)");
    const size_t need = irn_crf_prob_workspace_bytes(h, w, l);
    if (ws_bytes < need) return fail(IRN_ERR_STATE, "irn_crf_prob: workspace %zu < %zu bytes", ws_bytes, need);
    CrfWs W;
    carve_crf(ws, W, h, w, l, 0, 1, true);
    const int n = h * w;
    int rc = build_kernels(W, rgb_dev, h, w, l, t, s);
    if (rc) return rc;
    k_prob_unary<<<cdiv(n, TPB), TPB, 0, s>>>(prob_dev, l, n, W.neg_u);
    IRN_LAUNCH_CHECK("k_prob_unary");
    if ((rc = iterate_chunk(W, DenseUnary{W.neg_u}, n, 1, l, t, s))) return rc;
    k_finish<<<cdiv(n, TPB), TPB, 0, s>>>(W.q, n, 1, l, nullptr, nullptr, q_dev, nullptr, labels_dev);
    IRN_LAUNCH_CHECK("k_finish");
    return IRN_OK;
}
