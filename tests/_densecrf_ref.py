"""numpy restatement of the dense CRF behind reference misc/imutils.py:156-170 (`crf_inference_label` over pydensecrf)
and of step/cam_to_ir_label.py:22-39 — the oracle of irn_amd/csrc/crf.hip.

Written from the densecrf numerics (Krähenbühl & Koltun 2011; permutohedral lattice of Adams, Baek & Davis 2010) as the
issue that introduced the step lists them; pydensecrf itself was not available to compare against.

Lattice geometry (elevation, rounding, ranks, barycentric weights, vertex keys) is ALWAYS computed in float32 op for op,
as densecrf does: its integer decisions are part of the definition, and the GPU reproduces them bit for bit.  The data
path (splat / blur / slice, normalisation, mean field) runs in `dtype`: float64 by default, float32 on request.
"""
import numpy as np

F32 = np.float32

GAUSS_SXY, GAUSS_COMPAT = 3.0, 3.0
BILAT_SXY, BILAT_SRGB, BILAT_COMPAT = 50.0, 5.0, 10.0


# ---------------------------------------------------------------------------------------------------------------------
# unary and softmax
# ---------------------------------------------------------------------------------------------------------------------

def unary_from_labels(labels, n_labels, gt_prob=0.7):
    """pydensecrf.utils.unary_from_labels(labels, n_labels, gt_prob, zero_unsure=False): float32 [n_labels, N]."""
    labels = np.asarray(labels).reshape(-1)
    n_energy = -np.log((1.0 - gt_prob) / (n_labels - 1)) if n_labels > 1 else 0.0      # float64, then cast
    p_energy = -np.log(gt_prob)
    u = np.full((n_labels, labels.size), n_energy, dtype=F32)
    u[labels, np.arange(labels.size)] = p_energy
    return u


def softmax(x):
    """densecrf expAndNormalize over axis 0: subtract the column maximum, exp, multiply by 1/sum."""
    b = np.exp(x - x.max(axis=0, keepdims=True))
    return b * (1 / b.sum(axis=0, keepdims=True))


# ---------------------------------------------------------------------------------------------------------------------
# permutohedral lattice
# ---------------------------------------------------------------------------------------------------------------------

def _round_half_away(v):
    """C round() on float32: halves away from zero (np.round would round them to even)."""
    t = np.trunc(v)
    frac = v - t                                    # exact in float32
    return (t + np.where(np.abs(frac) >= F32(0.5), np.sign(v), F32(0))).astype(np.int64)


def scale_factors(d):
    inv_std_dev = F32(np.sqrt(2.0 / 3.0) * (d + 1))
    return np.array([1.0 / np.sqrt(float((i + 2) * (i + 1))) * float(inv_std_dev) for i in range(d)], F32)


class Lattice:
    """Permutohedral::init over features f [N, d].

    offset [N, d+1]: vertex of each (pixel, remainder); bary [N, d+1] float32 weights; keys [M, d] int64 vertex keys
    (first d components, np.unique order); full_keys [N, d+1, d+1] (all d+1 components); nbr [d+1, M, 2] blur
    neighbours (-1 = none); M."""

    def __init__(self, f):
        f = np.asarray(f, F32)
        n, d = f.shape
        self.n, self.d = n, d
        scale = scale_factors(d)
        # 1. elevate
        elev = np.zeros((n, d + 1), F32)
        sm = np.zeros(n, F32)
        for j in range(d, 0, -1):
            cf = f[:, j - 1] * scale[j - 1]
            elev[:, j] = sm - F32(j) * cf
            sm = sm + cf
        elev[:, 0] = sm
        # 2. closest 0-coloured point
        down = F32(1.0) / F32(d + 1)
        rd = _round_half_away(down * elev)
        rem0 = rd.astype(F32) * F32(d + 1)
        s = rd.sum(axis=1)
        # 3. ranks by pairwise comparison (ties go to the later coordinate)
        tmp = elev - rem0
        rank = np.zeros((n, d + 1), np.int64)
        for i in range(d):
            for j in range(i + 1, d + 1):
                lt = tmp[:, i] < tmp[:, j]
                rank[:, i] += lt
                rank[:, j] += ~lt
        # 4. back onto the plane
        rank += s[:, None]
        lo, hi = rank < 0, rank > d
        rank[lo] += d + 1
        rem0[lo] += F32(d + 1)
        rank[hi] -= d + 1
        rem0[hi] -= F32(d + 1)
        # 5. barycentric weights (each slot gets one + and at most one -: the order of the adds is immaterial)
        bary = np.zeros((n, d + 2), F32)
        rows = np.arange(n)
        v = (elev - rem0) * down
        for i in range(d + 1):
            bary[rows, d - rank[:, i]] += v[:, i]
            bary[rows, d - rank[:, i] + 1] -= v[:, i]
        bary[:, 0] = (bary[:, 0].astype(np.float64) + (1.0 + bary[:, d + 1].astype(np.float64))).astype(F32)
        self.bary = bary[:, :d + 1]
        # 6. vertices: key[i] = rem0[i] + canonical[r][rank[i]]
        r = np.arange(d + 1)[None, :, None]                     # [1, remainder, 1]
        rk = rank[:, None, :]                                   # [N, 1, component]
        canon = np.where(rk <= d - r, r, r - (d + 1))
        self.full_keys = rem0.astype(np.int64)[:, None, :] + canon     # [N, d+1, d+1]
        flat = self.full_keys[:, :, :d].reshape(-1, d)
        self.keys, inv = np.unique(flat, axis=0, return_inverse=True)
        self.offset = inv.reshape(n, d + 1)
        self.m = self.keys.shape[0]
        # 7. blur neighbours along each axis
        lo_k = int(self.keys.min()) - d - 1
        span = int(self.keys.max()) + d + 2 - lo_k
        packed = self._pack(self.keys, lo_k, span)
        self.nbr = np.full((d + 1, self.m, 2), -1, np.int64)
        for j in range(d + 1):
            n1, n2 = self.keys - 1, self.keys + 1
            if j < d:
                n1[:, j] = self.keys[:, j] + d
                n2[:, j] = self.keys[:, j] - d
            for side, nk in enumerate((n1, n2)):
                p = self._pack(nk, lo_k, span)
                pos = np.clip(np.searchsorted(packed, p), 0, self.m - 1)
                self.nbr[j, :, side] = np.where(packed[pos] == p, pos, -1)

    @staticmethod
    def _pack(k, lo, span):
        out = np.zeros(k.shape[0], np.int64)
        for i in range(k.shape[1]):
            out = out * span + (k[:, i] - lo)
        return out

    def compute(self, values, dtype=np.float64, reverse=False):
        """Permutohedral::compute of values [N, C]: splat w*in, d+1 blur passes new = old + 0.5 (n1 + n2), slice
        w * value * alpha.  `reverse` blurs the axes in the opposite order (densecrf's transpose: the adjoint)."""
        values = np.asarray(values, dtype)
        n, c = values.shape
        d = self.d
        w = self.bary.astype(dtype)
        acc = np.zeros((self.m + 1, c), dtype)                  # row m = the missing neighbour (reads 0)
        for ch in range(c):
            acc[:self.m, ch] = np.bincount(self.offset.reshape(-1), weights=(w * values[:, ch:ch + 1]).reshape(-1),
                                           minlength=self.m).astype(dtype)
        for j in (range(d, -1, -1) if reverse else range(d + 1)):
            n1 = self.nbr[j, :, 0]
            n2 = self.nbr[j, :, 1]
            new = acc.copy()
            new[:self.m] = acc[:self.m] + dtype(0.5) * (acc[n1] + acc[n2])      # index -1 = row m = 0
            acc = new
        alpha = dtype(1.0) / (dtype(1.0) + dtype(2.0) ** dtype(-d))
        out = np.zeros((n, c), dtype)
        for r in range(d + 1):
            out += w[:, r:r + 1] * acc[self.offset[:, r]] * alpha
        return out


def random_features(n, d, seed=0, spread=12.0):
    """n points uniform in [0, spread)^d (float32): a few lattice cells per axis, several points per vertex."""
    return (np.random.RandomState(100 * d + n + seed).rand(n, d) * spread).astype(F32)


class DenseKernel:
    """DIAG_KERNEL + NORMALIZE_SYMMETRIC: norm = 1/sqrt(compute(1) + 1e-20), K(Q) = norm * compute(norm * Q)."""

    def __init__(self, f, dtype=np.float64):
        self.lattice = Lattice(f)
        self.dtype = dtype
        ones = np.ones((self.lattice.n, 1), dtype)
        self.norm = (1.0 / np.sqrt(self.lattice.compute(ones, dtype)[:, 0].astype(np.float64) + 1e-20)).astype(dtype)

    def apply(self, q):
        """q [N, C] -> [N, C]."""
        nq = q * self.norm[:, None]
        return self.lattice.compute(nq, self.dtype) * self.norm[:, None]


# ---------------------------------------------------------------------------------------------------------------------
# the CRF
# ---------------------------------------------------------------------------------------------------------------------

def gaussian_features(h, w):
    """DenseCRF2D::addPairwiseGaussian(sxy=3): (x/3, y/3), x = column, y = row (float32)."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([xx.reshape(-1).astype(F32) / F32(GAUSS_SXY), yy.reshape(-1).astype(F32) / F32(GAUSS_SXY)], 1)


def bilateral_features(img):
    """DenseCRF2D::addPairwiseBilateral(sxy=50, srgb=5): (x/50, y/50, R/5, G/5, B/5) (float32)."""
    h, w = img.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    rgb = np.asarray(img).reshape(-1, 3).astype(F32) / F32(BILAT_SRGB)
    return np.concatenate([xx.reshape(-1, 1).astype(F32) / F32(BILAT_SXY), yy.reshape(-1, 1).astype(F32) / F32(BILAT_SXY),
                           rgb], 1)


class Kernels:
    """The two pairwise kernels of one image (shared by every CRF over it)."""

    def __init__(self, img, dtype=np.float64):
        h, w = img.shape[:2]
        self.gauss = DenseKernel(gaussian_features(h, w), dtype)
        self.bilat = DenseKernel(bilateral_features(img), dtype)


def inference(img, labels, t=10, n_labels=21, gt_prob=0.7, dtype=np.float64, kernels=None):
    """Q [n_labels, N] after t mean-field iterations (densecrf DenseCRF::inference, Potts compatibilities)."""
    neg_u = -unary_from_labels(labels, n_labels, gt_prob).astype(dtype)
    q = softmax(neg_u)
    if t == 0 or n_labels == 1:
        return q
    k = kernels if kernels is not None else Kernels(img, dtype)
    for _ in range(t):
        tmp = neg_u.copy()
        tmp -= -GAUSS_COMPAT * k.gauss.apply(q.T).T
        tmp -= -BILAT_COMPAT * k.bilat.apply(q.T).T
        q = softmax(tmp)
    return q


def crf_inference_label(img, labels, t=10, n_labels=21, gt_prob=0.7, dtype=np.float64, kernels=None):
    """misc/imutils.py:156-170: argmax over labels of Q (first maximum), [H, W]."""
    h, w = img.shape[:2]
    q = inference(img, labels, t, n_labels, gt_prob, dtype, kernels)
    return np.argmax(q.reshape(n_labels, h, w), axis=0)


def seed_labels(high_res, thres):
    """argmax of high_res padded with a float32 `thres` plane in front (step/cam_to_ir_label.py:26-27)."""
    cams = np.asarray(high_res, F32)
    return np.argmax(np.pad(cams, ((1, 0), (0, 0), (0, 0)), mode="constant", constant_values=thres), axis=0)


def combine(fg_conf, bg_conf):
    """step/cam_to_ir_label.py:36-39."""
    conf = fg_conf.copy()
    conf[fg_conf == 0] = 255
    conf[bg_conf + fg_conf == 0] = 0
    return conf.astype(np.uint8)


def ir_label(img, high_res, keys, fg_thres=0.30, bg_thres=0.05, t=10, gt_prob=0.7, dtype=np.float64, return_q=False):
    """step/cam_to_ir_label.py:22-39 for one image; with `return_q` also (Q_fg, Q_bg) (None for an image without keys)."""
    keys = np.pad(np.asarray(keys, np.int64) + 1, (1, 0), mode="constant")
    n_labels = keys.shape[0]
    h, w = img.shape[:2]
    if n_labels == 1:
        conf = np.zeros((h, w), np.uint8)
        return (conf, None) if return_q else conf
    kern = Kernels(img, dtype) if t > 0 else None
    fg_seed = seed_labels(high_res, fg_thres)
    bg_seed = seed_labels(high_res, bg_thres)
    q_fg = inference(img, fg_seed, t, n_labels, gt_prob, dtype, kern)
    q_bg = inference(img, bg_seed, t, n_labels, gt_prob, dtype, kern)
    fg = keys[np.argmax(q_fg, axis=0).reshape(h, w)]
    bg = keys[np.argmax(q_bg, axis=0).reshape(h, w)]
    conf = combine(fg, bg)
    return (conf, (q_fg, q_bg)) if return_q else conf
