"""numpy restatement of the probability-seeded dense CRF — the oracle of `ops.crf_prob`.

Everything but the unary is tests/_densecrf_ref.py's: the pairwise kernels (`Kernels`), the mean-field loop of `inference`
and `softmax`, the way tests/_score_crf_ref.py builds on them.  The unary: p' = max(p, EPS) and -U = log(p'), so
Q0 = softmax(-U) = p' / sum(p').  A pixel with a NaN has p' = 1 at its first NaN channel and EPS at every other one.  The clamp
runs in float32 (the probabilities' own type); the logarithm and everything behind it in `dtype`."""
import numpy as np

from _densecrf_ref import BILAT_COMPAT, GAUSS_COMPAT, Kernels, softmax

F32 = np.float32
EPS = F32(1e-5)


def clamped(prob):
    """p' float32 [l, N] of prob [l,H,W]."""
    v = np.asarray(prob, F32)
    v = v.reshape(v.shape[0], -1)
    nan = np.isnan(v)
    s = np.where(nan, EPS, np.maximum(v, EPS)).astype(F32)
    bad = nan.any(axis=0)
    if bad.any():
        s[:, bad] = EPS
        s[np.argmax(nan, axis=0)[bad], np.nonzero(bad)[0]] = F32(1.0)
    return s


def inference(img, prob, t=10, dtype=np.float64, kernels=None):
    """Q [l, N] after t mean-field iterations."""
    neg_u = np.log(clamped(prob).astype(dtype))
    q = softmax(neg_u)
    if t == 0:
        return q
    k = kernels if kernels is not None else Kernels(img, dtype)
    for _ in range(t):
        tmp = neg_u.copy()
        tmp -= -GAUSS_COMPAT * k.gauss.apply(q.T).T
        tmp -= -BILAT_COMPAT * k.bilat.apply(q.T).T
        q = softmax(tmp)
    return q


def labels_of(q, h, w):
    """The first maximum of Q, the label index itself; uint8 [H,W]."""
    return np.argmax(q, axis=0).reshape(h, w).astype(np.uint8)


def top2_gap(q):
    s = np.sort(q, axis=0)
    return s[-1] - s[-2]


def random_prob(l, h, w, seed):
    """float32 [l,h,w] probabilities of smooth random logits: a few labels dominate in patches, as a network's do."""
    rng = np.random.RandomState(seed)
    coarse = 3 * rng.standard_normal((l, -(-h // 8) + 1, -(-w // 8) + 1))
    z = np.kron(coarse, np.ones((8, 8)))[:, :h, :w] + 0.5 * rng.standard_normal((l, h, w))
    e = np.exp(z - z.max(0))
    return (e / e.sum(0)).astype(F32)
