"""numpy restatement of the score-seeded dense CRF — the oracle of `ops.crf_score_sweep`.

Everything but the unary is tests/_densecrf_ref.py's: the pairwise kernels (`Kernels`), the mean-field loop of `inference`
and `softmax`.  The unary: the labels are [background, class 1 .. class c] with the scores s = [theta, v_1 .. v_c],
s' = max(s, EPS) and -U = log(s'), so Q0 = softmax(-U) = s' / sum(s').  A pixel with a NaN score has s' = 1 at its first
NaN channel and EPS at every other label, the background included.  The clamp runs in float32 (the scores' own type);
the logarithm and everything behind it in `dtype`."""
import numpy as np

from _densecrf_ref import BILAT_COMPAT, GAUSS_COMPAT, Kernels, softmax

F32 = np.float32
EPS = F32(1e-5)


def clamped_scores(scores, thres):
    """s' float32 [c+1, N] of scores [c,H,W] and one background threshold."""
    thres = F32(thres)
    if not thres >= EPS:
        raise ValueError("the background threshold %r is below the clip %g (or NaN)" % (thres, EPS))
    v = np.asarray(scores, F32)
    c = v.shape[0]
    v = v.reshape(c, -1)
    s = np.concatenate([np.full((1, v.shape[1]), thres, F32), v], 0)
    nan = np.isnan(v)
    s = np.where(np.isnan(s), EPS, np.maximum(s, EPS)).astype(F32)
    bad = nan.any(axis=0)
    if bad.any():
        first = np.argmax(nan, axis=0)[bad]
        s[:, bad] = EPS
        s[first + 1, np.nonzero(bad)[0]] = F32(1.0)
    return s


def neg_unary(scores, thres, dtype=np.float64):
    return np.log(clamped_scores(scores, thres).astype(dtype))


def inference(img, scores, thres, t=10, dtype=np.float64, kernels=None):
    """Q [c+1, N] after t mean-field iterations."""
    neg_u = neg_unary(scores, thres, dtype)
    q = softmax(neg_u)
    if t == 0 or neg_u.shape[0] == 1:
        return q
    k = kernels if kernels is not None else Kernels(img, dtype)
    for _ in range(t):
        tmp = neg_u.copy()
        tmp -= -GAUSS_COMPAT * k.gauss.apply(q.T).T
        tmp -= -BILAT_COMPAT * k.bilat.apply(q.T).T
        q = softmax(tmp)
    return q


def labels_of(q, keys, h, w):
    """The first maximum of Q through the keys: 0 background, keys[i-1] + 1 otherwise; uint8 [H,W]."""
    lut = np.pad(np.asarray(keys, np.int64).reshape(-1) + 1, (1, 0), mode="constant")
    return lut[np.argmax(q, axis=0).reshape(h, w)].astype(np.uint8)


def top2_gap(q):
    """Gap between the two best entries of every column of Q [L, N] (inf with one label)."""
    if q.shape[0] < 2:
        return np.full(q.shape[1], np.inf)
    s = np.sort(q, axis=0)
    return s[-1] - s[-2]


def epilogue_rule(scores, thres, keys):
    """The label epilogue's rule on NaN-free scores: strict > over [theta, v], the first maximum wins; uint8 [H,W]."""
    v = np.asarray(scores, F32)
    c, h, w = v.shape
    stack = np.concatenate([np.full((1, h, w), F32(thres), F32), v], 0)
    lut = np.pad(np.asarray(keys, np.int64).reshape(-1) + 1, (1, 0), mode="constant")
    return lut[np.argmax(stack, axis=0)].astype(np.uint8)
