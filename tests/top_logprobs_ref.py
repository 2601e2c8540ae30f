"""The definition of top log-probs (include/mellow_hip.h, mellow_generate_top_logprobs) in numpy: the order over the fp32 values, the
log-probs in fp64, and the tolerance-aware membership check the GPU tests use against a teacher-forced forward."""
import numpy as np


def logsumexp64(l):
    """log sum exp over the last axis in fp64; -inf entries contribute nothing"""
    x = np.asarray(l, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))[..., 0]


def log_softmax64(l):
    x = np.asarray(l, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return x - logsumexp64(x)[..., None]


def topk_rows(logits, k):
    """-> (ids int32 [B][k], logprob64 float64 [B][k]): the first k tokens of every row in the order (value descending, index
    ascending) over the fp32 values -- a stable lexsort on (-value, index); -0 and +0 compare equal, -inf ranks last -- and
    l - logsumexp64(l) at those tokens (-inf for a banned token)."""
    l = np.asarray(logits, dtype=np.float32)
    if l.ndim == 1:
        l = l[None]
    B, V = l.shape
    k = int(k)
    assert 1 <= k <= V and not np.isnan(l).any()
    idx = np.arange(V)
    ids = np.stack([np.lexsort((idx, -row))[:k] for row in l]).astype(np.int32)
    lp = log_softmax64(l)
    return ids, np.take_along_axis(lp, ids.astype(np.int64), axis=1)


def membership(L, ids, band):
    """The check of recorded alternatives against an independent row of logits L [V] (a teacher-forced forward), whose log-softmax
    values carry an error of up to band / 2 each: with kth = the k-th largest log-softmax value of L,
      (a) every recorded id v has logsoftmax(L)[v] >= kth - band,
      (b) every token above kth + band is recorded.
    No decision is left out.  -> (ok, lowest recorded value - kth, number of tokens within the band of kth)"""
    ls = log_softmax64(np.asarray(L, dtype=np.float32))
    ids = np.asarray(ids, dtype=np.int64)
    k = ids.shape[0]
    kth = np.sort(ls)[::-1][k - 1]
    a = bool((ls[ids] >= kth - band).all())
    must = np.nonzero(ls > kth + band)[0]
    b = bool(np.isin(must, ids).all())
    return a and b and len(set(ids.tolist())) == k, float(ls[ids].min() - kth), int((np.abs(ls - kth) <= band).sum())
