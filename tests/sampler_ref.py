"""Reference for the engine's seeded nucleus sampler (include/mellow_hip.h, mellow_generate_sampled): a numpy Philox4x32-10
and an fp64 sampler that implements the definition literally.  A helper module of the tests, not collected by pytest.

`sample_ref` also returns the MARGINS of a draw -- how far it is from changing under rounding:
  gap   the Gumbel score gap between the winner and the runner-up among the kept tokens (inf with one kept token),
  mass  the distance of the boundary token's exclusive and inclusive nucleus mass from top_p -- inf when every token is kept,
        or when no token whose exclusive mass lies within `mass_tol` of top_p could change the draw by being kept or not.
The kernel computes z + g in fp32 and the nucleus masses in fixed point, so only draws whose margins exceed a small bound are
compared exactly."""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """Philox4x32-10 on arrays of counters (broadcast), key (k0, k1) -> four uint32 arrays"""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in (c0, c1, c2, c3)]
    c = np.broadcast_arrays(*c)
    c0, c1, c2, c3 = [x.copy() for x in c]
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [x.astype(np.uint32) for x in (c0, c1, c2, c3)]


def uniforms(n: int, seed: int, row: int, step: int) -> np.ndarray:
    """u_i, i < n, exactly as the kernel forms them (fp64 holds them exactly)"""
    i = np.arange(n, dtype=np.uint64)
    words = philox4x32_10(i >> np.uint64(2), step, row, 0, seed & MASK, (seed >> 32) & MASK)
    x = np.choose((i & np.uint64(3)).astype(np.int64), words).astype(np.uint64)
    return (2.0 * (x >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24


def scaled(logits_row, temperature: float) -> np.ndarray:
    """z = l / T in fp32 (IEEE division), -0 folded into +0"""
    return (np.asarray(logits_row, dtype=np.float32) / np.float32(temperature)).astype(np.float32) + np.float32(0.0)


def _nucleus(z: np.ndarray, top_p: float):
    """fp64 nucleus rule -> (kept mask, exclusive mass of every token, boundary margin), original token order"""
    zd = z.astype(np.float64)
    n = zd.shape[0]
    order = np.lexsort((np.arange(n), -zd))          # z desc, index asc
    p = np.exp(zd - zd.max())
    p /= p.sum()
    ps = p[order]
    incl = np.cumsum(ps)
    excl_s = incl - ps
    excl_s[0] = 0.0                                  # (exactly 0 in any arithmetic: the first token is always kept)
    keep_sorted = excl_s <= top_p if top_p < 1.0 else np.ones(n, dtype=bool)
    kept = np.zeros(n, dtype=bool)
    kept[order] = keep_sorted
    excl = np.empty(n)
    excl[order] = excl_s
    if keep_sorted.all():
        margin = np.inf if top_p >= 1.0 else float(top_p - excl_s[-1])
    else:
        b = int(np.nonzero(keep_sorted)[0][-1])          # the kept set is a prefix of the order
        margin = float(abs(incl[b] - top_p)) if b == 0 else float(min(abs(top_p - excl_s[b]), abs(incl[b] - top_p)))
    return kept, excl, margin


def nucleus_mask(z: np.ndarray, top_p: float):
    """kept mask of the fp64 nucleus rule + the boundary token's mass margin"""
    kept, _, margin = _nucleus(z, top_p)
    return kept, margin


def sample_ref(logits_row, top_p: float, temperature: float, seed: int, row: int, step: int, mass_tol: float = 1e-5):
    """-> (token, gap margin, mass margin) by the definition, in fp64.  The mass margin is the boundary token's distance from
    top_p when moving the boundary by the tokens within mass_tol of it could change the draw, else inf (the draw does not
    depend on which of those tokens are kept)."""
    l = np.asarray(logits_row, dtype=np.float32)
    nan = np.nonzero(np.isnan(l))[0]
    if nan.size:
        return int(nan[0]), np.inf, np.inf
    z = scaled(l, temperature)
    kept, excl, mmass = _nucleus(z, top_p)
    g = -np.log(-np.log(uniforms(z.shape[0], seed, row, step)))
    sc = z.astype(np.float64) + g
    s = np.where(kept, sc, -np.inf)
    tok = int(np.argmax(s))                          # first index among equal maxima
    if kept.sum() > 1:
        top2 = np.sort(s[kept])[-2:]
        gap = float(top2[1] - top2[0])
    else:
        gap = np.inf
    if top_p < 1.0 and np.isfinite(mmass):
        unsure = (np.abs(excl - top_p) <= mass_tol) & (excl > 0.0)
        lo = int(np.argmax(np.where(kept & ~unsure, sc, -np.inf)))
        hi = int(np.argmax(np.where(kept | unsure, sc, -np.inf)))
        if lo == tok and hi == tok:
            mmass = np.inf
    return tok, gap, mmass


def nucleus_probs(logits_row, top_p: float, temperature: float) -> np.ndarray:
    """fp64 renormalised nucleus probabilities (what the draws are distributed as)"""
    z = scaled(logits_row, temperature)
    kept, _, _ = _nucleus(z, top_p)
    zd = z.astype(np.float64)
    p = np.where(kept, np.exp(zd - zd.max()), 0.0)
    return p / p.sum()
