"""Reference for the sampler's candidate filters (include/mellow_hip.h, mellow_generate_filters): top_k, the nucleus inside the
top-k set and min_p, in fp64 and literal to the definition.  Philox, the uniforms and the temperature scaling are those of
tests/sampler_ref.py.  A helper module of the tests, not collected by pytest.

`sample_ref` returns the token and the MARGINS of the draw -- how far it is from changing under rounding:
  gap    the Gumbel score gap between the winner and the runner-up among the kept tokens (inf with one kept token);
  mass   the nucleus boundary token's distance from top_p, as a share of S_T (the mass of the top-k set) -- inf when the nucleus
         keeps all of the set, or when keeping or dropping the tokens whose exclusive share lies within `mass_tol` of top_p does not
         change the draw;
  minp   inf when keeping or dropping the tokens with |exp(z_i - m) - min_p| <= minp_tol * min_p does not change the draw, else the
         smallest such relative distance (<= minp_tol: the draw is unstable under the rounding of exp).
top_k needs no margin: it moves fp32 values only."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_ref as R  # noqa: E402

TWO31 = 2.0 ** 31


def _sets(z: np.ndarray, top_k: int, top_p: float, min_p: float):
    """-> dict of boolean masks in token order (T, nuc, mp) and the per-token numbers the margins need (share, p)"""
    zd = z.astype(np.float64)
    n = zd.shape[0]
    order = np.lexsort((np.arange(n), -zd))          # z desc, index asc
    K = int(top_k)
    in_T = np.zeros(n, dtype=bool)
    in_T[order[:K] if 0 < K < n else order] = True
    p = np.exp(zd - zd.max())                        # exp(z - m): 1 at the maximum
    p[zd == zd.max()] = 1.0
    q = np.rint(p * TWO31)                           # the fixed-point mass (fp64 holds it and every sum of it exactly)
    # nucleus inside T: integer masses, threshold (u64)(top_p * S_T)
    oT = order[in_T[order]]
    qs = q[oT]
    S_T = qs.sum()
    excl_s = np.cumsum(qs) - qs
    nuc = np.zeros(n, dtype=bool)
    share = np.full(n, np.inf)                       # exclusive mass as a share of S_T (tokens of T only)
    if top_p < 1.0:
        thr = np.floor(np.float64(np.float32(top_p)) * S_T) if top_p > 0.0 else 0.0
        nuc[oT] = excl_s <= thr
        share[oT] = excl_s / S_T
        incl_share = np.full(n, np.inf)
        incl_share[oT] = (excl_s + qs) / S_T
    else:
        nuc[oT] = True
        incl_share = None
    qmin = np.rint(np.float64(np.float32(min_p)) * TWO31)
    mp = q >= qmin
    return dict(order=order, T=in_T, nuc=nuc, mp=mp, share=share, incl_share=incl_share, p=p, top=zd == zd.max())


def kept_mask(logits_row, top_k: int, top_p: float, min_p: float, temperature: float) -> np.ndarray:
    """the kept set of the definition (a row without NaN)"""
    s = _sets(R.scaled(logits_row, temperature), top_k, top_p, min_p)
    return s["T"] & s["nuc"] & s["mp"]


def sample_ref(logits_row, top_k: int, top_p: float, min_p: float, temperature: float, seed: int, row: int, step: int,
               mass_tol: float = 1e-5, minp_tol: float = 1e-5):
    """-> (token, gap margin, mass margin, min-p margin) by the definition, in fp64"""
    l = np.asarray(logits_row, dtype=np.float32)
    nan = np.nonzero(np.isnan(l))[0]
    if nan.size:
        return int(nan[0]), np.inf, np.inf, np.inf
    z = R.scaled(l, temperature)
    s = _sets(z, top_k, top_p, min_p)
    T, nuc, mp = s["T"], s["nuc"], s["mp"]
    kept = T & nuc & mp
    g = -np.log(-np.log(R.uniforms(z.shape[0], seed, row, step)))
    sc = z.astype(np.float64) + g

    def draw(mask):
        return int(np.argmax(np.where(mask, sc, -np.inf)))          # first index among equal maxima

    tok = draw(kept)
    if kept.sum() > 1:
        top2 = np.sort(sc[kept])[-2:]
        gap = float(top2[1] - top2[0])
    else:
        gap = np.inf
    # nucleus boundary: the last kept token of T's order, its exclusive / inclusive share against top_p
    mmass = np.inf
    tp = float(np.float32(top_p))
    if top_p < 1.0 and not nuc[T].all():
        kept_nuc = T & nuc
        b = s["order"][kept_nuc[s["order"]]][-1]
        mmass = float(abs(s["incl_share"][b] - tp)) if s["share"][b] == 0.0 else \
            float(min(abs(tp - s["share"][b]), abs(s["incl_share"][b] - tp)))
        unsure = T & (np.abs(s["share"] - tp) <= mass_tol) & (s["share"] > 0.0)
        if draw(T & (nuc & ~unsure) & mp) == tok and draw(T & (nuc | unsure) & mp) == tok:
            mmass = np.inf
    mminp = np.inf
    fp = float(np.float32(min_p))
    if fp > 0.0:
        rel = np.abs(s["p"] - fp) / fp
        unsure = (rel <= minp_tol) & ~s["top"]          # (a token AT the maximum has q = 2^31 exactly)
        if unsure.any() and not (draw(T & nuc & (mp & ~unsure)) == tok and draw(T & nuc & (mp | unsure)) == tok):
            mminp = float(rel[unsure].min())
    return tok, gap, mmass, mminp


def filtered_probs(logits_row, top_k: int, top_p: float, min_p: float, temperature: float) -> np.ndarray:
    """fp64 renormalised probabilities over the kept set (what the draws are distributed as)"""
    z = R.scaled(logits_row, temperature)
    kept = kept_mask(logits_row, top_k, top_p, min_p, temperature)
    zd = z.astype(np.float64)
    p = np.where(kept, np.exp(zd - zd.max()), 0.0)
    return p / p.sum()
