"""Plain torch / numpy reference for the decode attention launch and the o_proj launch that merges its key splits
(tests/test_dec_attn_ref_cpu.py, tests/test_gpu_dec_attn.py).  Nothing here imports the engine: the float64 definition of the two
launches, the layout codecs (transcribed from the layout COMMENTS of mellow_amd/csrc/dec_common.h / dec_attn.hip / common.h / kernels.h, not from
their code), the merge of decoded partials, the seeded inputs, the case list and the tolerance rule.

The two launches (dec_attn_ref):
    p = sum of the slabs                                   [B][960] = q of 9 heads | k of 3 kv heads | v of 3 kv heads, 64 each
    fused 0: rscale = 1 / sqrt(sum(ssq1) / 576 + eps), x_new given;   fused 1: x_new = x_mid + sum of the down slabs and
    rscale = 1 / sqrt(sum(x_new^2) / 576 + eps)
    RoPE on pairs (i, i + 32) with rope_cur = cos | sin, on the 9 query heads and the 3 keys; q / 8; k, v appended at `pos`
    softmax over the keys 0 .. pos (the cached keys 0 .. pos - 1 of the slot's example and the new one); query head h reads kv
    head h // 3;   x_mid' = x_new + att . Wo^T;   ssq[t] = sum of squares of x_mid' over the columns 16 t .. 16 t + 15

Tolerance of a comparison with float64 (per case, set by the reference alone, never by the kernel under test), the rule of
tests/attn_ref.py:
    tol = max(c * e_ref, 2^-20 * max|v|),   e_ref = largest |float32 evaluation - float64 evaluation| of this reference.
c, derived from the code before any GPU run.  attn_ref's 16 is 8 x 2: 8 for the hardware exp2 after a multiply by log2(e)
(about 8 * 2^-23 relative where libm is within 1 ulp), 2 for the TWO exp factors a softmax weight of the prefill kernels is a
product of (its own exp(s - m) and the rescale of the accumulator once per key tile), summation order included.  A weight of the
decode path is a product of more such factors (mellow_amd/csrc/dec_attn.hip):
    1            p = fast_exp(s - m_new) of its chunk                                  (MELLOW_DA_CHUNK / chunk_mf)
    n - 1        alpha = fast_exp(m_run - m_new), once per LATER chunk of its wave, n = chunks the longest split runs
    1            f = fast_exp(mw - M): the merge of the 8 waves' partials               (dec_attn_kernel, after the barrier)
    1            f_s = fast_exp(m_s - M): the merge of the key splits                  (dec_oproj_kernel; counted at one split too)
so E = n + 2 factors and c = 8 * (n + 2): 24 at one chunk per split, 32 at two, 40 at three (chunks_of below; the case list
never runs more than three).  The same c over the whole chain gives the tolerance of x_mid' and of ssq (e_ref then is the error
of the float32 evaluation of the whole chain, the floor 2^-20 of the largest |x_mid'| / ssq).  The appended k, v have no exp at
all and keep attn_ref's 16.  The o_proj of the kernel's OWN decoded partials (merge + GEMV + residual, own_oproj) has one exp
factor and a 576-term sum: 16 as well.  bf16 pages add no term: the test gives bf16-valued pages, and the kernel uses the new key
and value in fp32.  c is never raised to make a measured case pass: a case above 1.0 is a finding."""
import functools

import numpy as np
import torch

QH, KVH, HD, HID = 9, 3, 64, 576
NPQ_UNFUSED, NPQ_FUSED, N_DOWN = 8, 6, 4       # DEC_KC_QKV, Q2_NPQ, Q2_HC of kernels.h: slabs of the two producers
DA_WAVES, DA_G, DA_GM = 8, 7, 8                # dec_attn.hip: waves, 4-key groups per wave and chunk (vector form / matrix form)
F32, F64 = torch.float32, torch.float64


# ---- the key split ------------------------------------------------------------------------------------------------------------------
def chunk_groups(kv16):
    """4-key groups one workgroup covers per pass: 56 (224 keys) on fp32 pages, 64 (256 keys) on bf16 pages"""
    return DA_WAVES * (DA_GM if kv16 else DA_G)


def split_groups(ctx_end, ts, kv16):
    """gs, the 4-key groups per key split: balanced at the end of the reserved context, rounded down to whole passes of a
    workgroup when that costs at most 4 groups of imbalance (the comment at the engine's rule)"""
    ng_end, chunk = (ctx_end - 1 + 3) // 4, chunk_groups(kv16)
    gs = (ng_end + ts - 1) // ts
    if gs > chunk and gs % chunk <= 4:
        gs -= gs % chunk
    return max(gs, 1)


def split_ranges(pos, gs, ts):
    """cached keys [lo, hi) of every split: split s owns the groups [s gs, (s + 1) gs), the last everything from s gs on (and
    the new key)"""
    return [(min(4 * gs * s, pos), pos if s == ts - 1 else min(4 * gs * (s + 1), pos)) for s in range(ts)]


def chunks_of(pos, gs, ts, kv16):
    """chunks the longest split runs (n of the module docstring): a wave's chunk count is that of the split's first wave"""
    ch = chunk_groups(kv16)
    n = 1
    for s in range(ts):
        g0 = gs * s
        g1 = min((pos + 3) // 4, 10 ** 9 if s == ts - 1 else g0 + gs)
        n = max(n, -(-(g1 - g0) // ch))
    return n


def c_of(case):
    return 8.0 * (chunks_of(case.pos, case.gs, case.ts, case.kv16) + 2)


# ---- the case list ------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, group, B, Tmax, pos, ctx_end, ts, kv16, why):
        self.group, self.B, self.Tmax, self.pos, self.ctx_end, self.ts, self.kv16, self.why = group, B, Tmax, pos, ctx_end, ts, bool(kv16), why
        self.rows = (B + 31) // 32 * 32
        self.RB = self.rows // 32
        self.P = self.rows + 1                       # one example no slot maps to
        self.gs = split_groups(ctx_end, ts, kv16)

    @property
    def id(self):
        return f"{self.group}-B{self.B}-T{self.Tmax}-pos{self.pos}-end{self.ctx_end}-ts{self.ts}-{'bf16' if self.kv16 else 'fp32'}"

    def __repr__(self):
        return f"{self.id} (gs {self.gs}, chunks {chunks_of(self.pos, self.gs, self.ts, self.kv16)}): {self.why}"


def _cases():
    V, M = chunk_groups(False), chunk_groups(True)          # 56, 64
    out = []
    # (a) the first positions, gs = 1 (ctx_end 8 -> 2 groups over 2 splits): seven or eight waves without keys in either split, a
    #     last split without cached keys (pos <= 4: the new key alone), the split boundary at key 4
    for pos, B in ((1, 1), (2, 3), (3, 32), (4, 3), (5, 1)):
        out.append(Case("a", B, 64, pos, 8, 2, False, "first positions at gs = 1: waves without keys, split boundary at key 4"))
    # (b) vector form around one chunk per split: gs = 56 from ctx_end 449 (112 groups / 2)
    assert split_groups(4 * 2 * V + 1, 2, False) == V
    for pos, B in ((4 * V - 1, 3), (4 * V, 1), (4 * V + 1, 32)):
        out.append(Case("b", B, 512, pos, 4 * 2 * V + 1, 2, False, "one chunk per split, pos around 4 gs = 224"))
    #     ... and a ctx_end whose gs = 58 the rounding rule pulls down to 56: the last split runs two chunks, the second partly masked
    assert (4 * 2 * (V + 2) + 1 - 1 + 3) // 4 == 2 * (V + 2) and split_groups(4 * 2 * (V + 2) + 1, 2, False) == V
    out.append(Case("b", 3, 512, 4 * 2 * (V + 2) - 4, 4 * 2 * (V + 2) + 1, 2, False, "gs 58 rounded down to 56: last split two chunks, second partly masked"))
    # (c) two chunks in split 0: gs = 112 (ctx_end 897), pos around 448 = 4 gs; gs = 128 (ctx_end 1024), pos around 4 gs = 512
    assert split_groups(4 * 4 * V + 1, 2, False) == 2 * V and split_groups(1024, 2, False) == 128
    for pos, B in ((8 * V - 1, 1), (8 * V, 3), (8 * V + 1, 3)):
        out.append(Case("c", B, 1024, pos, 4 * 4 * V + 1, 2, False, "two chunks in split 0, pos around 448 = 4 gs"))
    for pos, B in ((511, 3), (513, 1)):
        out.append(Case("c", B, 1024, pos, 1024, 2, False, "gs 128: pos around 4 gs = 512, split 0 runs three chunks"))
    # (d) one split at two row blocks (the f32x3 default), pos around 224 and 448; and the two splits the exact-fp32 mode keeps there
    for pos, B in ((4 * V - 1, 33), (4 * V + 1, 64), (8 * V - 1, 64), (8 * V + 1, 33)):
        out.append(Case("d", B, 512, pos, 512, 1, False, "ts = 1 at two row blocks, pos around 224 / 448"))
    out.append(Case("d", 33, 512, 4 * V + 1, 4 * 2 * V + 1, 2, False, "ts = 2 at two row blocks (exact-fp32 mode), the peeled first chunk"))
    out.append(Case("d", 64, 64, 5, 8, 2, False, "ts = 2 at two row blocks, first positions"))
    # (e) matrix form (bf16 pages): the partly masked first tile, then one chunk per split (gs 65 rounded down to 64) and two
    assert split_groups(64, 2, True) == 8 and split_groups(520, 2, True) == M
    for pos, B in ((31, 1), (32, 3), (33, 32)):
        out.append(Case("e", B, 64, pos, 64, 2, True, "matrix form, pos around one 32-key tile = 4 gs"))
    for pos, B in ((4 * M - 1, 3), (4 * M, 1), (4 * M + 1, 33), (8 * M - 1, 1), (8 * M, 3), (8 * M + 1, 3)):
        out.append(Case("e", B, 520, pos, 520, 2, True, "matrix form, pos around 256 (one chunk per split) / 512 (second chunk partly masked)"))
    out.append(Case("e", 64, 64, 33, 64, 2, True, "matrix form at two row blocks"))
    # (f) the last position of a page, and pages whose length is no multiple of 4: the last group's keys 62, 63 lie past Tmax (the clamp)
    for kv16 in (False, True):
        out.append(Case("f", 3, 64, 63, 64, 2, kv16, "pos = Tmax - 1"))
        out.append(Case("f", 3, 62, 61, 62, 2, kv16, "pos = Tmax - 1, Tmax % 4 = 2: the last key group reaches past Tmax"))
    assert len({c.id for c in out}) == len(out)
    return out


CASES = _cases()
CASE_IDS = [c.id for c in CASES]


def case(cid):
    return CASES[CASE_IDS.index(cid)]


# ---- codecs: element index of (row m, column k) in a raw image -------------------------------------------------------------------------
def _grid(rows, cols=HID):
    return np.arange(rows, dtype=np.int64)[:, None], np.arange(cols, dtype=np.int64)[None, :]


def f16_index(rows):
    """F16-layout (the attention partials of ONE split, x_mid for gate/up): float4 (((rb * 36 + k / 16) * 2 + m % 32 / 16) * 64
    + m % 16 + 16 * (k / 4 % 4)) holds the columns k .. k + 3 of row m of block rb"""
    m, k = _grid(rows)
    return ((((m // 32) * 36 + k // 16) * 2 + (m % 32) // 16) * 64 + m % 16 + 16 * ((k // 4) % 4)) * 4 + k % 4


def f32_index(rows):
    """F32-layout with 72 k-tiles: float4 ((rb * 72 + k / 8) * 64 + m % 32 + 32 * (k / 4 % 2)) holds the columns k .. k + 3"""
    m, k = _grid(rows)
    return (((m // 32) * 72 + k // 8) * 64 + m % 32 + 32 * ((k // 4) % 2)) * 4 + k % 4


def f3_32_index(rows):
    """F3-32, 36 pairs: 16-byte slot ((rb * 36 + T) * 3 + piece) * 64 + lane, lane = m % 32 + 32 h; element e: k = 16 T + 8 h + e.
    -> int64 [3][rows][576] indices of 2-byte elements"""
    m, k = _grid(rows)
    return np.stack([((((m // 32) * 36 + k // 16) * 3 + piece) * 64 + m % 32 + 32 * ((k // 8) % 2)) * 8 + k % 8 for piece in range(3)])


def f3_16_index(rows):
    """F3-16, 18 pairs: slot (((rb * 18 + T) * 2 + mh) * 3 + piece) * 64 + lane, lane = m % 16 + 16 q; k = 32 T + 8 q + e"""
    m, k = _grid(rows)
    return np.stack([(((((m // 32) * 18 + k // 32) * 2 + (m % 32) // 16) * 3 + piece) * 64 + m % 16 + 16 * ((k // 8) % 4)) * 8 + k % 8
                     for piece in range(3)])


def _np(t):
    return t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def f16_decode(raw, rows, n=1):
    """raw f32 [>= n * rows * 576] -> [n][rows][576]"""
    r = _np(raw).reshape(-1)[: n * rows * HID].reshape(n, rows * HID)
    return torch.from_numpy(r[:, f16_index(rows)].copy())


def f16_encode(x):
    n, rows, _ = x.shape
    out = np.empty((n, rows * HID), dtype=np.float32)
    out[:, f16_index(rows)] = _np(x)
    return torch.from_numpy(out.reshape(-1))


def f32_decode(raw, rows, n=1):
    r = _np(raw).reshape(-1)[: n * rows * HID].reshape(n, rows * HID)
    return torch.from_numpy(r[:, f32_index(rows)].copy())


def f32_encode(x):
    n, rows, _ = x.shape
    out = np.empty((n, rows * HID), dtype=np.float32)
    out[:, f32_index(rows)] = _np(x)
    return torch.from_numpy(out.reshape(-1))


def _bf16_to_f64(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def f3_decode(raw_i16, rows, index):
    """a raw F3 image (2-byte words) -> f32 [rows][576]: a triple decodes to the sum of its three bf16 pieces (exact in float64)"""
    u = _np(raw_i16).reshape(-1).view(np.uint16)
    return torch.from_numpy(_bf16_to_f64(u[index(rows)]).sum(axis=0).astype(np.float32))


def f3_encode(x, index):
    """the inverse (CPU tests only): round-to-nearest three-way bf16 split"""
    x = x.contiguous().float()
    rows = x.shape[0]
    hi = x.to(torch.bfloat16)
    r1 = x - hi.float()
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.float()).to(torch.bfloat16)
    out = np.full(rows * HID * 3, 0xFFFF, dtype=np.uint16)
    out[index(rows)] = np.stack([p.view(torch.int16).numpy().view(np.uint16) for p in (hi, mid, lo)])
    return torch.from_numpy(out.view(np.int16).copy())


def ml_decode(raw, rows, ts):
    """att_ml f32 [9 heads][rows][ts][2] -> (m [ts][rows][9], l [ts][rows][9])"""
    a = torch.as_tensor(raw).reshape(QH, rows, ts, 2)
    return a[..., 0].permute(2, 1, 0).contiguous(), a[..., 1].permute(2, 1, 0).contiguous()


def ml_encode(m, l):
    return torch.stack([m, l], dim=-1).permute(2, 1, 0, 3).contiguous()


def bf16_bits(x):
    """round-to-nearest-even bf16 of f32 values, as int16 words"""
    return x.contiguous().float().to(torch.bfloat16).view(torch.int16)


# ---- the merge of decoded partials ---------------------------------------------------------------------------------------------------
def merge(O, m, l, dtype=F64, swap_m=False):
    """att = sum_s f_s O_s / sum_s f_s L_s, f_s = exp(m_s - max m).  O [ts][n][576], m / l [ts][n][9] -> [n][576].
    swap_m: the mutant that hands the first two splits each other's m"""
    ts, n = O.shape[0], O.shape[1]
    O, m, l = O.to(dtype).view(ts, n, QH, HD), m.to(dtype), l.to(dtype)
    if swap_m:
        m = torch.cat([m[1:2], m[0:1], m[2:]])
    f = torch.exp(m - m.max(dim=0, keepdim=True).values)           # an empty split: m = -inf -> f = 0 (the last split is never empty)
    num = (f[..., None] * O).sum(0)
    den = (f * l).sum(0)
    return (num / den[..., None]).reshape(n, HID)


# ---- the float64 definition ----------------------------------------------------------------------------------------------------------
def _rope(x, rope_cur, sign=1.0):
    c, s = rope_cur[:32], rope_cur[32:] * sign
    x1, x2 = x[..., :32], x[..., 32:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def projected(inp, dtype=F64, rope_sign=1.0, scale=0.125, rscale_shift=0, resid_shift=0):
    """-> dict x_new [B][576], q [B][9][64] (RoPE'd, scaled), k / v [B][3][64] (the appended values).  rscale_shift / resid_shift:
    the mutants that take the RMS scale / the residual row of another slot"""
    p = inp["slabs"].to(dtype).sum(0)
    if inp["fused"]:
        x_new = inp["x_mid"].to(dtype) + inp["down"].to(dtype).sum(0)
        ms = (x_new * x_new).sum(1) / HID
    else:
        x_new = inp["x_new"].to(dtype)
        ms = inp["ssq1"].to(dtype).sum(1) / HID
    rscale = 1.0 / torch.sqrt(ms + inp["eps"])
    xs = p * torch.roll(rscale, rscale_shift)[:, None]
    B = p.shape[0]
    rc = inp["rope_cur"].to(dtype)
    q = _rope(xs[:, :QH * HD].view(B, QH, HD), rc, rope_sign) * scale
    k = _rope(xs[:, QH * HD:(QH + KVH) * HD].view(B, KVH, HD), rc, rope_sign)
    v = xs[:, (QH + KVH) * HD:].reshape(B, KVH, HD)
    return {"x_new": torch.roll(x_new, resid_shift, 0), "q": q, "k": k, "v": v}


def _keys(inp, pr, dtype, drop=(), include_next=False, drop_new=False):
    """-> K, V [B][3][n][64] of the keys a slot attends to, and the positions [n] (pos = the new key)"""
    pos, B = inp["pos"], pr["k"].shape[0]
    ros = inp.get("row_of_slot")
    rowsel = torch.arange(B) if ros is None else torch.as_tensor(ros[:B]).long()
    t = [i for i in range(pos) if i not in drop]
    K = inp["K"][rowsel][:, :, t].to(dtype)
    V = inp["V"][rowsel][:, :, t].to(dtype)
    if include_next:                       # the mutant that lets the first position after the context in: a finite key, the page's value
        K = torch.cat([K, 0.5 * inp["K"][rowsel][:, :, pos - 1:pos].to(dtype)], dim=2)
        V = torch.cat([V, inp["V"][rowsel][:, :, pos + 1:pos + 2].to(dtype)], dim=2)
        t = t + [pos + 1]
    if not drop_new:
        K = torch.cat([K, pr["k"][:, :, None]], dim=2)
        V = torch.cat([V, pr["v"][:, :, None]], dim=2)
        t = t + [pos]
    return K, V, t


def dec_attn_ref(inp, dtype=F64, kv_of=None, drop=(), include_next=False, drop_new=False, **proj_mutants):
    """the definition of the module docstring -> dict att [B][576], k / v [B][3][64], x_new, x_mid [B][576] and ssq [B][36] (with Wo)"""
    pr = projected(inp, dtype, **proj_mutants)
    K, V, _ = _keys(inp, pr, dtype, drop, include_next, drop_new)
    kv_of = [h // 3 for h in range(QH)] if kv_of is None else list(kv_of)
    s = torch.einsum("bhd,bhtd->bht", pr["q"], K[:, kv_of])
    att = torch.einsum("bht,bhtd->bhd", torch.softmax(s, dim=-1), V[:, kv_of]).reshape(-1, HID)
    out = {"att": att, "k": pr["k"], "v": pr["v"], "x_new": pr["x_new"]}
    if inp.get("Wo") is not None:
        out.update(oproj_ref(att, pr["x_new"], inp["Wo"], dtype))
    return out


def oproj_ref(att, x_new, Wo, dtype=F64):
    x = x_new.to(dtype) + att.to(dtype) @ Wo.to(dtype).T
    return {"x_mid": x, "ssq": (x * x).view(x.shape[0], HID // 16, 16).sum(-1)}


def split_partials(inp, gs, ts, dtype=F64):
    """the exact partials of every key split: O [ts][B][576], m / l [ts][B][9] (an empty split: m = -inf, l = 0, O = 0)"""
    pr = projected(inp, dtype)
    kv_of = [h // 3 for h in range(QH)]
    B, pos = pr["q"].shape[0], inp["pos"]
    K, V, t = _keys(inp, pr, dtype)
    t = torch.tensor(t)
    O, m, l = torch.zeros(ts, B, QH, HD, dtype=dtype), torch.full((ts, B, QH), float("-inf"), dtype=dtype), torch.zeros(ts, B, QH, dtype=dtype)
    for sp, (lo, hi) in enumerate(split_ranges(pos, gs, ts)):
        sel = (t >= lo) & (t < hi) | ((t == pos) if sp == ts - 1 else torch.zeros_like(t, dtype=torch.bool))
        if not bool(sel.any()):
            continue
        s = torch.einsum("bhd,bhtd->bht", pr["q"], K[:, kv_of][:, :, sel])
        m[sp] = s.max(dim=-1).values
        w = torch.exp(s - m[sp][..., None])
        l[sp] = w.sum(-1)
        O[sp] = torch.einsum("bht,bhtd->bhd", w, V[:, kv_of][:, :, sel])
    return O.reshape(ts, B, HID), m, l


def tolerance(ref64, ref32, vmax, c):
    """(tol, e_ref) of the module docstring"""
    e_ref = float((ref32.double() - ref64).abs().max())
    return max(c * e_ref, 2.0 ** -20 * float(vmax)), e_ref


def miss(got, ref64, tol):
    """largest |error| / tol; NaN or inf anywhere in `got` -> inf"""
    got = torch.as_tensor(got)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float((got.double() - ref64).abs().max()) / tol


# ---- the seeded inputs ---------------------------------------------------------------------------------------------------------------
def _bf16_round(t):
    return t.to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def inputs(cid, fused):
    """The host arrays of a case (shared, read-only).  Rows alternate between nearly uniform and peaked softmaxes (q scale 0.25 /
    1 / 4 by slot % 3, keys N(0, 1)); the RMS scale of a row lies in [0.5, 2] and differs from row to row; row 1 is all zero
    (B >= 3).  Pages: positions < pos N(0, 1); position pos finite junk; positions > pos NaN in K and +-1e30 in V; the pages of
    the pad slots and of the example no slot maps to hold finite values; bf16 cases: every page value rounded to bf16."""
    c = case(cid)
    g = torch.Generator().manual_seed(7919 * CASE_IDS.index(cid) + 31 * int(fused) + 1)
    rn = lambda *shape: torch.randn(*shape, generator=g)      # noqa: E731
    B, P, pos, Tmax = c.B, c.P, c.pos, c.Tmax
    n = NPQ_FUSED if fused else NPQ_UNFUSED
    qscale = torch.tensor([0.25, 1.0, 4.0])[torch.arange(B) % 3]
    rms = 2.0 ** (2.0 * torch.rand(B, generator=g) - 1.0)                 # 1 / rscale of the row, in [0.5, 2]
    slabs = rn(n, B, 960) / n ** 0.5
    slabs[:, :, :QH * HD] *= qscale[None, :, None]
    slabs *= rms[None, :, None]                                            # ... so that the scaled q, k, v have the scales above
    zero = 1 if B >= 3 else None
    inp = {"fused": bool(fused), "pos": pos, "eps": 1e-5, "B": B}
    if fused:
        x = rn(1 + N_DOWN, B, HID)
        x = x / (x.sum(0).pow(2).mean(1).sqrt()[None, :, None]) * rms[None, :, None]       # rms of x_mid + sum of down = rms
        if zero is not None:
            x[:, zero] = 0
        inp["x_mid"], inp["down"] = x[0].contiguous(), x[1:].contiguous()
    else:
        ssq1 = torch.rand(B, 8, generator=g) + 0.5
        ssq1 = ssq1 / ssq1.sum(1, keepdim=True) * (HID * rms * rms)[:, None]
        x_new = rn(B, HID) * rms[:, None]
        if zero is not None:
            ssq1[zero] = 0
            x_new[zero] = 0
        inp["ssq1"], inp["x_new"] = ssq1, x_new
    if zero is not None:
        slabs[:, zero] = 0
    inp["slabs"] = slabs
    # cos | sin of an angle per pair: any rotation will do, the launch takes the row as staged
    ang = torch.rand(32, generator=g) * 6.2831853
    inp["rope_cur"] = torch.cat([torch.cos(ang), torch.sin(ang)]).float()
    K, V = torch.zeros(P, KVH, Tmax, HD), torch.zeros(P, KVH, Tmax, HD)
    K[:B], V[:B] = rn(B, KVH, Tmax, HD), rn(B, KVH, Tmax, HD)
    K[B:], V[B:] = rn(1, KVH, Tmax, HD), rn(1, KVH, Tmax, HD)             # pad slots and the unmapped example: one finite page, repeated
    K[:, :, pos], V[:, :, pos] = 100.0 * rn(P, KVH, HD), 100.0 * rn(P, KVH, HD)
    if pos + 1 < Tmax:
        K[:, :, pos + 1:] = float("nan")
        V[:, :, pos + 1:] = 1e30 * torch.sign(rn(P, KVH, Tmax - pos - 1, HD))
    if c.kv16:
        K, V = _bf16_round(K), _bf16_round(V)
    inp["K"], inp["V"] = K, V
    inp["Wo"] = torch.randn(HID, HID, generator=torch.Generator().manual_seed(4242)) / HID ** 0.5
    return inp


@functools.lru_cache(maxsize=None)
def reference(cid, fused):
    """the float64 reference of a case with its tolerances: dict ref (dec_attn_ref), tol / e_ref per output name, c"""
    c, inp = case(cid), inputs(cid, fused)
    r64, r32 = dec_attn_ref(inp), dec_attn_ref(inp, dtype=F32)
    cc = c_of(c)
    vmax = {"att": float(torch.maximum(inp["V"][:c.B, :, :c.pos].abs().max(), r64["v"].abs().max())), "k": float(r64["k"].abs().max()),
            "v": float(r64["v"].abs().max()), "x_mid": float(r64["x_mid"].abs().max()), "ssq": float(r64["ssq"].abs().max())}
    tol, e_ref = {}, {}
    for name in vmax:
        tol[name], e_ref[name] = tolerance(r64[name], r32[name], vmax[name], cc if name in ("att", "x_mid", "ssq") else 16.0)
    return {"ref": r64, "ref32": r32, "tol": tol, "e_ref": e_ref, "c": cc}


def own_oproj(att_own, x_new, Wo):
    """x_mid' of the kernel's OWN merged partials (float64) and its tolerance: isolates merge + GEMV + residual"""
    r64, r32 = oproj_ref(att_own, x_new, Wo)["x_mid"], oproj_ref(att_own.float(), x_new, Wo, F32)["x_mid"]
    tol, _ = tolerance(r64, r32, float(r64.abs().max()), 16.0)
    return r64, tol


if __name__ == "__main__":
    for c_ in CASES:
        print(c_)
