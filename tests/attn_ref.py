"""Plain torch / numpy references for the attention kernels (tests/test_attn_ref_cpu.py, tests/test_gpu_attention.py).  Nothing here
imports the engine: the definitions, the APB slot formula (transcribed from the comment in mellow_amd/csrc/common.h, not from its
code), the seeded inputs both test modules use, and the tolerance rule.

Tolerance of a comparison with float64 (per case, set by the reference alone, never by the kernel under test):
    tol = max(16 * e_ref, 2^-20 * max|v|)
e_ref = largest |float32 evaluation - float64 evaluation| of the reference on the same inputs.  16 = 8 (the kernels take the
hardware exp2 after a multiply by log2(e): about 1e-6 = 8 * 2^-23 relative, where libm is within 1 ulp) x 2 (the online softmax
rescales its accumulator once per key tile and sums in MFMA order).  The floor is the exp2 figure itself: at T = 1 the float32
evaluation is exact."""
import functools

import numpy as np
import torch

QH, KVH, HD = 9, 3, 64          # query heads, kv heads, head dim of the LM
WIN, WHD = 64, 24               # tokens per Swin window, head dim of the encoder


# ---- definitions -------------------------------------------------------------------------------------------------------------------
def causal_gqa_ref(q, k, v, T, qpos0=0, dtype=torch.float64, keep=None, kv_of=None):
    """q [B][T - qpos0][576] (row i = position qpos0 + i), k / v pages [B][3][Tmax][64] -> [B][T - qpos0][576] in `dtype`.
    scores (q / 8) . k over the keys <= the query's position, softmax, . v; query head hq reads kv head hq // 3.
    keep (bool [T - qpos0][T]) replaces the causal rule and kv_of (9 kv head indices) the head map: the mutants of the
    sensitivity test."""
    B, Tq = q.shape[0], T - qpos0
    assert q.shape == (B, Tq, QH * HD) and k.shape[:2] == (B, KVH) and k.shape[3] == HD and k.shape[2] >= T and v.shape == k.shape
    kv_of = [h // 3 for h in range(QH)] if kv_of is None else list(kv_of)
    qq = q.to(dtype).view(B, Tq, QH, HD).permute(0, 2, 1, 3)
    kk = k[:, kv_of, :T].to(dtype)
    vv = v[:, kv_of, :T].to(dtype)
    s = (qq / 8) @ kk.transpose(-1, -2)
    if keep is None:
        keep = torch.arange(T)[None, :] <= (qpos0 + torch.arange(Tq))[:, None]
    s = s.masked_fill(~keep, float("-inf"))
    return (torch.softmax(s, dim=-1) @ vv).permute(0, 2, 1, 3).reshape(B, Tq, QH * HD)


def window_ref(qkv, bias, mask, nW, nH, dtype=torch.float64, use_bias=True, mask_shift=0):
    """qkv [M][3 C] rows in window order (C = 24 nH), bias [nH][64][64], mask [nW][64][64] or None -> [M][C] in `dtype`.
    The reference's order: (q * fp32(24 ** -0.5)) @ k^T, + bias, + mask[window % nW], softmax, @ v.
    use_bias / mask_shift: the mutants of the sensitivity test."""
    M, C = qkv.shape[0], qkv.shape[1] // 3
    assert C == WHD * nH and M % WIN == 0
    nwin = M // WIN
    x = qkv.to(dtype).view(nwin, WIN, 3, nH, WHD).permute(2, 0, 3, 1, 4)
    scale = torch.tensor(24 ** -0.5, dtype=torch.float32).to(dtype)
    s = (x[0] * scale) @ x[1].transpose(-1, -2)
    if use_bias:
        s = s + bias.to(dtype)[None]
    if mask is not None:
        s = s + mask.to(dtype)[(torch.arange(nwin) + mask_shift) % nW][:, None]
    return (torch.softmax(s, dim=-1) @ x[2]).permute(0, 2, 1, 3).reshape(M, C)


def tolerance(ref64, ref32, vmax):
    """(tol, e_ref) of the module docstring"""
    e_ref = float((ref32.double() - ref64).abs().max())
    return max(16.0 * e_ref, 2.0 ** -20 * float(vmax)), e_ref


# ---- APB: an activation matrix [M][K] pre-split in three bf16 pieces, in 16-byte slots of 8 consecutive columns ----------------------
def _apb_slots(Mp, K):
    """slot index of (row m, column octet k8, piece) for every row of the image -> int64 [Mp][K / 8][3]"""
    assert Mp % 128 == 0 and K % 16 == 0
    m = np.arange(Mp, dtype=np.int64)[:, None, None]
    k8 = np.arange(K // 8, dtype=np.int64)[None, :, None]
    piece = np.arange(3, dtype=np.int64)[None, None, :]
    return ((m // 128 * (K // 16) + k8 // 2) * 12 + piece * 4 + (m // 32) % 4) * 64 + m % 32 + 32 * (k8 % 2)


def apb_decode(image_int32, M, K):
    """the raw image (int32 words, roundup(M, 128) rows of 6 bytes per element) -> (x float32 [M][K]: the three pieces of each element
    summed in float64 and cast, unowned bool [slots]: the slots no row < M owns, halves uint16 [slots][8]: the image by slot)"""
    Mp = (M + 127) // 128 * 128
    img = np.ascontiguousarray(np.asarray(image_int32, dtype=np.int32))
    assert img.size * 4 == Mp * K * 6, (img.size, Mp, K)
    halves = img.view(np.uint16).reshape(-1, 8)
    slots = _apb_slots(Mp, K)
    assert np.array_equal(np.sort(slots.reshape(-1)), np.arange(halves.shape[0]))      # every slot has exactly one owner
    f = (halves[slots[:M]].astype(np.uint32) << 16).view(np.float32).astype(np.float64)      # [M][K / 8][3][8]
    x = f.sum(axis=2).reshape(M, K).astype(np.float32)
    unowned = np.ones(halves.shape[0], dtype=bool)
    unowned[slots[:M].reshape(-1)] = False
    return torch.from_numpy(x), unowned, halves


def _bf16_bits(t):
    return t.view(torch.int16).numpy().view(np.uint16)


def apb_encode(x):
    """the inverse (CPU tests only): float32 [M][K] -> int32 image; round-to-nearest three-way bf16 split, unowned slots 0xFF bytes"""
    x = x.contiguous().float()
    M, K = x.shape
    Mp = (M + 127) // 128 * 128
    hi = x.to(torch.bfloat16)
    r1 = x - hi.float()
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.float()).to(torch.bfloat16)
    pieces = np.stack([_bf16_bits(p).reshape(M, K // 8, 8) for p in (hi, mid, lo)], axis=2)      # [M][K / 8][3][8]
    halves = np.full((Mp * K * 6 // 16, 8), 0xFFFF, dtype=np.uint16)
    halves[_apb_slots(Mp, K)[:M]] = pieces
    return torch.from_numpy(halves.reshape(-1).view(np.int32).copy())


# ---- the seeded inputs of the two test modules --------------------------------------------------------------------------------------
PREFILL_SHAPES = [(1, 1, 1), (1, 31, 31), (2, 32, 40), (1, 33, 64), (3, 64, 64), (1, 65, 70), (2, 97, 128), (2, 389, 453)]      # (B, T, Tmax)
PAST_CASES = [(33, 32), (64, 32), (97, 64), (300, 256), (389, 256)]                                                                # (T, qpos0), B = 2
WINDOW_SHAPES = [(1, 4, 0), (3, 4, 0), (8, 4, 4), (2, 8, 2), (2, 32, 2)]                                                         # (windows, nH, nW; 0 = no mask)


def _bf16_round(t):
    return t.to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def prefill_inputs(B, T, Tmax, bf16=False):
    """q [B][T][576] and k / v pages [B][3][Tmax][64] of N(0, 1) values, every (example, kv head) page from a seed of its own (and
    every T from seeds of its own: two shapes share no data); the page positions >= T hold NaN.  bf16: the values rounded to bf16
    (variants 2 and 3)."""
    def draw(seed, *shape):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(10007 * T + seed))
    q = torch.stack([draw(1000 + b, T, QH * HD) for b in range(B)])
    k = torch.full((B, KVH, Tmax, HD), float("nan"))
    v = torch.full((B, KVH, Tmax, HD), float("nan"))
    for b in range(B):
        for g in range(KVH):
            k[b, g, :T] = draw(2000 + 3 * b + g, T, HD)
            v[b, g, :T] = draw(3000 + 3 * b + g, T, HD)
    if bf16:
        q, k, v = _bf16_round(q), _bf16_round(k), _bf16_round(v)
    return q, k, v


@functools.lru_cache(maxsize=None)
def prefill_case(B, T, Tmax, bf16=False):
    """the inputs with their float64 reference and tolerance: dict q, k, v, ref, tol, e_ref, vmax (computed once, shared, read-only)"""
    q, k, v = prefill_inputs(B, T, Tmax, bf16)
    ref = causal_gqa_ref(q, k, v, T)
    vmax = float(v[:, :, :T].abs().max())
    tol, e_ref = tolerance(ref, causal_gqa_ref(q, k, v, T, dtype=torch.float32), vmax)
    return {"q": q, "k": k, "v": v, "ref": ref, "tol": tol, "e_ref": e_ref, "vmax": vmax}


def window_masks(nW):
    """nW mutually different masks of 0 / -100: tokens carry a region label, pairs of different regions are masked (the diagonal never)"""
    out = []
    for w in range(nW):
        lab = torch.randint(0, 3, (WIN,), generator=torch.Generator().manual_seed(500 + w))
        out.append(torch.where(lab[:, None] == lab[None, :], 0.0, -100.0))
    m = torch.stack(out)
    assert all(not torch.equal(m[a], m[b]) for a in range(nW) for b in range(a))
    return m


@functools.lru_cache(maxsize=None)
def window_case(windows, nH, nW, bf16=False):
    """dict qkv [64 windows][72 nH], bias [nH][64][64], mask [nW][64][64] or None (nW = 0), ref, tol, e_ref, vmax"""
    C = WHD * nH
    qkv = torch.randn(windows * WIN, 3 * C, generator=torch.Generator().manual_seed(4000 + windows * 100 + nH))
    if bf16:
        qkv = _bf16_round(qkv)
    bias = torch.randn(nH, WIN, WIN, generator=torch.Generator().manual_seed(4500 + nH))
    mask = window_masks(nW) if nW else None
    ref = window_ref(qkv, bias, mask, nW, nH)
    vmax = float(qkv[:, 2 * C:].abs().max())
    tol, e_ref = tolerance(ref, window_ref(qkv, bias, mask, nW, nH, dtype=torch.float32), vmax)
    return {"qkv": qkv, "bias": bias, "mask": mask, "ref": ref, "tol": tol, "e_ref": e_ref, "vmax": vmax}
