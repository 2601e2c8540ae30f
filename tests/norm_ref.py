"""Float64 references for the norm kernels and their APB / MXFP8 hand-over images (tests/test_norm_ref_cpu.py, tests/test_gpu_norm.py).
Nothing here imports the engine: the definitions, the seeded inputs both test modules use, the AMX decoder and encoder, the tolerance
rule and the comparison functions.  The APB decode is the one of tests/attn_ref.py.

Definitions (float64): LayerNorm with the biased variance and eps 1e-5, an optional row map applied as src = (m // ntok) ntok +
map[m % ntok]; patch-merging LayerNorm over the four tokens (2i, 2j), (2i+1, 2j), (2i, 2j+1), (2i+1, 2j+1) of a 2 x 2 patch side by side
in that order; RMSNorm w (x rsqrt(mean x^2 + eps)).

Tolerance, per element, from the reference alone (derived, never measured on the kernel under test); u = 2^-24, any-order summation
bounds, first-order propagation.  LayerNorm with d = x - mu, v = mean d^2, s = (v + eps)^-1/2:
    dmu = (C + 1) u mean|x|                          the mean: C - 1 additions in any order and one division
    dd  = dmu + u |d|                                the subtraction
    dv  = 2 mean(|d| dd) + (C + 3) u v               the squares of perturbed d, then their sum in any order and one division
    rho = dv / (2 (v + eps)) + 3 u                   relative error of s: the addition, the square root, the division
    tol = |w| s (dd + |d| (rho + 3 u)) + 2 u max(|y|, |w d s|)
RMSNorm: tol = |y| ((C + 2) / 2 + 5) u  (the sum of squares within (C + 2) u relative, halved by the square root, plus five roundings).
The any-order bound grows with C while a good summation order does not: at wide rows the rule is loose.  A one-pass variance
(E x^2 - mu^2) misses it by 45 x at C = 96 on these inputs but stays inside at C = 768 (0.09) and C = 1536 (0.03); eps = 1e-6 and the unbiased variance are outside at every
width (tests/test_norm_ref_cpu.py prints the table).  The rule is not to be tightened with anything measured on a kernel.

AMX ("MXFP8"): e4m3 elements, one E8M0 scale byte per 32 columns of a row, in the order of gemm_mx8_kernel's LDS stage (the layout is
transcribed from the comments in mellow_amd/csrc/common.h and gemm_fp8.hip, not from their code).  The engine's rule, which amx_encode
states: E = the smallest exponent with amax / 2^(E - 127) <= 448, clamped to [1, 253]; an all-zero block takes 127; elements are
x 2^(127 - E) converted with torch.float8_e4m3fn (round to nearest even).

An AMX image against float64 (amx_bracket): for the exponent the kernel chose, every decoded element g must satisfy
Q(y - tol) <= g <= Q(y + tol), Q = e4m3 round-to-nearest-even at that scale; rounding is monotone, so the bracket is exact.  The scale
byte must lie in [E(max(|y| - tol)), E(max(|y| + tol))] over the block: the reference exponent, or its neighbour where the amax
straddles 448 2^n within its tolerance.  The share of elements whose bracket is wider than one value and the share of blocks with two
admissible exponents are computed from the reference alone (ambiguity); tests/test_norm_ref_cpu.py caps them at 2 % and 1 % per
(op, C) family, so that the GPU module cannot pass by ambiguity.  One row of each case is ill-conditioned by construction (mean 100,
spread 0.01: dmu alone is several per cent of d), which is why the cap is taken over the family and not over a single 31-row case;
the byte identity with amx_encode of the fp32 output (amx_same) holds such rows exactly.

Inputs are finite: no NaN, no Inf and no fp32 denormal.  Nothing in the repository specifies how the kernels convert those."""
import functools

import numpy as np
import torch

import attn_ref as R
import gemm_ref as G

U = 2.0 ** -24
LN_EPS = 1e-5
miss = G.miss


def rup(x, n):
    return (x + n - 1) // n * n


# ---- float64 definitions -----------------------------------------------------------------------------------------------------------
def src_rows(M, row_map=None, inverted=False):
    """input row of every output row m [M]; inverted: the inverse permutation (the sensitivity test)"""
    m = torch.arange(M)
    if row_map is None:
        return m
    rm = torch.as_tensor(row_map).long()
    ntok = rm.numel()
    assert M % ntok == 0
    if inverted:
        inv = torch.empty_like(rm)
        inv[rm] = torch.arange(ntok)
        rm = inv
    return (m // ntok) * ntok + rm[m % ntok]


def layernorm_ref(x, w, b, row_map=None, mutant=None):
    """-> (y float64 [M][C], tol).  mutant: "eps" (1e-6), "unbiased", "map_inverted"."""
    M, C = x.shape
    xs = x.double()[src_rows(M, row_map, inverted=mutant == "map_inverted")]
    eps = 1e-6 if mutant == "eps" else LN_EPS
    w, b = w.double(), b.double()
    mu = xs.mean(dim=1, keepdim=True)
    d = xs - mu
    v = (d * d).sum(dim=1, keepdim=True) / (C - 1 if mutant == "unbiased" else C)
    s = (v + eps) ** -0.5
    y = d * s * w + b
    dmu = (C + 1) * U * xs.abs().mean(dim=1, keepdim=True)
    dd = dmu + U * d.abs()
    dv = 2 * (d.abs() * dd).mean(dim=1, keepdim=True) + (C + 3) * U * v
    rho = dv / (2 * (v + eps)) + 3 * U
    tol = w.abs() * s * (dd + d.abs() * (rho + 3 * U)) + 2 * U * torch.maximum(y.abs(), (w * d * s).abs())
    return y, tol


def merge_gather(x, n, R, mutant=None):
    """x [n][R R][Cin] -> [n (R / 2)^2][4 Cin]: output row (clip, i, j) = tokens (2i, 2j), (2i+1, 2j), (2i, 2j+1), (2i+1, 2j+1) side by
    side.  mutant "swap12": segments 1 and 2 exchanged."""
    assert x.shape[0] == n and x.shape[1] == R * R and R % 2 == 0
    R2 = R // 2
    i = torch.arange(R2)[:, None].expand(R2, R2).reshape(-1)
    j = torch.arange(R2)[None, :].expand(R2, R2).reshape(-1)
    order = [(0, 0), (1, 0), (0, 1), (1, 1)]
    if mutant == "swap12":
        order = [(0, 0), (0, 1), (1, 0), (1, 1)]
    segs = [x[:, (2 * i + di) * R + 2 * j + dj, :] for di, dj in order]          # each [n][R2 R2][Cin]
    return torch.cat(segs, dim=2).reshape(n * R2 * R2, 4 * x.shape[2])


def merge_layernorm_ref(x, n, R, w, b, mutant=None):
    return layernorm_ref(merge_gather(x, n, R, mutant), w, b)


def rmsnorm_ref(x, w, eps):
    """-> (y float64 [M][C], tol)"""
    C = x.shape[1]
    xd = x.double()
    y = w.double() * (xd * ((xd * xd).mean(dim=1, keepdim=True) + eps) ** -0.5)
    return y, y.abs() * (((C + 2) / 2 + 5) * U)


# ---- AMX ---------------------------------------------------------------------------------------------------------------------------------
def amx_dims(C):
    KT64 = (C + 63) // 64
    return KT64, (KT64 + 3) // 4


@functools.lru_cache(maxsize=None)
def _amx_index(Mp, C, scale_pos_mutant=False):
    """(byte offset of element (m, k) int64 [Mp][rup(C, 64)], byte offset of the scale of (m, block kb) int64 [Mp][2 KT64])"""
    assert Mp % 128 == 0
    KT64, KQ = amx_dims(C)
    m = np.arange(Mp, dtype=np.int64)[:, None]
    k = np.arange(KT64 * 64, dtype=np.int64)[None, :]
    s, j, h = k // 64, (k // 32) % 2, (k // 16) % 2
    slot = ((((m >> 7) * KT64 + s) * 4 + ((m >> 5) & 3)) * 2 + j) * 64 + (m & 31) + 32 * h
    data = slot * 16 + k % 16
    kb = np.arange(2 * KT64, dtype=np.int64)[None, :]
    s, j = kb // 2, kb % 2
    last = s if scale_pos_mutant else (s & 3)
    scale = ((((m >> 7) * KQ + (s >> 2)) * 4 + ((m >> 5) & 3)) * 64 + (m & 31) + 32 * j) * 4 + last
    return data, scale


_E4M3 = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double().numpy()          # 0x7F / 0xFF: NaN


def _u8(t):
    return np.ascontiguousarray(t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.uint8).reshape(-1)


def amx_decode(data_u8, scales_u8, M, C):
    """the raw image and its scale bytes -> (value float32 [M][rup(C, 64)] = e4m3(byte) 2^(E - 127), E uint8 [M][2 KT64], bytes uint8
    [M][rup(C, 64)], data_unowned bool [data bytes]: no row < M owns them, scale_unowned bool [scale bytes]: no (row < M, k64 step <
    KT64) owns them)"""
    KT64, KQ = amx_dims(C)
    Mp = rup(M, 128)
    data, sc = _u8(data_u8), _u8(scales_u8)
    assert data.size == Mp * KT64 * 64 and sc.size == Mp * 8 * KQ, (data.size, sc.size, Mp, C)
    di, si = _amx_index(Mp, C)
    assert np.array_equal(np.sort(di.reshape(-1)), np.arange(data.size))          # every data byte has exactly one owner
    assert np.unique(si.reshape(-1)).size == si.size and si.max() < sc.size
    byt = data[di[:M]]
    E = sc[si[:M]]
    with np.errstate(over="ignore", invalid="ignore"):          # an unwritten scale byte (0xFF) is 2^128
        val = (_E4M3[byt] * np.exp2(np.repeat(E.astype(np.float64), 32, axis=1) - 127.0)).astype(np.float32)
    d_un = np.ones(data.size, dtype=bool)
    d_un[di[:M].reshape(-1)] = False
    s_un = np.ones(sc.size, dtype=bool)
    s_un[si[:M].reshape(-1)] = False
    return torch.from_numpy(val), torch.from_numpy(E.copy()), torch.from_numpy(byt.copy()), d_un, s_un


def mx8_exponent(amax):
    """the rule, exactly: the smallest E with amax / 2^(E - 127) <= 448, clamped to [1, 253]; 127 for amax == 0.  amax: any float
    tensor (frexp is exact: amax = f 2^p with f in [0.5, 1), and 448 = 0.875 2^9)"""
    a = amax.double()
    f, p = torch.frexp(a)
    n = torch.where(f <= 0.875, p - 9, p - 8)
    E = (n + 127).clamp(1, 253)
    return torch.where(a > 0, E, torch.full_like(E, 127)).to(torch.int64)


def mx8_exponent_kernel_f32(amax):
    """what common.h's mx8_exponent computes in fp32: exponent field of amax * fl(1 / 448), plus one where the mantissa is not zero"""
    t = (amax.float() * torch.tensor(1.0 / 448.0, dtype=torch.float32)).contiguous().view(torch.int32).to(torch.int64)
    E = ((t >> 23) & 0xFF) + ((t & 0x7FFFFF) != 0).to(torch.int64)
    return torch.where(amax > 0, E.clamp(1, 253), torch.full_like(E, 127))


def amx_encode(x, pad_rows="ff", mutant=None):
    """the inverse of amx_decode (CPU tests, and the byte identities of the GPU module): float32 [M][C] -> (data uint8, scales uint8).
    Pad columns [C, rup(C, 64)) are zeros (an all-pad block: scale 127).  pad_rows: the rows [M, rup(M, 128)) of the last panel
    are left as 0xFF bytes ("ff": the norm kernels) or written as zeros with scale 127 ("zero": launch_quant_mx8).  Scale bytes of k64
    steps >= KT64 inside a scale word stay 0xFF.  mutant: "exp_plus1", "scale_pos" (byte s instead of s % 4), "pad_nonzero"."""
    x = x.contiguous().float()
    M, C = x.shape
    KT64, KQ = amx_dims(C)
    Mp, K64 = rup(M, 128), KT64 * 64
    rows = Mp if pad_rows == "zero" else M
    xp = torch.zeros(rows, K64, dtype=torch.float32)
    xp[:M, :C] = x
    if mutant == "pad_nonzero":
        xp[:M, C:] = 2.0 ** -3
    blk = xp.view(rows, 2 * KT64, 32)
    E = mx8_exponent(blk.abs().amax(dim=2))
    if mutant == "exp_plus1":
        E = torch.where(blk.abs().amax(dim=2) > 0, E + 1, E)
    inv = torch.exp2((127 - E).double()).float()                                   # a power of two in the fp32 range
    q = (blk * inv[:, :, None]).to(torch.float8_e4m3fn).view(torch.uint8).reshape(rows, K64)
    di, si = _amx_index(Mp, C, scale_pos_mutant=mutant == "scale_pos")
    data = np.full(Mp * K64, 0xFF, dtype=np.uint8)
    sc = np.full(Mp * 8 * KQ, 0xFF, dtype=np.uint8)
    data[di[:rows].reshape(-1)] = q.numpy().reshape(-1)
    sidx = si[:rows].reshape(-1)
    ok = sidx < sc.size                                                           # (the scale_pos mutant may point behind the buffer)
    sc[sidx[ok]] = E.numpy().astype(np.uint8).reshape(-1)[ok]
    return torch.from_numpy(data), torch.from_numpy(sc)


def e4m3_rne(t):
    """float64 -> the nearest e4m3 value (ties to even, saturating at +-448), in float64: one rounding, no detour through fp32"""
    a = t.abs()
    _, p = torch.frexp(a)                                                        # a = f 2^p, f in [0.5, 1): floor(log2 a) = p - 1
    e = (p - 1).clamp(min=-6)                                                     # below 2^-6 the subnormal spacing 2^-9 holds
    step = torch.exp2((e - 3).double())
    q = torch.round(a / step) * step                                             # torch.round: half to even
    return torch.copysign(q.clamp(max=448.0), t)


# ---- comparisons (what the GPU module calls; tests/test_norm_ref_cpu.py shows them catching the mutants) -----------------------------------
def _blocks(t, M, C):
    KT64, _ = amx_dims(C)
    p = torch.zeros(M, KT64 * 64, dtype=torch.float64)
    p[:, :C] = t
    return p.view(M, 2 * KT64, 32)


def exponent_range(y, tol, C):
    """admissible scale exponents of every block from the float64 reference and its tolerance: (lo, hi int64 [M][2 KT64], zero_ok bool:
    the block's amax may be 0 within the tolerance, so 127 -- an all-zero block's exponent by decree -- is admissible as well)"""
    M = y.shape[0]
    ya, tb = _blocks(y.abs(), M, C), _blocks(tol, M, C)
    lo_amax = (ya - tb).clamp(min=0).amax(dim=2)
    hi = mx8_exponent((ya + tb).amax(dim=2))
    lo = torch.where(lo_amax > 0, mx8_exponent(lo_amax), torch.where(hi == 127, hi, torch.ones_like(hi)))
    return torch.minimum(lo, hi), hi, lo_amax == 0


def ambiguity(y, tol, C):
    """(elements whose bracket holds more than one e4m3 value, elements, blocks with two admissible exponents, blocks): from the
    reference alone, at the reference exponent of every block; pad columns and all-pad blocks are not counted"""
    M = y.shape[0]
    yb, tb = _blocks(y, M, C), _blocks(tol, M, C)
    E = mx8_exponent(yb.abs().amax(dim=2))
    sc = torch.exp2((E - 127).double())[:, :, None]
    wide = (e4m3_rne((yb - tb) / sc) != e4m3_rne((yb + tb) / sc)).reshape(M, -1)[:, :C]
    lo, hi, _ = exponent_range(y, tol, C)
    real = (torch.arange(lo.shape[1]) * 32 < C)[None, :].expand_as(lo)
    return int(wide.sum()), M * C, int(((lo != hi) & real).sum()), int(real.sum())


def amx_guards(data_u8, scales_u8, M, C, pad_rows):
    """the guard conventions of an AMX producer -> list of violations (empty: all hold).  pad_rows "ff": rows >= M of the last panel
    are untouched (data and scale bytes 0xFF); "zero": written as zeros, scale 127.  Always: scale bytes of k64 steps >= KT64 stay
    0xFF, pad columns are +0.0 bytes, an all-pad block has scale 127, every owned byte is written and finite."""
    bad = []
    KT64, KQ = amx_dims(C)
    Mp = rup(M, 128)
    _, E, byt, d_un, s_un = amx_decode(data_u8, scales_u8, M, C)
    _, Ep, bytp, _, s_none = amx_decode(data_u8, scales_u8, Mp, C)
    data, sc = _u8(data_u8), _u8(scales_u8)
    if not np.all(sc[s_none] == 0xFF):
        bad.append("a scale byte of a k64 step >= KT64 was written")
    if pad_rows == "ff":
        if not np.all(data[d_un] == 0xFF):
            bad.append("a data byte of a row >= M was written")
        if not np.all(sc[s_un] == 0xFF):
            bad.append("a scale byte of a row >= M was written")
    else:
        if not bool((bytp[M:] == 0).all()):
            bad.append("a row >= M of the last panel is not written as +0.0 bytes")
        if not bool((Ep[M:] == 127).all()):
            bad.append("a row >= M of the last panel has a scale byte other than 127")
    if not bool((byt[:, C:] == 0).all()):
        bad.append("a pad column [C, rup(C, 64)) is not a +0.0 byte")
    full_pad = torch.arange(2 * KT64) * 32 >= C
    if bool(full_pad.any()) and not bool((E[:, full_pad] == 127).all()):
        bad.append("an all-pad block has a scale byte other than 127")
    if bool(((byt[:, :C] & 0x7F) == 0x7F).any()):
        bad.append("an owned data byte was not written (or is a NaN code)")
    if bool((E[:, ~full_pad] == 0xFF).any()):
        bad.append("an owned scale byte was not written")
    return bad


def amx_bracket(data_u8, scales_u8, M, C, y, tol):
    """the image against the float64 reference -> (violations, largest distance outside the bracket in e4m3 steps of the block, share
    of blocks whose exponent is not the reference's own)"""
    bad = []
    val, E, _, _, _ = amx_decode(data_u8, scales_u8, M, C)
    E = E.to(torch.int64)
    lo, hi, zero_ok = exponent_range(y, tol, C)
    n_out = int((((E < lo) | (E > hi)) & ~(zero_ok & (E == 127))).sum())
    if n_out:
        bad.append(f"{n_out} scale bytes outside the admissible exponents of the reference")
    yb, tb = _blocks(y, M, C), _blocks(tol, M, C)
    sc = torch.exp2((E - 127).double())[:, :, None]
    g = val.double().view(M, -1, 32) / sc
    ql, qh = e4m3_rne((yb - tb) / sc), e4m3_rne((yb + tb) / sc)
    out = torch.maximum(ql - g, g - qh).clamp(min=0)
    out = torch.where(torch.isnan(g), torch.full_like(out, float("inf")), out)
    n_el = int((out > 0).sum())
    if n_el:
        bad.append(f"{n_el} elements outside [Q(y - tol), Q(y + tol)], the farthest by {float(out.max()):.4g} (scaled units)")
    E_ref = mx8_exponent(yb.abs().amax(dim=2))
    return bad, float(out.max()), float((E != E_ref).double().mean())


def amx_same(data_u8, scales_u8, x32, pad_rows):
    """the image against amx_encode of fp32 rows, byte for byte -> list of violations"""
    wd, ws = amx_encode(x32, pad_rows)
    d, s = torch.from_numpy(_u8(data_u8).copy()), torch.from_numpy(_u8(scales_u8).copy())
    bad = []
    if d.shape != wd.shape or s.shape != ws.shape:
        return [f"sizes {tuple(d.shape)} / {tuple(s.shape)} are not {tuple(wd.shape)} / {tuple(ws.shape)}"]
    if not torch.equal(d, wd):
        bad.append(f"{int((d != wd).sum())} of {d.numel()} data bytes differ from amx_encode")
    if not torch.equal(s, ws):
        bad.append(f"{int((s != ws).sum())} of {s.numel()} scale bytes differ from amx_encode")
    return bad


def apb_unpack(image_int32, M, C, pad_rows):
    """the APB image -> (x float32 [M][C] with the sign of a zero read from the leading piece, violations of the guard convention).
    pad_rows "ff": the slots of rows >= M are untouched (the norm kernels); "zero": written as zeros (launch_split_rows_apb)."""
    img = np.asarray(image_int32.numpy() if isinstance(image_int32, torch.Tensor) else image_int32, dtype=np.int32)
    x, unowned, halves = R.apb_decode(img, M, C)
    bad = []
    if pad_rows == "ff" and not np.all(halves[unowned] == 0xFFFF):
        bad.append("an APB slot no row < M owns was written")
    if pad_rows == "zero" and not np.all(halves[unowned] == 0):
        bad.append("an APB slot of a row >= M is not written as zeros")
    if not np.all((halves[~unowned] & 0x7F80) != 0x7F80):
        bad.append("an APB slot of a real row was not written (or holds a non-finite piece)")
    hi = halves[R._apb_slots(rup(M, 128), C)[:M, :, 0]].reshape(M, C)
    neg_zero = torch.from_numpy((hi == 0x8000) & (x.numpy() == 0))
    return torch.where(neg_zero, torch.tensor(-0.0), x), bad


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- fp32 emulations (the tolerance check of tests/test_norm_ref_cpu.py) -----------------------------------------------------------------
def _sum32(t, order):
    """float32 row sums of t [M][C] in one of four orders"""
    t = t.float()
    M, C = t.shape
    if order == "torch":
        return t.sum(dim=1, keepdim=True)
    if order == "sequential":
        acc = torch.zeros(M, dtype=torch.float32)
        for c in range(C):
            acc = acc + t[:, c]
        return acc[:, None]
    if order == "reverse":
        return _sum32(t.flip(1), "sequential")
    assert order == "lanes"          # one float4 per lane and 64-lane stride, (x + y) + (z + w), then a butterfly over the 64 lanes
    nv = C // 4
    q4 = t.view(M, nv, 4)
    part = (q4[:, :, 0] + q4[:, :, 1]) + (q4[:, :, 2] + q4[:, :, 3])
    lanes = torch.zeros(M, 64, dtype=torch.float32)
    for q in range((nv + 63) // 64):
        seg = part[:, 64 * q:64 * q + 64]
        lanes[:, :seg.shape[1]] = lanes[:, :seg.shape[1]] + seg
    for off in (1, 2, 4, 8, 16, 32):
        lanes = lanes + lanes[:, torch.arange(64) ^ off]
    return lanes[:, :1]


ORDERS = ("torch", "sequential", "reverse", "lanes")


def layernorm_f32(x, w, b, order, mutant=None):
    """the kernels' expression in float32, sums in `order`.  mutant "one_pass": variance as max(E x^2 - mu^2, 0)"""
    x, w, b = x.float(), w.float(), b.float()
    C = x.shape[1]
    Cf = torch.tensor(float(C), dtype=torch.float32)
    mean = _sum32(x, order) / Cf
    d = x - mean
    if mutant == "one_pass":
        var = (_sum32(x * x, order) / Cf - mean * mean).clamp(min=0)
    else:
        var = _sum32(d * d, order) / Cf
    rstd = 1.0 / torch.sqrt(var + torch.tensor(LN_EPS, dtype=torch.float32))
    return d * rstd * w + b


def rmsnorm_f32(x, w, eps, order):
    x, w = x.float(), w.float()
    Cf = torch.tensor(float(x.shape[1]), dtype=torch.float32)
    r = 1.0 / torch.sqrt(_sum32(x * x, order) / Cf + torch.tensor(eps, dtype=torch.float32))
    return w * (x * r)


# ---- seeded inputs -------------------------------------------------------------------------------------------------------------------
LN_C = (96, 192, 384, 768)
LN_M = (1, 31, 33, 127, 129, 200)
LN_MAPPED = ((16, 4, 512), (8, 0, 128))                       # (R, shift, M) of gemm_ref.window_map
MERGE_CASES = ((1, 2, 96), (2, 8, 96), (2, 8, 192), (3, 4, 384))          # (n, R, Cin)
RMS_C = (64, 576)
RMS_M = (1, 33, 129, 389)
PLAIN_CASES = ((1, 64), (70, 96), (129, 224), (389, 576))
PLAIN_AMX_ONLY = ((70, 100),)                               # launch_quant_mx8 documents K % 4


def special_rows(M):
    """the rows of a case that hold the five special rows (none in a case of fewer than six rows)"""
    return [(k + 1) * M // 6 for k in range(5)] if M >= 6 else []


def _flush(x):
    """no fp32 denormal in an input"""
    return torch.where((x != 0) & (x.abs() < 2.0 ** -126), torch.zeros_like(x), x)


@functools.lru_cache(maxsize=None)
def rows(M, C, seed=0, zero_row=True):
    """x [M][C] float32: rows of different scale and offset; with M >= 6 also a large-mean / small-spread row (mean 100, spread 0.01;
    mean -1000, spread 1e-3 in every other case), a row whose variance is within 10 x of eps, a constant row, an all-zero row
    (zero_row) and a one-hot row.  w [C] about 1 +- 0.3 with one exact zero and one negative entry, b [C] N(0, 1).  Computed once,
    shared, read-only."""
    g = G._gen(M, C, seed, 4242)
    x = torch.randn(M, C, generator=g) * (0.2 + 3.0 * torch.rand(M, 1, generator=g)) + 0.5 * torch.randn(M, 1, generator=g)
    sp = special_rows(M)
    if sp:
        big = (100.0, 0.01) if (M + C // 32) % 2 == 0 else (-1000.0, 1e-3)
        x[sp[0]] = big[0] + big[1] * torch.randn(C, generator=g)
        x[sp[1]] = (3e-5 ** 0.5) * torch.randn(C, generator=g)
        x[sp[2]] = 0.7321
        x[sp[3]] = 0.0 if zero_row else torch.randn(C, generator=g)
        x[sp[4]] = 0.0
        x[sp[4], (7 * M + 5) % C] = 5.0
    w = 1.0 + 0.3 * (2.0 * torch.rand(C, generator=g) - 1.0)
    w[3 % C] = 0.0
    w[min(7, C - 1)] = -w[min(7, C - 1)]
    b = torch.randn(C, generator=g)
    return _flush(x), w, b


@functools.lru_cache(maxsize=None)
def merge_tokens(n, R, Cin):
    """x [n][R R][Cin] whose gathered rows are rows(n (R / 2)^2, 4 Cin): the special rows are special OUTPUT rows"""
    M = n * (R // 2) ** 2
    y, w, b = rows(M, 4 * Cin, seed=R)
    idx = merge_gather(torch.arange(n * R * R * Cin).view(n, R * R, Cin), n, R)          # [M][4 Cin] -> flat token element
    x = torch.empty(n * R * R * Cin)
    x[idx.reshape(-1)] = y.reshape(-1)
    return x.view(n, R * R, Cin), w, b


def _special_blocks(g):
    """32-column blocks for the quantiser: amax 448 2^n and its two fp32 neighbours (n = -20, 0, 20), e4m3 subnormals and ties under
    amax 448, -0.0, magnitudes 1e-30 and 1e30"""
    out = []
    for n in (-20, 0, 20):
        a = torch.tensor(448.0 * 2.0 ** n, dtype=torch.float32)
        for nb in (torch.nextafter(a, torch.tensor(0.0)), a, torch.nextafter(a, torch.tensor(float("inf")))):
            blk = (2.0 * torch.rand(32, generator=g) - 1.0) * 0.9 * a
            blk[int(torch.randint(0, 32, (1,), generator=g))] = nb if n else -nb
            out.append(blk)
    tie = torch.zeros(32)
    tie[0], tie[5], tie[6], tie[7], tie[8], tie[9] = 448.0, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -9, -(2.0 ** -10), -3 * 2.0 ** -10
    out.append(tie)
    out.append(torch.full((32,), -0.0))
    for mag in (1e-30, 1e30):
        out.append(mag * (0.5 + 1.5 * torch.rand(32, generator=g)) * torch.where(torch.rand(32, generator=g) < 0.5, -1.0, 1.0))
    return out


@functools.lru_cache(maxsize=None)
def plain_rows(M, C):
    """the input of op 3 (no norm): rows(M, C) with the special blocks placed over whole 32-column blocks of ordinary rows, as many as
    the case has room for (all 13 from 70 x 96 on)"""
    x = rows(M, C, seed=3)[0].clone()
    g = G._gen(M, C, 3, 777)
    nb = C // 32
    free = [(m, k) for m in range(M) if m not in special_rows(M) for k in range(nb)]
    blocks = _special_blocks(g)
    stride = max(1, len(free) // len(blocks))
    for i, blk in enumerate(blocks[:len(free)]):
        m, k = free[(i * stride) % len(free)] if len(free) >= len(blocks) else free[i]
        x[m, 32 * k:32 * k + 32] = blk
    return _flush(x)
