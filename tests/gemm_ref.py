"""Float64 references for the GEMM kernels and their shared epilogue (tests/test_gemm_ref_cpu.py, tests/test_gpu_gemm.py).  Nothing here
imports the engine: the definitions, the seeded inputs both test modules use, and the tolerance rule.  The APB decode is the one of
tests/attn_ref.py.

Tolerance, per element, from the reference alone (derived, never measured on the kernel under test):
    delta = (K + 8) * 2^-24 * r * (|A| . |W|^T)[m][n]                      in float64
    tol   = L * delta + 8 * 2^-24 * max(|ref|, |largest intermediate|)
delta is the any-order fp32 accumulation bound K u sum|a||w| (u = 2^-24); the 8 covers the three dropped piece products of the f32x3
split (< 2^-23 |a w| each term in total).  r is the consumer row scale (1 without one).  L is the Lipschitz constant of what follows the
accumulator, taken from the float64 reference: 1 (no activation), 1.13 (GELU: max |gelu'| = 1.129), 0.25 (sigmoid); a RoPE output
o1 = x1 cos - x2 sin takes |cos| delta(x1) + |sin| delta(x2) (L = |cos| + |sin| with each factor on the accumulator it multiplies);
SwiGLU takes 1.1 |up| delta(gate) + |silu(gate)| delta(up) (max |silu'| = 1.0998).  The last term allows for the device erff / expf
and the roundings of the epilogue arithmetic: 8 units in the last place of the largest value the epilogue forms.  (A ROCm
installation carries OCML as bitcode only, with no document of its ulp bounds, so the figure stays this 8.)

ssq_out: against the float64 sum of squares of the STORED fp32 values of the row's 64-column group, within 2^-18 relative (63 additions
plus 64 squarings, first order: 127 * 2^-24 < 2^-17; pairwise in the half-wave it is far less, 2^-18 is what is asked)."""
import functools
import math

import torch

U = 2.0 ** -24
QH, KVH, HD = 9, 3, 64
ACT_L = {"none": 1.0, "gelu": 1.13, "sigmoid": 0.25}
SSQ_RTOL = 2.0 ** -18


# ---- float64 definitions -----------------------------------------------------------------------------------------------------------
def acc64(A, W):
    """(A . W^T, |A| . |W|^T) in float64"""
    a, w = A.double(), W.double()
    return a @ w.T, a.abs() @ w.abs().T


def row_scale(rs_ssq, rs_dim, rs_eps):
    """r [M] = 1 / sqrt(sum_p ssq[m][p] / rs_dim + rs_eps) in float64; None -> None"""
    if rs_ssq is None:
        return None
    return 1.0 / torch.sqrt(rs_ssq.double().sum(dim=1) / float(rs_dim) + float(rs_eps))


def _act(x, act):
    if act == "gelu":
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if act == "sigmoid":
        return 1.0 / (1.0 + torch.exp(-x))
    assert act == "none"
    return x


def crows(M, crow_map=None, rows_out=0):
    """(C row of every GEMM row m [M], number of C rows)"""
    m = torch.arange(M)
    if crow_map is None:
        return m, M
    cm = torch.as_tensor(crow_map).long()
    rows_in = cm.numel()
    assert M % rows_in == 0
    return (m // rows_in) * rows_out + cm[m % rows_in], M // rows_in * rows_out


def linear_ref(A, W, N, bias=None, act="none", resid=None, crow_map=None, rows_out=0, rs=None, mutant=None):
    """act(acc r + bias) + resid, scattered to the mapped rows.  A [M][K], W [Nw][K], N >= Nw stored columns (weight rows and bias
    beyond Nw are zeros), resid [C rows][N], rs = (ssq [M][parts], dim, eps) or None.
    -> (ref float64 [C rows][N] with NaN in the rows no GEMM row maps to, tol [C rows][N] likewise, crow [M])
    mutant: "bias_after_act", "resid_before_act", "crow_inverted", "rs_after_bias" (the sensitivity test)."""
    M, K = A.shape
    Nw = W.shape[0]
    Wn = torch.zeros(N, K, dtype=W.dtype)
    Wn[:Nw] = W
    acc, aabs = acc64(A, Wn)
    r = torch.ones(M, dtype=torch.float64) if rs is None else row_scale(*rs)
    b = torch.zeros(N, dtype=torch.float64)
    if bias is not None:
        b[:Nw] = bias.double()
    cmap = crow_map
    if mutant == "crow_inverted":
        cm = torch.as_tensor(crow_map).long()
        lo = int(cm.min())
        inv = torch.empty_like(cm)
        inv[cm - lo] = torch.arange(cm.numel())
        cmap = inv + lo
    crow, n_c = crows(M, cmap, rows_out)
    res = torch.zeros(M, N, dtype=torch.float64) if resid is None else resid.double()[crow]
    x = acc * r[:, None]
    if mutant == "rs_after_bias":
        pre = (acc + b) * r[:, None]
    elif mutant == "bias_after_act":
        pre = x
    elif mutant == "resid_before_act":
        pre = x + b + res
    else:
        pre = x + b
    y = _act(pre, act)
    if mutant == "bias_after_act":
        y = y + b
    out = y if mutant == "resid_before_act" else y + res
    delta = (K + 8) * U * r[:, None] * aabs
    big = torch.stack([out.abs(), x.abs(), pre.abs(), y.abs(), res.abs()]).amax(dim=0)
    tol = ACT_L[act] * delta + 8 * U * big
    ref_c = torch.full((n_c, N), float("nan"), dtype=torch.float64)
    tol_c = torch.full((n_c, N), float("nan"), dtype=torch.float64)
    ref_c[crow] = out
    tol_c[crow] = tol
    return ref_c, tol_c, crow


def swiglu_ref(A, Wg, Wu, rs=None, mutant=None):
    """silu(gate) * up on the logical gate / up weights [N][K] -> (ref float64 [M][N], tol).  mutant: "swap_gate_up"."""
    K = A.shape[1]
    if mutant == "swap_gate_up":
        Wg, Wu = Wu, Wg
    g, gabs = acc64(A, Wg)
    u, uabs = acc64(A, Wu)
    r = torch.ones(A.shape[0], dtype=torch.float64) if rs is None else row_scale(*rs)
    g, u = g * r[:, None], u * r[:, None]
    sg = g / (1.0 + torch.exp(-g))
    out = sg * u
    dg, du = (K + 8) * U * r[:, None] * gabs, (K + 8) * U * r[:, None] * uabs
    big = torch.stack([out.abs(), g.abs(), u.abs(), sg.abs()]).amax(dim=0)
    return out, 1.1 * u.abs() * dg + sg.abs() * du + 8 * U * big


def qkv_rope_ref(A, W, B, T, Tmax, pos0, cos, sin, rs=None, mutant=None):
    """HF apply_rotary_pos_emb on the 9 q and 3 k heads at position pos0 + m % (T - pos0), v unrotated; W [960][K] = 576 q, 192 k,
    192 v rows; cos / sin [Tmax][32].  -> dict q, k, v (float64; pages [B][3][Tmax][64], NaN at the positions nobody writes) and
    q_tol, k_tol, v_tol.  mutant: "rot_sign", "no_pos0", "v_rotated", "kv_head_off"."""
    M, K = A.shape
    Tq = T - pos0
    assert M == B * Tq and W.shape[0] == 960
    acc, aabs = acc64(A, W)
    r = torch.ones(M, dtype=torch.float64) if rs is None else row_scale(*rs)
    x = (acc * r[:, None]).view(M, 15, 2, 32)
    d = ((K + 8) * U * r[:, None] * aabs).view(M, 15, 2, 32)
    m = torch.arange(M)
    b, t = m // Tq, pos0 + m % Tq
    tr = m % Tq if mutant == "no_pos0" else t
    c, s = cos.double()[tr][:, None, :], sin.double()[tr][:, None, :]
    sign = -1.0 if mutant == "rot_sign" else 1.0
    x1, x2, d1, d2 = x[:, :, 0], x[:, :, 1], d[:, :, 0], d[:, :, 1]
    o = torch.stack([x1 * c - sign * x2 * s, x2 * c + sign * x1 * s], dim=2)          # q cos + rotate_half(q) sin
    big = torch.stack([x1.abs(), x2.abs()]).amax(dim=0)
    to = torch.stack([c.abs() * d1 + s.abs() * d2, c.abs() * d2 + s.abs() * d1], dim=2) + 8 * U * torch.maximum(o.abs(), big[:, :, None])
    tx = d + 8 * U * x.abs()
    rot = 15 if mutant == "v_rotated" else 12
    y = torch.cat([o[:, :rot], x[:, rot:]], dim=1).reshape(M, 960)
    ty = torch.cat([to[:, :rot], tx[:, rot:]], dim=1).reshape(M, 960)
    out = {"q": y[:, :576], "q_tol": ty[:, :576]}
    for name, c0 in (("k", 576), ("v", 768)):
        page = torch.full((B, KVH, Tmax, HD), float("nan"), dtype=torch.float64)
        ptol = torch.full((B, KVH, Tmax, HD), float("nan"), dtype=torch.float64)
        for h in range(KVH):
            hs = (h + 1) % KVH if mutant == "kv_head_off" else h
            page[b, h, t] = y[:, c0 + 64 * hs:c0 + 64 * hs + 64]
            ptol[b, h, t] = ty[:, c0 + 64 * hs:c0 + 64 * hs + 64]
        out[name], out[name + "_tol"] = page, ptol
    return out


def ssq_ref(stored, group_shift=0):
    """float64 sums of squares of the stored fp32 rows [M][N] over each 64-column group -> [M][N / 64].  group_shift = 1: the
    neighbouring group (the sensitivity test)."""
    M, N = stored.shape
    s = (stored.double() ** 2).view(M, N // 64, 64).sum(dim=2)
    return torch.roll(s, group_shift, dims=1) if group_shift else s


def miss(got, ref, tol):
    """largest |got - ref| / tol over the elements the reference owns (tol is NaN elsewhere)"""
    own = ~torch.isnan(tol)
    err, t = (got.double() - ref).abs()[own], tol[own]
    # tol == 0 (an exact zero: a zero weight row and nothing added): only the exact value passes
    ratio = torch.where(t > 0, err / t, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(ratio.max())


# ---- seeded inputs -------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    seed = 12345
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def operands(M, Nw, K, seed=0):
    """A [M][K] with rows of different scale, W [Nw][K], bias [Nw]: computed once, shared, read-only"""
    g = _gen(M, Nw, K, seed)
    A = torch.randn(M, K, generator=g) * (0.2 + 3.0 * torch.rand(M, 1, generator=g))
    W = torch.randn(Nw, K, generator=g) * 0.05 * (1.0 + torch.rand(Nw, 1, generator=g))
    bias = torch.randn(Nw, generator=g)
    return A, W, bias


@functools.lru_cache(maxsize=None)
def residual(rows, N, seed=0):
    return torch.randn(rows, N, generator=_gen(rows, N, seed, 77))


@functools.lru_cache(maxsize=None)
def row_ssq(M, parts=9, dim=576.0, seed=0):
    """sum-of-squares partials of rows of different scale -> (ssq [M][parts], dim, eps) as rs"""
    g = _gen(M, parts, seed, 99)
    s = (0.5 + torch.rand(M, parts, generator=g)) * (dim / parts) * (0.3 + 2.0 * torch.rand(M, 1, generator=g)) ** 2
    return s.float(), float(dim), 1e-5


@functools.lru_cache(maxsize=None)
def rope_tables(Tmax, offset=17, theta=100000.0):
    """cos / sin [Tmax][32] float32 of the angle (t + offset) inv_freq: no row is the trivial (1, 0) and all rows differ"""
    inv = theta ** (-torch.arange(0, HD, 2, dtype=torch.float64) / HD)
    ang = (torch.arange(Tmax, dtype=torch.float64) + offset)[:, None] * inv[None, :]
    return torch.cos(ang).float(), torch.sin(ang).float()


def emb_map(seed=5):
    """32 -> 33 rows, as the engine's emb_row_map ({1 .. 32}: row 0 of every 33 is somebody else's) but a real permutation"""
    return (1 + torch.randperm(32, generator=_gen(seed, 33))).to(torch.int32), 33


def window_map(R=16, shift=4):
    """the shifted-window row map (roll by -shift, partition in 8 x 8 windows): row m of the window-ordered batch is token map[m]"""
    tok = torch.arange(R * R).view(R, R)
    if shift:
        tok = torch.roll(tok, shifts=(-shift, -shift), dims=(0, 1))
    ws = min(R, 8)
    return tok.view(R // ws, ws, R // ws, ws).permute(0, 2, 1, 3).reshape(-1).to(torch.int32), R * R
