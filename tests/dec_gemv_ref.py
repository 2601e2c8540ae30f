"""Plain torch / numpy reference for the q/k/v, gate/up, down, fused down + q/k/v and final-norm launches of a decode step
(tests/test_dec_gemv_ref_cpu.py, tests/test_gpu_dec_gemv.py).  Nothing here imports the engine: the float64 definition of every
launch, the layouts and the slab ownership (transcribed from the COMMENTS of mellow_amd/csrc/dec_common.h, dec_gemv.hip and kernels.h, not from
their code; the codecs of the 576-column images are those of tests/dec_attn_ref.py), the seeded inputs, the case list, the
tolerance rule, an emulation of the tap's raw outputs in float32 (`emulate`: what the CPU test and its mutants feed to `check`)
and the one function that judges a set of raw outputs (`check`: the GPU test hands it the tap's).

The launches (rows = roundup(B, 32); slots B .. rows - 1 are zeros):
    op 0  x_new = x_mid + sum of the kcd down slabs; pq slab kc = W' . x_new over the columns 72 kc .. 72 kc + 71 (8 slabs);
          ssq1[kc] = sum of squares of the same columns; xnewR = the float32 sum in slab order (x_mid, then slab 0, 1, ...);
          first: rope_cur = row pos + inc_pos of the tables (cos | sin), the position word becomes pos + inc_pos
    op 1  r2 = 1 / sqrt(sum(ssq[0 .. 35]) / 576 + eps);  h = silu(r2 g) * (r2 u), g / u = gate / up . x_mid
    op 2  down slab kc = Wd . h over the columns 192 kc .. 192 kc + 191 (8 slabs)
    op 3  pq slab s (s = 0, 1) = W' . x_mid over the columns 288 s .. 288 s + 287 (2 chunks of 36 k-tiles); pq slab 2 + hc = Q . h
          over the columns 384 hc .. 384 hc + 383 (Q2_HC = 4 chunks); down slab hc = Wd . h over the same columns (the side tiles);
          Q = W' . Wd formed in float64 and rounded once
    op 4  xn = w * ((x_mid + sum of the kcd slabs) * rsqrt(mean^2 + eps))

Tolerance, per element, the rule of tests/gemm_ref.py unchanged (derived from the reference alone, never measured on a kernel):
    delta = (K + 8) * 2^-24 * r * (|A| . |W|^T),   tol = L * delta + 8 * 2^-24 * max(|ref|, |largest intermediate|)
K = the number of terms the accumulator sums.  Where the A operand is itself a float32 sum formed by the launch (x_new of op 0:
kcd additions, each within 2^-24 of a partial sum that |x_mid| + sum |slab| bounds), |A| is that bound and K grows by kcd: the
accumulation error is <= 72 u sum |a| |w| and the operand error <= kcd u |A| . |W|, together (72 + kcd) u |A| . |W|.  The sum of the
slabs is compared in float64 with the sum of the slabs' tolerances.  Op 1 is gemm_ref.swiglu_ref itself (K = 576, r = r2).
ssq1: within 144 * 2^-24 relative of the float64 sum of squares of the float32 x_new (72 squarings and 71 additions of
non-negative terms).  Op 3 is compared with W' x_mid + Q_returned h, so the rounding of Q adds no term there.  Q itself: within
2^-24 |Q64| (one rounding) + 576 * 2^-53 * (|W'| . |Wd|) (the float64 accumulation) of the float64 product.  The algebra, once:
sum of the six slabs against W' (x_mid + Wd h); replacing Q64 by its float32 rounding moves an element of Q by at most 2^-24 |Q64|,
hence the sum over k of Q h by at most 2^-24 (|Q64| . |h|): that term is added to the sum of the slabs' tolerances.
Op 4 (no accumulator: derived here).  x has the operand error kcd u |A| above; ss = sum x^2 over 576 columns has the relative error
<= 2 sum |x| dx / ss + 1151 u, and r = 1 / sqrt(ss / 576 + eps) half of it plus three roundings; y = w * (x * r) two more:
    tol = |w| r ((kcd + 2) u |A| + |x| (kcd u sum_j |A_j| |x_j| / (ss + 576 eps) + (576 + 8) u)) + 8 u |y|
The constants are never raised to make a measured case pass: a case above 1.0 is a finding."""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dec_attn_ref as A  # noqa: E402
import gemm_ref as G  # noqa: E402

HID, NQ, INTER = 576, 960, 1536
KC_QKV, KC_DOWN, Q2_HC, Q2_NPQ = 8, 8, 4, 6        # DEC_KC_QKV, DEC_KC_DOWN, Q2_HC, Q2_NPQ of kernels.h
U = G.U
F32, F64 = torch.float32, torch.float64
TMAX, POS = 16, 5
BIG_EPS = 4.0


# ---- layouts of the 1536-column images (the 576-column ones: dec_attn_ref) ------------------------------------------------------------
def f32_index(rows, K=HID):
    """F32-layout with K / 8 k-tiles: float4 ((rb * K/8 + k / 8) * 64 + m % 32 + 32 * (k / 4 % 2)) holds the columns k .. k + 3"""
    m, k = A._grid(rows, K)
    return (((m // 32) * (K // 8) + k // 8) * 64 + m % 32 + 32 * ((k // 4) % 2)) * 4 + k % 4


def f3_32_index(rows, K=HID):
    """F3-32, K / 16 pairs: 16-byte slot ((rb * K/16 + T) * 3 + piece) * 64 + lane, lane = m % 32 + 32 h; element e: k = 16 T + 8 h + e"""
    m, k = A._grid(rows, K)
    return np.stack([((((m // 32) * (K // 16) + k // 16) * 3 + piece) * 64 + m % 32 + 32 * ((k // 8) % 2)) * 8 + k % 8 for piece in range(3)])


def encode(x, index, total=None):
    """row-major f32 [rows][K] -> raw f32 image (elements nobody owns: 0xFF bytes)"""
    out = np.full(total or x.numel(), -1, dtype=np.int32).view(np.float32)
    out[index] = A._np(x.float())
    return torch.from_numpy(out)


def decode(raw, index):
    return torch.from_numpy(A._np(raw).reshape(-1)[index].copy())


def split3(x):
    x = x.contiguous().float()
    hi = x.to(torch.bfloat16)
    r1 = x - hi.float()
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.float()).to(torch.bfloat16)
    return np.stack([p.view(torch.int16).numpy() for p in (hi, mid, lo)])


def f3_encode(x, index3, total=None):
    """row-major f32 -> raw int16 image of bf16 triples (round-to-nearest three-way split)"""
    out = np.full(total or x.numel() * 3, -1, dtype=np.int16)
    out[index3] = split3(x)
    return torch.from_numpy(out)


def f3_decode(raw_i16, index3):
    u = A._np(raw_i16).reshape(-1).view(np.uint16)
    return torch.from_numpy(A._bf16_to_f64(u[index3]).sum(axis=0).astype(np.float32))


# ---- the case list ----------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, op, form, B, kcd=0, first=0, inc_pos=0, blk=None, eps=1e-5, want_x3=0):
        self.op, self.form, self.B, self.kcd, self.first, self.inc_pos = op, form, B, kcd, first, inc_pos
        self.blk, self.eps, self.want_x3 = (None if blk is None else tuple(blk)), eps, want_x3
        self.rows = (B + 31) // 32 * 32
        self.RB = self.rows // 32
        assert blk is None or len(blk) == self.RB >= 2

    @property
    def id(self):
        s = f"op{self.op}-f{self.form}-B{self.B}"
        if self.op in (0, 4):
            s += f"-kcd{self.kcd}"
        if self.op == 0 and self.first:
            s += f"-first-inc{self.inc_pos}"
        if self.want_x3:
            s += "-x3"
        if self.eps != 1e-5:
            s += "-bigeps"
        if self.blk is not None:
            s += "-blk" + "".join(str(b) for b in self.blk)
        return s

    @property
    def live_rows(self):
        """bool [rows]: the rows of the row blocks that run (pad rows of a live block are computed, on zeros)"""
        live = torch.ones(self.rows, dtype=torch.bool)
        if self.blk is not None:
            live = torch.tensor(self.blk, dtype=torch.bool).repeat_interleave(32)
        return live


def _cases():
    out = []
    forms = ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (1, 1), (3, 1))
    # the fp32 kernels: one row, a full block, two blocks with one row in the second (the 12-wave dec_qkv2), three blocks
    for B in (1, 32, 33, 70):
        out.append(Case(0, 0, B, 0, 1, 1))
        out.append(Case(0, 0, B, KC_DOWN))
        out.append(Case(1, 0, B, eps=BIG_EPS if B == 33 else 1e-5))
        out.append(Case(2, 0, B))
        out.append(Case(3, 0, B))
        out.append(Case(4, 0, B, 0, eps=BIG_EPS if B == 33 else 1e-5))
        out.append(Case(4, 0, B, KC_DOWN, want_x3=1))
    out.append(Case(0, 0, 33, 0, 1, 0))
    out.append(Case(4, 0, 33, KC_DOWN))
    out.append(Case(4, 0, 1, 0, want_x3=1))
    # the f32x3 forms: RBM 1 (RB 1), RBM 2 (RB 2), RBM 4 with a partial pass (RB 3), RBM 4 with a second pass of one block (RB 5)
    for B in (20, 33, 70, 130):
        out.append(Case(1, 1, B, eps=BIG_EPS if B == 33 else 1e-5))
        out.append(Case(3, 1, B))
    # blk_live, every launcher: a stopped middle block at RB = 3, a stopped last block at RB = 5
    for op, form in forms:
        kw = {"kcd": KC_DOWN} if op in (0, 4) else {}
        out.append(Case(op, form, 70, blk=(1, 0, 1), **kw))
        out.append(Case(op, form, 130, blk=(1, 1, 1, 1, 0), **kw))
    assert len({c.id for c in out}) == len(out)
    return out


CASES = _cases()
CASE_IDS = [c.id for c in CASES]


def case(cid):
    return CASES[CASE_IDS.index(cid)]


# ---- the seeded inputs ------------------------------------------------------------------------------------------------------------------
def _w(g, n, k):
    """rows and columns of different scale"""
    return torch.randn(n, k, generator=g) * 0.05 * (1.0 + torch.rand(n, 1, generator=g)) * (0.5 + torch.rand(1, k, generator=g))


@functools.lru_cache(maxsize=None)
def weights():
    """the logical weights every case shares (read-only): W' [960][576], gate / up [1536][576] (folded), Wd [576][1536], the down
    weight of another layer, the final norm vector (away from 1), and Q64 = W' . Wd in float64 with the bound of its accumulation"""
    g = torch.Generator().manual_seed(20240)
    w = {"Wq": _w(g, NQ, HID), "Wg": _w(g, INTER, HID), "Wu": _w(g, INTER, HID), "Wd": _w(g, HID, INTER), "Wd_other": _w(g, HID, INTER),
         "wn": 0.5 + 1.5 * torch.rand(HID, generator=g)}
    w["Q64"] = w["Wq"].double() @ w["Wd"].double()
    w["Q64_abs"] = w["Wq"].double().abs() @ w["Wd"].double().abs()
    w["rope"] = G.rope_tables(TMAX)
    return w


def q_tolerance():
    w = weights()
    return U * w["Q64"].abs() + HID * 2.0 ** -53 * w["Q64_abs"]


@functools.lru_cache(maxsize=None)
def inputs(B):
    """The activations of a batch (shared, read-only), at `rows` rows with zeros behind B: x_mid with a row rms of 2 .. 4, eight
    down slabs of the size of x_mid each, h with rows of different scale, ssq [rows][40] = the sums of squares of x_mid over 16
    columns each (36 of them; the columns 36 .. 39, which nobody reads, hold NaN)"""
    rows = (B + 31) // 32 * 32
    g = torch.Generator().manual_seed(1009 * B + 7)
    x = torch.zeros(rows, HID)
    x[:B] = torch.randn(B, HID, generator=g) * (2.0 + 2.0 * torch.rand(B, 1, generator=g))
    down = torch.zeros(KC_DOWN, rows, HID)
    down[:, :B] = torch.randn(KC_DOWN, B, HID, generator=g) * 3.0
    h = torch.zeros(rows, INTER)
    h[:B] = torch.randn(B, INTER, generator=g) * (0.2 + 3.0 * torch.rand(B, 1, generator=g))
    ssq = torch.full((rows, 40), float("nan"))
    ssq[:, :36] = (x.double() ** 2).view(rows, 36, 16).sum(-1).float()
    return {"x": x, "down": down, "h": h, "ssq": ssq}


# ---- float64 definitions (dtype = F32: the float32 evaluation) --------------------------------------------------------------------------
def _chunks(x, W, n, mutant=None):
    """the n split-K slabs of x . W^T by k-range -> [n][rows][N].  mutants: "swap" (slabs 0 and 1 take each other's k-range),
    "ktile" (the k-tile 5 of slab 1, eight columns, is left out)"""
    K = x.shape[1]
    w = K // n
    rng = [(i * w, i * w + w) for i in range(n)]
    if mutant == "swap":
        rng[0], rng[1] = rng[1], rng[0]
    out = []
    for i, (lo, hi) in enumerate(rng):
        xs = x[:, lo:hi]
        if mutant == "ktile" and i == 1:
            xs = xs.clone()
            xs[:, 40:48] = 0
        out.append(xs @ W[:, lo:hi].T)
    return torch.stack(out)


def x_new_of(inp, kcd, dtype, leave_out=None):
    """x_mid + the slabs in slab order (the float32 evaluation IS the kernel's sum: IEEE additions in a fixed order)"""
    x = inp["x"].to(dtype)
    for s in range(kcd):
        if s != leave_out:
            x = x + inp["down"][s].to(dtype)
    return x


def silu(g):
    return g / (1.0 + torch.exp(-g))


def ref(c, dtype=F64, mutant=None, Q=None):
    """the definition of case c's launch -> dict of row-major tensors [..][rows][..]"""
    w, inp = weights(), inputs(c.B)
    t = lambda name: w[name].to(dtype)      # noqa: E731
    km = mutant if mutant in ("swap", "ktile") else None
    if c.op == 0:
        x = x_new_of(inp, c.kcd, dtype, 3 if mutant == "slab_out" else None)
        out = {"pq": _chunks(x, t("Wq"), KC_QKV, km), "xnew": x, "ssq1": (x * x).view(c.rows, KC_QKV, 72).sum(-1)}
        if c.first:
            p = POS + (0 if mutant == "rope_row" else c.inc_pos)
            out["rope"] = torch.cat([w["rope"][0][p], w["rope"][1][p]])
            out["pos"] = POS + c.inc_pos
        return out
    if c.op == 1:
        x = inp["x"].to(dtype)
        Wg, Wu = (t("Wu"), t("Wg")) if mutant == "swap_gate_up" else (t("Wg"), t("Wu"))
        if km == "ktile":
            x = x.clone()
            x[:, 40:48] = 0
        g, u = x @ Wg.T, x @ Wu.T
        eps = 0.0 if mutant == "no_eps" else c.eps
        r2 = (1.0 / torch.sqrt(inp["ssq"][:, :36].to(dtype).sum(1) / HID + eps))[:, None]
        if mutant == "r2_one_factor":
            return {"h": silu(r2 * g) * u}
        if mutant == "r2_after_silu":
            return {"h": silu(g) * r2 * (r2 * u)}
        return {"h": silu(r2 * g) * (r2 * u)}
    if c.op == 2:
        return {"down": _chunks(inp["h"].to(dtype), t("Wd"), KC_DOWN, km)}
    if c.op == 3:
        Qm = (w["Q64"] if Q is None else Q.double()).to(dtype)
        x, h = inp["x"].to(dtype), inp["h"].to(dtype)
        side = Qm[:HID] if mutant == "side_q" else t("Wd")
        return {"pq": torch.cat([_chunks(x, t("Wq"), 2, km), _chunks(h, Qm, Q2_HC, km)]), "down": _chunks(h, side, Q2_HC, km)}
    x = x_new_of(inp, c.kcd, dtype, 3 if mutant == "slab_out" else None)
    eps = 0.0 if mutant == "no_eps" else c.eps
    r = 1.0 / torch.sqrt((x * x).sum(1, keepdim=True) / HID + eps)
    wn = torch.ones(HID, dtype=dtype) if mutant == "no_weight" else t("wn")
    return {"xn": wn * (x * r)}


def _slab_tol(x_abs, W, n, K_extra=0):
    K = x_abs.shape[1]
    w = K // n
    return torch.stack([(w + K_extra + 8) * U * (x_abs[:, i * w:i * w + w].double() @ W[:, i * w:i * w + w].double().abs().T) for i in range(n)])


@functools.lru_cache(maxsize=None)
def expected(cid, q_key=None):
    """the float64 reference of a case and its per-element tolerances (module docstring): dict ref, tol.  Op 3 takes the Q the launch
    used (q_key: a key of _Q_CACHE; None = Q64 rounded to float32)"""
    c, w, inp = case(cid), weights(), inputs(case(cid).B)
    Q = _Q_CACHE[q_key] if q_key is not None else w["Q64"].float()
    r = ref(c, F64, Q=Q)
    tol = {}
    a_abs = inp["x"].abs().double() + (inp["down"].abs().double().sum(0) if c.kcd else 0.0)
    if c.op == 0:
        tol["pq"] = _slab_tol(a_abs, w["Wq"], KC_QKV, c.kcd) + 8 * U * r["pq"].abs()
        x32 = x_new_of(inp, c.kcd, F32)
        r["xnew32"] = x32
        r["ssq1"] = (x32.double() ** 2).view(c.rows, KC_QKV, 72).sum(-1)          # of the float32 x_new, as the kernel forms it
        tol["ssq1"] = 144 * U * r["ssq1"]
    elif c.op == 1:
        r["h"], tol["h"] = G.swiglu_ref(inp["x"], w["Wg"], w["Wu"], rs=(inp["ssq"][:, :36], float(HID), c.eps))
    elif c.op == 2:
        tol["down"] = _slab_tol(inp["h"].abs(), w["Wd"], KC_DOWN) + 8 * U * r["down"].abs()
    elif c.op == 3:
        tol["pq"] = torch.cat([_slab_tol(inp["x"].abs(), w["Wq"], 2), _slab_tol(inp["h"].abs(), Q, Q2_HC)]) + 8 * U * r["pq"].abs()
        tol["down"] = _slab_tol(inp["h"].abs(), w["Wd"], Q2_HC) + 8 * U * r["down"].abs()
        x64, h64 = inp["x"].double(), inp["h"].double()
        r["algebra"] = (x64 + h64 @ w["Wd"].double().T) @ w["Wq"].double().T
        tol["algebra"] = tol["pq"].sum(0) + U * (h64.abs() @ w["Q64"].abs().T)
    else:
        x = x_new_of(inp, c.kcd, F64)
        ss = (x * x).sum(1, keepdim=True)
        rr = 1.0 / torch.sqrt(ss / HID + c.eps)
        rel = c.kcd * U * (a_abs * x.abs()).sum(1, keepdim=True) / (ss + HID * c.eps) + (HID + 8) * U
        tol["xn"] = w["wn"].double().abs() * rr * ((c.kcd + 2) * U * a_abs + x.abs() * rel) + 8 * U * r["xn"].abs()
    return {"ref": r, "tol": tol}


_Q_CACHE = {}


def register_q(Q):
    """remember a Q a launch returned, under a key that `expected` can be cached on"""
    key = hash(Q.numpy().tobytes())
    _Q_CACHE.setdefault(key, Q.clone())
    return key


# ---- the raw outputs of the tap: emulated (float32 evaluation) and judged ----------------------------------------------------------------
def _rows_mask(c, n_slabs, owned_slabs, width):
    m = torch.zeros(n_slabs, c.rows, width, dtype=torch.bool)
    m[:owned_slabs] = c.live_rows[None, :, None]
    return m


def _put_rows(values, mask, guard_rows):
    """row-major slabs [n][rows][width] -> raw f32 [(n * rows + guard_rows)][width], 0xFF where the mask is off"""
    n, rows, width = mask.shape
    out = torch.from_numpy(np.full(((n * rows + guard_rows), width), -1, dtype=np.int32).view(np.float32).copy())
    body = out[:n * rows].view(n, rows, width)
    full = torch.zeros(n, rows, width)
    full[:values.shape[0]] = values.float()
    body[mask] = full[mask]
    return out


def _put_image(values, mask, index, total):
    """row-major [n][rows][K] -> n consecutive raw f32 images + guard elements, 0xFF where the mask is off"""
    n, rows, K = mask.shape
    out = np.full(total, -1, dtype=np.int32).view(np.float32).copy()
    full = torch.zeros(n, rows, K)
    full[:values.shape[0]] = values.float()
    for s in range(n):
        idx = index[mask[s].numpy()] + s * rows * K
        out[idx] = full[s][mask[s]].numpy()
    return torch.from_numpy(out)


def emulate(c, mutant=None):
    """what the tap returns for case c when the launch computes the float32 evaluation of `ref` (or of a mutant of it) -> dict as
    Engine.debug_dec_gemv's, or None where the mutant does not apply to the case.  "dead_rows": the rows of a stopped block are
    written all the same; "q_other": Q composed with the down weight of another layer"""
    applies = {None: True, "swap": c.op in (0, 2, 3), "ktile": c.op in (0, 1, 2, 3), "slab_out": c.op in (0, 4) and c.kcd > 0,
               "swap_gate_up": c.op == 1, "r2_one_factor": c.op == 1, "r2_after_silu": c.op == 1,
               "no_eps": c.op in (1, 4) and c.eps == BIG_EPS, "rope_row": c.op == 0 and c.first and c.inc_pos, "q_other": c.op == 3,
               "side_q": c.op == 3, "no_weight": c.op == 4, "dead_rows": c.blk is not None}[mutant]
    if not applies:
        return None
    w = weights()
    cc = c
    if mutant == "dead_rows":
        cc = Case(c.op, c.form, c.B, c.kcd, c.first, c.inc_pos, None, c.eps, c.want_x3)
    Q = (w["Wq"].double() @ w["Wd_other" if mutant == "q_other" else "Wd"].double()).float() if c.op == 3 else None
    r = ref(c, F32, None if mutant in ("dead_rows", "q_other") else mutant, Q=Q)
    rows, out = c.rows, {}
    if c.op in (0, 3):
        out["pq"] = _put_rows(r["pq"], _rows_mask(cc, KC_QKV, KC_QKV if c.op == 0 else Q2_NPQ, NQ), 32)
    if c.op in (2, 3):
        out["down"] = _put_image(r["down"], _rows_mask(cc, KC_DOWN, KC_DOWN if c.op == 2 else Q2_HC, HID), f32_index(rows), KC_DOWN * rows * HID + 32 * HID)
    if c.op == 0:
        out["ssq1"] = _put_rows(r["ssq1"][None], _rows_mask(cc, 1, 1, KC_QKV), 32)
        out["xnew"] = _put_rows(r["xnew"][None], _rows_mask(cc, 1, 1, HID), 32)
        out["rope"] = torch.from_numpy(np.full(128, -1, dtype=np.int32).view(np.float32).copy())
        if c.first:
            out["rope"][:64] = r["rope"]
        out["pos"] = r["pos"] if c.first else POS
    if c.op == 1:
        mask = _rows_mask(cc, 1, 1, INTER)
        out["gu"] = _put_image(r["h"][None], mask, f32_index(rows, INTER), (rows + 32) * INTER)
        if c.form:
            img = np.full((rows + 32) * INTER * 3, -1, dtype=np.int16)
            idx3 = f3_32_index(rows, INTER)
            m = mask[0].numpy()
            img[idx3[:, m]] = split3(r["h"].float())[:, m]
            out["h3"] = torch.from_numpy(img)
    if c.op == 3:
        out["q"] = Q
    if c.op == 4:
        mask = _rows_mask(cc, 1, 1, HID)
        if c.want_x3:
            img = np.full((rows + 32) * HID * 3, -1, dtype=np.int16)
            idx3 = f3_32_index(rows)
            m = mask[0].numpy()
            img[idx3[:, m]] = split3(r["xn"].float())[:, m]
            out["xn"] = torch.from_numpy(img)
        else:
            out["xn"] = _put_image(r["xn"][None], mask, f32_index(rows), (rows + 32) * HID)
        if c.blk is not None:
            snap = torch.full((64,), -1, dtype=torch.int32)
            snap[:32] = 0
            snap[:c.RB] = torch.tensor(c.blk, dtype=torch.int32)
            out["snap"] = snap
    return out


def _ones(t):
    """bool: the words that still hold 0xFF bytes"""
    t = torch.as_tensor(t)
    return (t.view(torch.int32) if t.dtype == torch.float32 else t) == -1


def _guard(name, raw, owned_raw, res):
    """every word no live slot owns still holds 0xFF; every owned word is finite (an image of bf16 triples: no piece is inf / NaN)"""
    raw = torch.as_tensor(raw).reshape(-1)
    owned_raw = owned_raw.reshape(-1)
    res["guard " + name] = 0.0 if bool(_ones(raw)[~owned_raw].all()) else float("inf")
    own = raw[owned_raw]
    fin = torch.isfinite(own).all() if own.dtype == torch.float32 else ((own.int() & 0x7F80) != 0x7F80).all()
    res["finite " + name] = 0.0 if bool(fin) else float("inf")


def _own_rows(mask, guard_rows):
    n, rows, width = mask.shape
    return torch.cat([mask.reshape(n * rows, width), torch.zeros(guard_rows, width, dtype=torch.bool)])


def _own_image(mask, index, total):
    n, rows, K = mask.shape
    o = np.zeros(total, dtype=bool)
    for s in range(n):
        o[index[mask[s].numpy()] + s * rows * K] = True
    return torch.from_numpy(o)


def _miss(got, r, tol, live):
    """largest err / tol over the live rows (gemm_ref.miss: a zero tolerance asks for the exact value)"""
    return G.miss(got[..., live, :], r[..., live, :], tol[..., live, :])


def _bits(a, b):
    return 0.0 if torch.equal(torch.as_tensor(a).contiguous().view(torch.int32), torch.as_tensor(b).contiguous().view(torch.int32)) else float("inf")


def check(c, out):
    """judge the raw outputs of case c's launch -> dict name -> err / tol (bit statements and guards: 0 or inf).  A launch is right
    when every figure is <= 1."""
    res, rows, live = {}, c.rows, c.live_rows
    e = expected(c.id, register_q(out["q"]) if c.op == 3 else None)
    r, tol = e["ref"], e["tol"]
    if c.op in (0, 3):
        n_own = KC_QKV if c.op == 0 else Q2_NPQ
        mask = _rows_mask(c, KC_QKV, n_own, NQ)
        _guard("pq", out["pq"], _own_rows(mask, 32), res)
        got = out["pq"][:KC_QKV * rows].view(KC_QKV, rows, NQ)[:n_own]
        res["pq slabs"] = _miss(got, r["pq"], tol["pq"], live)
        res["pq sum"] = _miss(got.double().sum(0), r["pq"].sum(0), tol["pq"].sum(0), live)
    if c.op in (2, 3):
        n_own = KC_DOWN if c.op == 2 else Q2_HC
        mask, idx = _rows_mask(c, KC_DOWN, n_own, HID), f32_index(rows)
        _guard("down", out["down"], _own_image(mask, idx, KC_DOWN * rows * HID + 32 * HID), res)
        got = A.f32_decode(out["down"], rows, KC_DOWN)[:n_own]
        res["down slabs"] = _miss(got, r["down"], tol["down"], live)
        res["down sum"] = _miss(got.double().sum(0), r["down"].sum(0), tol["down"].sum(0), live)
    if c.op == 0:
        _guard("ssq1", out["ssq1"], _own_rows(_rows_mask(c, 1, 1, KC_QKV), 32), res)
        _guard("xnew", out["xnew"], _own_rows(_rows_mask(c, 1, 1, HID), 32), res)
        res["ssq1"] = _miss(out["ssq1"][:rows], r["ssq1"], tol["ssq1"], live)
        res["xnewR bits"] = _bits(out["xnew"][:rows][live], r["xnew32"][live])
        rope_own = torch.zeros(128, dtype=torch.bool)
        rope_own[:64] = bool(c.first)
        _guard("rope", out["rope"], rope_own, res)
        if c.first:
            res["rope_cur bits"] = _bits(out["rope"][:64], r["rope"])
        res["pos"] = 0.0 if int(out["pos"]) == (r["pos"] if c.first else POS) else float("inf")
    if c.op == 1:
        mask, idx = _rows_mask(c, 1, 1, INTER), f32_index(rows, INTER)
        _guard("gu", out["gu"], _own_image(mask, idx, (rows + 32) * INTER), res)
        got = decode(out["gu"], idx)
        res["h"] = _miss(got, r["h"], tol["h"], live)
        if c.form:
            idx3 = f3_32_index(rows, INTER)
            own = np.zeros((rows + 32) * INTER * 3, dtype=bool)
            own[idx3[:, mask[0].numpy()]] = True
            _guard("h3", out["h3"], torch.from_numpy(own), res)
            res["h3 == guF bits"] = _bits(f3_decode(out["h3"], idx3)[live], got[live])
    if c.op == 3:
        w = weights()
        res["Q"] = G.miss(out["q"], w["Q64"], q_tolerance())
        got = out["pq"][:Q2_NPQ * rows].view(Q2_NPQ, rows, NQ)
        res["algebra"] = _miss(got.double().sum(0), r["algebra"], tol["algebra"], live)
    if c.op == 4:
        mask = _rows_mask(c, 1, 1, HID)
        if c.want_x3:
            idx3 = f3_32_index(rows)
            own = np.zeros((rows + 32) * HID * 3, dtype=bool)
            own[idx3[:, mask[0].numpy()]] = True
            _guard("xn3", out["xn"], torch.from_numpy(own), res)
            got = f3_decode(out["xn"], idx3)
        else:
            idx = f32_index(rows)
            _guard("xn", out["xn"], _own_image(mask, idx, (rows + 32) * HID), res)
            got = decode(out["xn"], idx)
        res["xn"] = _miss(got, r["xn"], tol["xn"], live)
        if c.blk is not None:
            snap = torch.full((64,), -1, dtype=torch.int32)
            snap[:32] = 0
            snap[:c.RB] = torch.tensor(c.blk, dtype=torch.int32)
            res["blk_snap"] = 0.0 if torch.equal(torch.as_tensor(out["snap"]).int(), snap) else float("inf")
    return res


def worst(res):
    return max(res.values())


def sub_inputs(inp, B, keep=None):
    """the first B rows of a batch's activations as a batch of their own (zeros behind B); keep: bool [B], the rows that stay --
    the others become zero rows (the bit-identity tests: a row alone, the same rows in another block)"""
    rows = (B + 31) // 32 * 32
    sel = torch.ones(B, dtype=torch.bool) if keep is None else torch.as_tensor(keep)
    out = {"x": torch.zeros(rows, HID), "down": torch.zeros(KC_DOWN, rows, HID), "h": torch.zeros(rows, INTER), "ssq": torch.zeros(rows, 40)}
    out["ssq"][:, 36:] = float("nan")
    for name in ("x", "h", "ssq"):
        out[name][:B][sel] = inp[name][:B][sel]
    out["down"][:, :B][:, sel] = inp["down"][:, :B][:, sel]
    return out


def decoded(c, out):
    """the raw outputs of case c's launch as row-major tensors [..][rows][width] (bit-exact; an image of triples: their sum)"""
    rows, d = c.rows, {}
    if "pq" in out:
        d["pq"] = out["pq"][:KC_QKV * rows].view(KC_QKV, rows, NQ)
    if "down" in out:
        d["down"] = A.f32_decode(out["down"], rows, KC_DOWN)
    for name in ("ssq1", "xnew"):
        if name in out:
            d[name] = out[name][:rows]
    if "gu" in out:
        d["gu"] = decode(out["gu"], f32_index(rows, INTER))
    if "h3" in out:
        d["h3"] = f3_decode(out["h3"], f3_32_index(rows, INTER))
    if "xn" in out:
        d["xn"] = f3_decode(out["xn"], f3_32_index(rows)) if c.want_x3 else decode(out["xn"], f32_index(rows))
    return d


def tap_args(c, inp=None):
    """the keyword arguments of Engine.debug_dec_gemv for case c (host tensors; raw images of all rows); inp: other activations
    than the case's own (sub_inputs)"""
    w, inp, B, rows = weights(), (inputs(c.B) if inp is None else inp), c.B, c.rows
    kw = {"op": c.op, "B": B, "form": c.form, "eps": c.eps, "blk_live": None if c.blk is None else torch.tensor(c.blk, dtype=torch.int32)}
    if c.op == 0:
        kw.update(W=w["Wq"], x=inp["x"][:B], kcd=c.kcd, first=bool(c.first), inc_pos=bool(c.inc_pos), pos=POS)      # (a later launch leaves the word alone)
        if c.first:
            kw.update(Tmax=TMAX, rope_cos=w["rope"][0], rope_sin=w["rope"][1])
    elif c.op == 1:
        kw.update(W=w["Wg"], W2=w["Wu"], ssq=inp["ssq"])
        kw["x_img"] = f3_encode(inp["x"], A.f3_16_index(rows)) if c.form else A.f16_encode(inp["x"][None])
    elif c.op == 2:
        kw.update(W=w["Wd"], h=inp["h"][:B])
    elif c.op == 3:
        kw.update(W=w["Wq"], W2=w["Wd"])
        if c.form:
            kw.update(x_img=f3_encode(inp["x"], f3_32_index(rows)), h_img=f3_encode(inp["h"], f3_32_index(rows, INTER)))
        else:
            kw.update(x=inp["x"][:B], h=inp["h"][:B])
    else:
        kw.update(W=w["wn"], x=inp["x"][:B], kcd=c.kcd, want_x3=bool(c.want_x3))
    if c.op in (0, 4) and c.kcd:
        kw["down"] = inp["down"][:, :B]
    return kw


if __name__ == "__main__":
    for c_ in CASES:
        print(c_.id)
