"""Plain torch / numpy / Python reference for the launches that end a decode step: the lm_head (fp32 and streaming f32x3 form), the
arg-max with the step epilogue, the row repack and the row load (tests/test_dec_tail_ref_cpu.py, tests/test_gpu_dec_tail.py).
Nothing here imports the engine: the float64 definition of the head, an integer model of the step epilogue and of the repack
(transcribed from the COMMENTS of mellow_amd/csrc/step_tail.h, kernels.h and dec_tail.hip, not from their code; the codecs are those of
tests/dec_gemv_ref.py), the seeded inputs, the case list, the tolerance rules, an emulation of the tap's raw outputs (`emulate`: what
the CPU test and its mutants feed to `check`) and the one function that judges a set of raw outputs (`check`: the GPU test hands it
the tap's).

The launches (rows = roundup(B, 32); a tile = 32 columns of the vocabulary; n = V / 32):
    head    logits = x . W^T, K = 576; per row and tile cand_val / cand_idx = the winner in arg_better order (NaN wins, lowest column on
            ties) of the tile's stored logits, cand_sum = sum_j exp(l_j - cand_val)
    argmax  per slot b: example row = row_of_slot[b] (or b); dead = blk_snap[b / 32] == 0 or row < 0.  A live slot: token = the
            arg_better winner of its n planted (cand_val, cand_idx), clamped into [0, 32 n); tokens[b] = token; with a state: column
            step = pos - T0 + 1 of the EXAMPLE's record takes the token (0 <= step < max_len), and -log S with S = sum_t s_t exp(m_t - M);
            a token == stop_id of an example not yet stopped sets seen_stop[row], n_seen += 1, blk_left[b / 32] -= 1, and the one that
            brings it to 0 clears blk_live[b / 32]; write_x: embed[token] becomes the F32-layout row of the SLOT.  Every slot, dead
            ones too, arrives; the last resets `arrive` to 0, ticket += 1 and publishes (ticket << 32 | n_seen).
    pack    active = row >= 0 and blk_live[slot / 32] and not seen_stop[row]; if ceil(n_act / 32) < live blocks: the active slots
            move, stably, to the slots 0 .. n_act - 1 (x rows and row_of_slot; the other row_of_slot entries below B become -1, the
            other x rows stay), blk_left[k] = clamp(n_act - 32 k, 0, 32), blk_live = blk_left > 0, n_compactions += 1; else NOTHING changes
    load    x row b = in[clamp(row_ids[b], 0, n_src - 1)], or in[b T_last + T_last - 1]

Tolerances (derived from the reference alone, never measured on a kernel; a case above 1.0 is a finding, no constant is raised):
    logits    the rule of tests/gemm_ref.py unchanged, both forms: (K + 8) * 2^-24 * (|x| . |W|^T) + 8 * 2^-24 * |ref|, K = 576
    cand_val / cand_idx   exact: bit for bit the winner of the logits the SAME launch stored (of its twin launch with want_logits = 0)
    cand_sum  against the float64 sum over the tile's STORED float32 logits, relative (31 + 8 + max_j |l_j - m|) * 2^-24: 31 additions of
              positive terms, the 8 of gemm_ref.py for the device expf, and the rounding of the exponent's argument (a relative error
              2^-24 of l_j - m moves exp by |l_j - m| * 2^-24)
    logprob   S relative (ceil(n / 256) + 6 + 3 + 1 + 8) * 2^-24: the chain of dec_lse_sum (a thread's ceil(n / 256) terms, six butterfly
              steps, three additions of the waves), one product, and the expf allowance; -log S takes that figure plus 2^-24 |log S|
    everything else (tokens, records, counters, words, moved and gathered rows) is exact
Where a token is compared with the float64 arg-max, the float64 gap between best and runner-up exceeds twice the tolerance: the
seeds are searched until that holds on EVERY row that is neither a tie nor NaN (`head_inputs`)."""
import functools
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dec_gemv_ref as D  # noqa: E402
import gemm_ref as G  # noqa: E402

HID = 576
U = G.U
F32, F64 = torch.float32, torch.float64
INT_MAX = 0x7FFFFFFF
INF = float("inf")


def _ff(shape, dtype=np.float32):
    """an array of 0xFF bytes"""
    return np.full(shape, -1, dtype=np.int32 if dtype == np.float32 else dtype).view(dtype).copy()


def _is_ff(t):
    t = torch.as_tensor(t)
    return (t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t) == -1


def _bits_equal(a, b):
    a, b = torch.as_tensor(a).contiguous(), torch.as_tensor(b).contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _yes(ok):
    return 0.0 if bool(ok) else INF


# ---- the case list ----------------------------------------------------------------------------------------------------------------------
class Case:
    """kind "head": form, B, V, want_logits, want_sum, blk;  "argmax" / "pack" / "load": name (the planted state: `planted`)"""

    def __init__(self, kind, B, form=0, V=0, want_logits=1, want_sum=0, blk=None, name=""):
        self.kind, self.B, self.form, self.V, self.want_logits, self.want_sum = kind, B, form, V, want_logits, want_sum
        self.blk, self.name = (None if blk is None else tuple(blk)), name
        self.rows = (B + 31) // 32 * 32
        self.RB = self.rows // 32
        self.n = V // 32
        assert blk is None or len(blk) == self.RB >= 2

    @property
    def id(self):
        if self.kind != "head":
            return f"{self.kind}-{self.name}"
        s = f"head-f{self.form}-V{self.V}-B{self.B}-l{self.want_logits}s{self.want_sum}"
        return s + ("" if self.blk is None else "-blk" + "".join(str(b) for b in self.blk))

    @property
    def live_rows(self):
        """bool [rows]: the rows of the row blocks that run (pad rows of a live block are computed, on zeros)"""
        if self.blk is None:
            return torch.ones(self.rows, dtype=torch.bool)
        return torch.tensor(self.blk, dtype=torch.bool).repeat_interleave(32)

    def twin(self):
        """the same launch with the logits stored"""
        return Case("head", self.B, self.form, self.V, 1, self.want_sum, self.blk)


def head_G(RB):
    """row blocks a pass of the streaming kernel holds (1, 2, or 4 for every larger count)"""
    return RB if RB in (1, 2) else 4


ARGMAX_NAMES = ("B3-n8-noloop", "B3-n8-noloop-x", "B33-n264-noloop-x", "B3-n8-col0-lp-x", "B3-n8-colm1", "B3-n8-collast-lp", "B3-n8-colmax",
                "B33-n8-stops", "B70-n264-blk-slots-lp-x", "B70-n8-blk-x")
PACK_NAMES = ("B64-5-in-block1", "B96-101-holes", "B64-slots1to40", "B96-slots1to40", "B1024-40-scattered", "B64-33-none", "B64-nact0")
LOAD_NAMES = ("B33-ids-clamped", "B70-Tlast3-ld600", "B1-id")


def _cases():
    out = []
    # the fp32 kernel: one row, a full block, two blocks with one row in the second, three blocks; V = 96 has P-layout pad rows
    for V, Bs in ((96, (1, 33)), (256, (32,)), (768, (70,)), (8448, (33,))):
        out += [Case("head", B, 0, V, 1, 1) for B in Bs]
    out.append(Case("head", 1, 0, 768, 1, 0))
    out.append(Case("head", 32, 0, 96, 1, 0))
    # the streaming kernel: G 1 (B 1, 20), G 2 (33), G 4 with gn = 3 (70), G 4 full (128), a second pass of one block (130)
    for B, V in ((1, 256), (20, 768), (33, 8448), (70, 768), (128, 256), (130, 768)):
        out.append(Case("head", B, 1, V, 1, 1))
    out.append(Case("head", 20, 1, 256, 1, 0))
    out.append(Case("head", 130, 1, 8448, 1, 0))
    # want_sum x want_logits at B = 70 (l1s1 is above), and blk_live at RB 3 / RB 5 with and without want_sum, both forms
    for form in (0, 1):
        out += [Case("head", 70, form, 768, lg, sm) for lg, sm in ((1, 0), (0, 1), (0, 0))]
        for sm in (0, 1):
            out.append(Case("head", 70, form, 768, 1, sm, blk=(1, 0, 1)))
            out.append(Case("head", 130, form, 256, 1, sm, blk=(1, 1, 1, 1, 0)))
    out += [Case("argmax", int(nm.split("-")[0][1:]), V=32 * int(nm.split("-")[1][1:]), name=nm) for nm in ARGMAX_NAMES]
    out += [Case("pack", int(nm.split("-")[0][1:]), name=nm) for nm in PACK_NAMES]
    out += [Case("load", int(nm.split("-")[0][1:]), name=nm) for nm in LOAD_NAMES]
    assert len({c.id for c in out}) == len(out)
    return out


CASES = _cases()
CASE_IDS = [c.id for c in CASES]


def case(cid):
    return CASES[CASE_IDS.index(cid)]


# ---- head: the seeded inputs --------------------------------------------------------------------------------------------------------------
def tie_cols(V):
    """the columns that hold one and the same weight row: n + 2 and n + 5 of tile 1 (the two h halves of the streaming kernel), 8 q
    apart in tile 2, a tile of another workgroup (8 tiles each) and one more than 256 tiles away, where the vocabulary has them"""
    cols = [32 + 2, 32 + 5, 64 + 3, 64 + 11]
    if V >= 768:
        cols.append(9 * 32 + 7)
    if V >= 8448:
        cols.append(258 * 32 + 2)
    return cols


PEAK_COL = 20


@functools.lru_cache(maxsize=None)
def head_weight(V):
    """W [V][576]: rows x 1 .. 2, columns x 0.5 .. 1.5; the row of tie_cols(V)[0] duplicated at the others"""
    g = torch.Generator().manual_seed(5000 + V)
    W = torch.randn(V, HID, generator=g) * 0.05 * (1.0 + torch.rand(V, 1, generator=g)) * (0.5 + torch.rand(1, HID, generator=g))
    cols = tie_cols(V)
    W[cols[1:]] = W[cols[0]].clone()
    return W


def planted_rows(B):
    """row -> what is planted there, B permitting: peaked (proportional to a weight row), zero, nan, tie (proportional to the
    duplicated weight row); a second tie row ends the batch from two blocks on"""
    p = {}
    if B >= 20:
        p.update({1: "peaked", 2: "zero", 3: "nan", 4: "tie"})
    if B >= 33:
        p[B - 1] = "tie"
    return p


def _head_x(V, B, seed):
    g = torch.Generator().manual_seed(seed)
    rows = (B + 31) // 32 * 32
    W = head_weight(V)
    x = torch.zeros(rows, HID)
    x[:B] = torch.randn(B, HID, generator=g) * (0.25 * 16.0 ** torch.rand(B, 1, generator=g))      # row rms 0.25 .. 4
    for r, what in planted_rows(B).items():
        w = W[PEAK_COL if what == "peaked" else tie_cols(V)[0]]
        x[r] = {"zero": torch.zeros(HID), "nan": torch.full((HID,), float("nan"))}.get(what, w * (2.0 / w.pow(2).mean().sqrt()))
    return x


def _head_ref(V, x):
    W = head_weight(V).double()
    ref = x.double() @ W.T
    tol = (HID + 8) * U * (x.double().abs() @ W.abs().T) + 8 * U * ref.abs()
    return ref, tol


def _gap_ok(V, B, x, ref, tol):
    """on every row that is neither a tie nor NaN: float64 best - runner-up > 2 x the larger of their tolerances"""
    plain = [r for r in range(B) if planted_rows(B).get(r) not in ("tie", "nan", "zero")]
    top = torch.topk(ref[plain], 2, dim=1)
    t = torch.gather(tol[plain], 1, top.indices).amax(1)
    return bool(((top.values[:, 0] - top.values[:, 1]) > 2 * t).all())


@functools.lru_cache(maxsize=None)
def head_inputs(V, B):
    """x [rows][576] (zeros behind B), the float64 logits, their tolerance, the seed that was taken (module docstring: the gap rule)"""
    for seed in range(1000 * B + V, 1000 * B + V + 64):
        x = _head_x(V, B, seed)
        ref, tol = _head_ref(V, x)
        if _gap_ok(V, B, x, ref, tol):
            return {"x": x, "ref": ref, "tol": tol, "seed": seed}
    raise AssertionError(f"no seed separates the arg-max of every plain row at V = {V}, B = {B}")


def compared_rows(c):
    """rows whose arg-max is compared with the float64 arg-max: the plain and peaked ones of the live blocks"""
    live = c.live_rows
    return [r for r in range(c.B) if planted_rows(c.B).get(r) not in ("tie", "nan", "zero") and bool(live[r])]


@functools.lru_cache(maxsize=None)
def head_logits32(V, B):
    """the float32 evaluation: a product per element and a sum per (row, column) in one fixed order, so duplicated weight rows give
    equal bits as they do on one kernel instantiation"""
    x, W = head_inputs(V, B)["x"], head_weight(V)
    return torch.stack([(W * x[r]).sum(1) if r < B else torch.zeros(V) for r in range(x.shape[0])])      # (a pad row: zeros)


# ---- head: partials of stored logits --------------------------------------------------------------------------------------------------------
def tile_winner(logits, pick="low"):
    """logits f32 [R][V] -> (cand_val bits-exact f32 [R][n], cand_idx i32 [R][n]) in arg_better order: NaN wins, lowest column on ties"""
    L = logits.numpy().reshape(logits.shape[0], -1, 32)
    key = np.where(np.isnan(L), np.inf, L)
    idx = key.argmax(axis=2)                                   # numpy: the first occurrence
    val = np.take_along_axis(L, idx[..., None], axis=2)[..., 0]
    cols = idx + 32 * np.arange(L.shape[1])[None, :]
    return torch.from_numpy(val.copy()), torch.from_numpy(cols.astype(np.int32))


def tile_sum64(logits, m=None):
    """float64 sum_j exp(l_j - m) over each tile of the stored logits (m: the tile maximum) and max_j |l_j - m|"""
    L = logits.double().reshape(logits.shape[0], -1, 32)
    m = L.amax(2, keepdim=True) if m is None else m
    d = L - m
    return torch.exp(d).sum(2), d.abs().amax(2)


# ---- head: emulate and check ------------------------------------------------------------------------------------------------------------------
HEAD_MUTANTS = ("kpair", "phase_swap", "tail_fill", "half_tie", "sum_rowmax", "sum_half", "dead_rows")


def _head_mut_logits(c, mutant):
    inp = head_inputs(c.V, c.B)
    l32 = head_logits32(c.V, c.B)
    x, W = inp["x"].double(), head_weight(c.V).double()
    Gn = head_G(c.RB)

    def part(xs, ws):
        return x[:, xs] @ W[:, ws].T
    if mutant == "kpair":                        # k-pair 7 (16 columns) of the second phase (the second half of K at G 1) left out
        k0 = (576 // max(Gn, 2)) + 7 * 16
        return (l32.double() - part(slice(k0, k0 + 16), slice(k0, k0 + 16))).float()
    if mutant == "phase_swap":                   # the activations of phases 0 and 1 exchanged: x of one k-range against W of the other
        w = 576 // Gn
        a, b = slice(0, w), slice(w, 2 * w)
        return (l32.double() - part(a, a) - part(b, b) + part(a, b) + part(b, a)).float()
    return l32


def emulate_head(c, mutant=None):
    applies = {None: True, "kpair": True, "phase_swap": c.form == 1 and head_G(c.RB) >= 2, "tail_fill": c.form == 1 and c.RB % head_G(c.RB) != 0,
               "half_tie": c.form == 1, "sum_rowmax": bool(c.want_sum), "sum_half": c.form == 1 and bool(c.want_sum),
               "dead_rows": c.blk is not None}[mutant]
    if not applies:
        return None
    rows, n, V = c.rows, c.n, c.V
    l32 = _head_mut_logits(c, mutant)
    # "tail_fill": the stage slots of the groups g >= gn are filled from block rb0 + g instead of block rb0 -- those slots feed
    # accumulators that are neither formed (g < gn guards the products) nor stored, so the outputs are the baseline's
    live = torch.ones(rows, dtype=torch.bool) if mutant == "dead_rows" else c.live_rows
    val, idx = tile_winner(l32)
    if mutant == "half_tie":                     # the exchange of the two half-tiles keeps the higher column when both halves tie
        L = l32.numpy().reshape(rows, n, 4, 2, 4)                    # column = 8 q + 4 h + j
        half = [np.ascontiguousarray(L[:, :, :, h, :]).reshape(rows, n, 16) for h in (0, 1)]
        best = []
        for h in (0, 1):
            key = np.where(np.isnan(half[h]), np.inf, half[h])
            i = key.argmax(2)
            best.append((np.take_along_axis(key, i[..., None], 2)[..., 0], 8 * (i // 4) + 4 * h + i % 4))
        tie = torch.from_numpy(best[0][0] == best[1][0])
        hi = torch.from_numpy(np.maximum(best[0][1], best[1][1]).astype(np.int32)) + 32 * torch.arange(n, dtype=torch.int32)[None, :]
        idx = torch.where(tie, hi, idx)
    out = {"logits": torch.from_numpy(_ff((rows + 32, V))), "cand_val": torch.from_numpy(_ff((rows + 32, n))),
           "cand_idx": torch.from_numpy(_ff((rows + 32, n), np.int32)), "cand_sum": torch.from_numpy(_ff((rows + 32, n)))}
    if c.want_logits:
        out["logits"][:rows][live] = l32[live]
    out["cand_val"][:rows][live] = val[live]
    out["cand_idx"][:rows][live] = idx[live]
    if c.want_sum:
        L = l32.reshape(rows, n, 32)
        m = L.amax(2, keepdim=True)
        m = torch.where(torch.isnan(L).any(2, keepdim=True), torch.full_like(m, float("nan")), m)
        if mutant == "sum_rowmax":
            m = m.amax(1, keepdim=True).expand(rows, n, 1)
        e = torch.exp(L - m)
        if mutant == "sum_half":                 # the partner's sixteen columns (h = 1) left out
            e = e.reshape(rows, n, 4, 2, 4)[:, :, :, 0, :].reshape(rows, n, 16)
        out["cand_sum"][:rows][live] = e.sum(2)[live]
    return out


def check_head(c, out, twin=None):
    """twin: the outputs of the same launch with want_logits = 1 (needed where c stores no logits)"""
    res, rows, n, V, B = {}, c.rows, c.n, c.V, c.B
    inp, live = head_inputs(V, B), c.live_rows
    plant = planted_rows(B)
    nan_rows = torch.zeros(rows, dtype=torch.bool)
    nan_rows[[r for r, w in plant.items() if w == "nan"]] = True
    own = torch.zeros(rows + 32, dtype=torch.bool)
    own[:rows] = live
    logits = out["logits"]
    # guards: what no live row owns holds 0xFF, what one owns is finite (the NaN row apart)
    fin = own.clone()
    fin[:rows] &= ~nan_rows
    for name, on in (("logits", c.want_logits), ("cand_val", 1), ("cand_idx", 1), ("cand_sum", c.want_sum)):
        t = out[name]
        res["guard " + name] = _yes(_is_ff(t)[~own].all() and (on or _is_ff(t).all()))
        if on and t.dtype == torch.float32:
            res["finite " + name] = _yes(torch.isfinite(t[fin]).all())
    if c.want_logits:
        ok = live & ~nan_rows
        res["logits"] = G.miss(logits[:rows][ok], inp["ref"][ok], inp["tol"][ok])
        res["nan row"] = _yes(torch.isnan(logits[:rows][live & nan_rows]).all())
        src = logits[:rows]
    else:
        assert twin is not None, "a launch without logits is judged on the logits of its twin"
        src = twin["logits"][:rows]
        for name in ("cand_val", "cand_idx") + (("cand_sum",) if c.want_sum else ()):
            res[name + " == twin bits"] = _yes(_bits_equal(out[name], twin[name]))
    val, idx = tile_winner(src)
    res["cand_val bits"] = _yes(_bits_equal(out["cand_val"][:rows][live], val[live]))
    res["cand_idx"] = _yes(torch.equal(out["cand_idx"][:rows][live], idx[live]))
    if c.want_sum:
        ok = live & ~nan_rows
        s64, dmax = tile_sum64(src[ok])
        got = out["cand_sum"][:rows][ok].double()
        res["cand_sum"] = float(((got - s64).abs() / ((31 + 8 + dmax) * U * s64)).max())
        res["cand_sum nan row"] = _yes(torch.isnan(out["cand_sum"][:rows][live & nan_rows]).all())
        zero = [r for r, w in plant.items() if w == "zero" and bool(live[r])] + [r for r in range(B, rows) if bool(live[r])]
        res["cand_sum zero rows"] = _yes((out["cand_sum"][:rows][zero] == 32.0).all())
    # the row arg-max the partials give, in arg_better order, against float64 / the planted ties
    tok = row_winner(out["cand_val"][:rows], out["cand_idx"][:rows])
    cmp_rows = compared_rows(c)
    res["arg-max == float64"] = _yes(torch.equal(tok[cmp_rows], inp["ref"][cmp_rows].argmax(1).int()))
    for r, what in plant.items():
        if bool(live[r]) and what != "peaked":
            res[f"arg-max {what} row {r}"] = _yes(int(tok[r]) == (tie_cols(V)[0] if what == "tie" else 0))
        if bool(live[r]) and what == "peaked":
            res["arg-max peaked row"] = _yes(int(tok[r]) == PEAK_COL)
    return res


# ---- arg_better over a row's partials ------------------------------------------------------------------------------------------------------
def arg_better(v, i, bv, bi):
    """torch.argmax order: NaN compares as the maximum, the lowest index wins among equals (common.h)"""
    vn, bn = v != v, bv != bv
    if vn or bn:
        return vn and (not bn or i < bi)
    return v > bv or (v == bv and i < bi)


def row_winner(cand_val, cand_idx, with_value=False):
    """per row the arg_better winner of its (value, index) pairs, starting from (-inf, INT_MAX) -> i32 [R] (unclamped)"""
    v = cand_val.double().numpy()
    i = cand_idx.numpy().astype(np.int64)
    key_nan = np.isnan(v)
    out, vals = [], []
    for r in range(v.shape[0]):
        if key_nan[r].any():
            j = int(np.flatnonzero(key_nan[r])[np.argmin(i[r][key_nan[r]])])
        else:
            order = np.lexsort((i[r], -v[r]))
            j = int(order[0])
        if not key_nan[r].any() and v[r][j] == -np.inf and i[r][j] >= INT_MAX:
            out.append(INT_MAX)
        else:
            out.append(int(i[r][j]))
        vals.append(float(v[r][j]))
    t = torch.tensor(out, dtype=torch.int64).clamp(-2 ** 31, INT_MAX).int()
    return (t, torch.tensor(vals, dtype=torch.float64)) if with_value else t


# ---- arg-max: planted state, integer model, emulate, check ----------------------------------------------------------------------------------
MAX_LEN, STOP, T0 = 6, 77, 11


@functools.lru_cache(maxsize=None)
def planted(cid):
    """the planted inputs of an argmax / pack / load case (shared, read-only)"""
    c = case(cid)
    g = torch.Generator().manual_seed(zlib.crc32(cid.encode()))
    B, rows, RB, nm = c.B, c.rows, c.RB, c.name
    if c.kind == "load":
        if nm == "B70-Tlast3-ld600":
            return {"in": torch.randn(3 * B, 600, generator=g), "ld": 600, "n_src": 3 * B, "T_last": 3, "ids": None}
        n_src = 50
        ids = torch.randint(0, n_src, (B,), generator=g, dtype=torch.int32)
        if B >= 33:
            ids[5], ids[32], ids[7], ids[20] = -3, n_src + 5, 0, n_src - 1
        return {"in": torch.randn(n_src, HID, generator=g), "ld": HID, "n_src": n_src, "T_last": 0, "ids": ids}
    if c.kind == "pack":
        ros = torch.arange(rows, dtype=torch.int32)
        seen = torch.ones(rows, dtype=torch.int32)
        live = torch.ones(RB, dtype=torch.int32)
        act = []
        if nm == "B64-5-in-block1":
            act = [33, 40, 41, 55, 63]
        elif nm == "B96-101-holes":
            live = torch.tensor([1, 0, 1], dtype=torch.int32)
            ros = torch.randperm(rows, generator=g).int()
            act = [0, 3, 4, 17, 31, 64, 70, 71, 90, 95]
            seen[ros[40].item()] = 0                     # a running row in the stopped block: not active
            for hole in (2, 5, 66, 94):
                seen[ros[hole].item()] = 0               # the example is running, but no slot holds it any more
                ros[hole] = -1
        elif nm in ("B64-slots1to40", "B96-slots1to40"):
            act = list(range(1, 41))
        elif nm == "B1024-40-scattered":
            act = sorted({64 * w + 13 * w % 64 for w in range(16)} | {64 * w + 63 - w for w in range(16)} | {64 * w + 31 for w in range(0, 16, 2)})
            assert len(act) == 40 and len({a // 64 for a in act}) == 16
        elif nm == "B64-33-none":
            act = list(range(0, 64, 2)) + [63]
        for s in act:
            seen[ros[s].item()] = 0
        left = torch.tensor([sum(1 for s in act if s // 32 == k) for k in range(RB)], dtype=torch.int32)
        return {"ros": ros, "seen": seen, "live": live, "left": left, "x": torch.randn(B, HID, generator=g), "ncomp": 3, "act": act}
    # argmax
    n = c.n
    val = torch.randn(B, n, generator=g) * 3.0
    idx = (torch.arange(n, dtype=torch.int32) * 32)[None, :] + torch.randint(0, 32, (B, n), generator=g, dtype=torch.int32)
    cs = 1.0 + 31.0 * torch.rand(B, n, generator=g)
    p = {"val": val, "idx": idx, "sum": cs if "-lp" in nm else None, "embed": torch.randn(32 * n, HID, generator=g), "write_x": int(nm.endswith("-x")),
         "with_logprob": int("-lp" in nm), "state": None, "seen": None, "left": None, "live": None, "snap": None, "ros": None}

    def win(b, tile, token=None, v=50.0):
        val[b, tile] = v
        if token is not None:
            idx[b, tile] = token
    if "noloop" in nm:
        if B == 33:                                        # n = 264: the stride loop runs a second round (tiles 256 ..)
            val[1, 5], val[1, 200] = float("nan"), float("nan")                  # two NaNs: the lower index wins
            idx[1, 5], idx[1, 200] = 6000, 170
            win(2, 10, v=40.0), win(2, 70, v=40.0), win(2, 140, v=40.0)           # a tie across waves (threads 10, 70, 140)
            win(3, 260, v=40.0), win(3, 4, 9000, v=40.0)                          # a tie across the stride: thread 4 holds tiles 4 and 260
            val[4] = -INF                                                          # nothing beats the start value's -inf but the index
            idx[4] = INT_MAX
            val[5] = -INF
            win(6, 100, -5)                                                        # an index below the table: clamped to 0
            win(7, 263, 264 * 32 + 9)                                              # ... and above: clamped to 32 n - 1
        return p
    col = {"col0": 0, "colm1": -1, "collast": MAX_LEN - 1, "colmax": MAX_LEN}.get(nm.split("-")[2], 2)
    p["state"] = {"max_len": MAX_LEN, "stop_id": STOP, "T0": T0, "pos": T0 - 1 + col, "n_seen": 4, "arrive": 0, "ticket": 41}
    seen = torch.zeros(rows, dtype=torch.int32)
    if nm.startswith("B3-"):
        win(0, 2, STOP)                                    # a fresh row hits the stop id in every column case
        seen[1] = 1
        win(1, 2, STOP)                                    # ... and a row that had stopped hits it again
    elif nm == "B33-n8-stops":
        seen[[3, 9]] = 1
        for b in (3, 4, 32):
            win(b, 2, STOP)                                # 3 had stopped; 4 and 32 are fresh
        val[6, 3] = float("nan")
        val[7] = -INF
    else:
        ros = torch.arange(rows, dtype=torch.int32)
        if "slots" in nm:
            ros = torch.randperm(rows, generator=g).int()
            ros[[6, 30, 65]] = -1
        blk2 = [b for b in range(64, B) if ros[b] >= 0]
        for b in blk2[:-2]:
            seen[ros[b].item()] = 1                        # all of block 2 but its last two rows had stopped ...
        for b in blk2[-2:]:
            win(b, 1, STOP)                                # ... and those two stop in this launch
        b0 = [b for b in range(32) if ros[b] >= 0]
        for b in b0:
            if b not in (b0[5], b0[7]):
                seen[ros[b].item()] = 1                    # block 0: two rows are still running
        win(b0[3], 1, STOP)                                # a stopped row of block 0 repeats the stop id
        win(b0[5], 1, STOP)                                # a running one hits it: blk_left 2 -> 1, the block stays live
        win(40, 1, STOP)                                   # a slot of the dead block: nothing of it may show
        left0 = sum(1 for b in b0 if seen[ros[b].item()] == 0)
        p.update(ros=ros if "slots" in nm else None, left=torch.tensor([left0, 0, 2], dtype=torch.int32), live=torch.tensor([1, 0, 1], dtype=torch.int32),
                 snap=torch.tensor([1, 0, 1], dtype=torch.int32))
        if n > 256:
            win(10, 260, v=60.0), win(10, 4, 8000, v=60.0)     # a tie across the stride inside a live row
    p["seen"] = seen
    return p


ARGMAX_MUTANTS = ("col_minus_1", "record_by_slot", "stop_twice", "live_at_1", "dead_no_arrival", "arrive_kept", "gather_src_row", "gather_dst_row")


def argmax_model(c, p, mutant=None, dtype=F64):
    """the step epilogue in plain Python -> dict of the tap's raw outputs (float outputs in `dtype`: F64 the yardstick, F32 the
    emulation).  Transcribed from the comments of step_tail.h / kernels.h (module docstring)."""
    B, rows, n = c.B, c.rows, c.n
    st = p["state"]
    tokens = np.full(rows + 32, -1, dtype=np.int32)
    xrows = {}                                             # slot -> embedding row gathered there
    out = {"tokens": tokens}
    win, M = row_winner(p["val"], p["idx"], with_value=True)
    tok_of = win.long().clamp(0, 32 * n - 1)
    if st is not None:
        max_len, step = st["max_len"], st["pos"] - st["T0"] + 1
        if mutant == "col_minus_1":
            step -= 1
        rec = np.full((rows, max_len), -1, dtype=np.int32)
        lp = np.full((rows, max_len), np.nan)
        lp_set = np.zeros((rows, max_len), dtype=bool)
        seen = p["seen"].clone().numpy()
        n_seen, arrive, ticket = st["n_seen"], st["arrive"], st["ticket"]
        left = None if p["left"] is None else p["left"].clone().numpy()
        live = None if p["live"] is None else p["live"].clone().numpy()
    for b in range(B):
        row = b if p["ros"] is None else int(p["ros"][b])
        dead = (p["snap"] is not None and int(p["snap"][b >> 5]) == 0) or row < 0
        if not dead:
            t = int(tok_of[b])
            tokens[b] = t
            if p["write_x"]:
                src = row if mutant == "gather_src_row" else t
                xrows[row if mutant == "gather_dst_row" else b] = p["embed"][src]
            if st is not None:
                r = b if mutant == "record_by_slot" else row
                if 0 <= step < max_len:
                    rec[r, step] = t
                    if p["with_logprob"]:
                        m, s = p["val"][b].to(dtype), p["sum"][b].to(dtype)
                        Mb = M[b].to(dtype)
                        S = torch.where(m > -INF, s * torch.exp(m - Mb), torch.zeros_like(s)).sum()
                        lp[r, step] = float(-torch.log(S.double())) if np.isfinite(float(M[b])) else np.nan
                        lp_set[r, step] = True
                if t == st["stop_id"] and (seen[row] == 0 or mutant == "stop_twice"):
                    seen[row] = 1
                    n_seen += 1
                    if left is not None:
                        left[b >> 5] -= 1
                        if left[b >> 5] == (1 if mutant == "live_at_1" else 0):
                            live[b >> 5] = 0
        if st is not None and not (dead and mutant == "dead_no_arrival"):
            arrive += 1
    out["x_rows"] = xrows
    if st is not None:
        published = arrive == B
        out.update(record=rec, logprob=lp, logprob_set=lp_set, seen_stop=seen, n_seen=n_seen, blk_left=left, blk_live=live,
                   arrive=0 if published and mutant != "arrive_kept" else arrive, ticket=ticket + 1 if published else ticket,
                   progress=((ticket + 1) << 32 | n_seen) if published else -1)
    return out


def lp_tolerance(c, p, lp64):
    """-log S: the relative tolerance of S plus 2^-24 |log S| (module docstring)"""
    return (-(-c.n // 256) + 6 + 3 + 1 + 8) * U + U * np.abs(lp64)


def _x_image(rows, xrows, base=None):
    """raw f32 [(rows + 32) * 576]: 0xFF (or `base`, the rows sent) with the rows of the dict written in F32-layout"""
    img = _ff(((rows + 32) * HID,)) if base is None else base.copy()
    idx = D.f32_index(rows)
    for slot, v in xrows.items():
        img[idx[slot]] = v.float().numpy()
    return img


def _words(rows, seen=None, left=None, live=None, ros=None):
    """the planted int32 arrays as the tap returns them: margins of 0xFF, zeros behind RB in the block words"""
    o = {"seen_stop": np.full(rows + 32, -1, dtype=np.int32), "blk_left": np.full(64, -1, dtype=np.int32), "blk_live": np.full(64, -1, dtype=np.int32),
         "row_of_slot": np.full(rows + 32, -1, dtype=np.int32)}
    if seen is not None:
        o["seen_stop"][:rows] = np.asarray(seen)
    for name, t in (("blk_left", left), ("blk_live", live)):
        if t is not None:
            o[name][:32] = 0
            o[name][:len(t)] = t.numpy() if torch.is_tensor(t) else t
    if ros is not None:
        o["row_of_slot"][:rows] = ros.numpy() if torch.is_tensor(ros) else ros
    return o


def emulate_argmax(c, mutant=None):
    p = planted(c.id)
    st = p["state"]
    in_record = st is not None and 0 <= st["pos"] - st["T0"] + 1 <= st["max_len"]          # (the column, or the one before it, exists)
    applies = {None: True, "col_minus_1": in_record, "record_by_slot": p["ros"] is not None, "stop_twice": st is not None,
               "live_at_1": p["left"] is not None, "dead_no_arrival": p["snap"] is not None, "arrive_kept": st is not None,
               "gather_src_row": bool(p["write_x"]), "gather_dst_row": bool(p["write_x"]) and p["ros"] is not None}[mutant]
    if not applies:
        return None
    m = argmax_model(c, p, mutant, F32)
    out = {"tokens": torch.from_numpy(m["tokens"]), "x": torch.from_numpy(_x_image(c.rows, m["x_rows"]))}
    if st is not None:
        w = _words(c.rows, m["seen_stop"], m["blk_left"], m["blk_live"], p["ros"])
        out.update({k: torch.from_numpy(v) for k, v in w.items()})
        out.update(record=torch.from_numpy(m["record"]), n_seen=m["n_seen"], arrive=m["arrive"], ticket=m["ticket"], progress=m["progress"],
                   n_compactions=-1)
        if p["with_logprob"]:
            lp = _ff(m["record"].shape)
            lp[m["logprob_set"]] = m["logprob"][m["logprob_set"]].astype(np.float32)
            out["logprob"] = torch.from_numpy(lp)
    return out


def check_argmax(c, out):
    p = planted(c.id)
    m = argmax_model(c, p)
    res = {"tokens": _yes(torch.equal(torch.as_tensor(out["tokens"]), torch.from_numpy(m["tokens"])))}      # 0xFF at dead slots and beyond B
    res["x rows and guard"] = _yes(_bits_equal(out["x"], torch.from_numpy(_x_image(c.rows, m["x_rows"]))))
    if p["state"] is None:
        return res
    w = _words(c.rows, m["seen_stop"], m["blk_left"], m["blk_live"], p["ros"])
    for name, t in w.items():
        res[name] = _yes(torch.equal(torch.as_tensor(out[name]), torch.from_numpy(t)))
    res["record"] = _yes(torch.equal(torch.as_tensor(out["record"]), torch.from_numpy(m["record"])))
    for name in ("n_seen", "arrive", "ticket", "progress"):
        res[name] = _yes(int(out[name]) == int(m[name]))
    res["n_compactions untouched"] = _yes(int(out["n_compactions"]) == -1)
    if p["with_logprob"]:
        got, own = torch.as_tensor(out["logprob"]), torch.from_numpy(m["logprob_set"])
        res["guard logprob"] = _yes(_is_ff(got)[~own].all())
        ref = torch.from_numpy(m["logprob"])[own]
        g = got[own].double()
        nan = torch.isnan(ref)
        res["logprob nan"] = _yes(torch.isnan(g[nan]).all())
        if bool((~nan).any()):
            tol = torch.from_numpy(lp_tolerance(c, p, ref[~nan].numpy()))
            res["logprob"] = float(((g[~nan] - ref[~nan]).abs() / tol).max())
    return res


# ---- repack -------------------------------------------------------------------------------------------------------------------------------------
PACK_MUTANTS = ("unstable", "always_move", "left_off_32")


def pack_model(c, p, mutant=None):
    B, rows, RB = c.B, c.rows, c.RB
    ros, seen, live, left = (p[k].clone().numpy() for k in ("ros", "seen", "live", "left"))
    act = [s for s in range(B) if ros[s] >= 0 and live[s >> 5] != 0 and seen[ros[s]] == 0]
    n_act, n_live = len(act), int((live != 0).sum())
    x_rows, ncomp = {}, p["ncomp"]
    if -(-n_act // 32) < n_live or mutant == "always_move":
        src = act[::-1] if mutant == "unstable" else act
        new = np.full(B, -1, dtype=np.int32)
        for d, s in enumerate(src):
            new[d] = ros[s]
            x_rows[d] = p["x"][s]
        ros[:B] = new
        off = 32 if mutant == "left_off_32" else 0
        left = np.array([min(max(n_act - 32 * k - off, 0), 32) for k in range(RB)], dtype=np.int32)
        live = (left > 0).astype(np.int32)
        ncomp += 1
    return {"ros": ros, "seen": seen, "live": live, "left": left, "x_rows": x_rows, "ncomp": ncomp, "n_act": n_act, "moved": bool(x_rows) or ncomp != p["ncomp"]}


def _pack_raw(c, p, m):
    base = _ff(((c.rows + 32) * HID,))
    xs = torch.zeros(c.rows, HID)
    xs[:c.B] = p["x"]
    base[D.f32_index(c.rows).reshape(-1)] = xs.numpy().reshape(-1)
    out = {k: torch.from_numpy(v) for k, v in _words(c.rows, m["seen"], m["left"], m["live"], m["ros"]).items()}
    out.update(x=torch.from_numpy(_x_image(c.rows, m["x_rows"], base)), n_compactions=m["ncomp"], n_seen=-1, arrive=-1, ticket=-1)
    return out


def emulate_pack(c, mutant=None):
    p = planted(c.id)
    base = pack_model(c, p)
    applies = {None: True, "unstable": base["moved"] and base["n_act"] > 1, "always_move": not base["moved"], "left_off_32": base["moved"] and base["n_act"] > 0}[mutant]
    return _pack_raw(c, p, pack_model(c, p, mutant)) if applies else None


def check_pack(c, out):
    p = planted(c.id)
    ref = _pack_raw(c, p, pack_model(c, p))
    res = {name: _yes(torch.equal(torch.as_tensor(out[name]), ref[name])) for name in ("seen_stop", "blk_left", "blk_live", "row_of_slot")}
    res["x rows and guard"] = _yes(_bits_equal(out["x"], ref["x"]))
    res["n_compactions"] = _yes(int(out["n_compactions"]) == ref["n_compactions"])
    res["other scalars untouched"] = _yes(all(int(out[k]) == -1 for k in ("n_seen", "arrive", "ticket")))
    return res


# ---- load ---------------------------------------------------------------------------------------------------------------------------------------
LOAD_MUTANTS = ("no_low_clamp",)


def emulate_load(c, mutant=None):
    p = planted(c.id)
    if mutant == "no_low_clamp" and (p["ids"] is None or int(p["ids"].min()) >= 0):
        return None
    rows_of = {}
    for b in range(c.B):
        if p["ids"] is None:
            s = b * p["T_last"] + p["T_last"] - 1
        else:
            s = min(int(p["ids"][b]), p["n_src"] - 1)
            s = s % p["n_src"] if mutant == "no_low_clamp" else max(s, 0)       # (a negative id read as some other row of the table)
        rows_of[b] = p["in"][s, :HID]
    return {"x": torch.from_numpy(_x_image(c.rows, rows_of))}


def check_load(c, out):
    return {"x rows and guard": _yes(_bits_equal(out["x"], emulate_load(c)["x"]))}


# ---- one entry for every kind -------------------------------------------------------------------------------------------------------------------
MUTANTS = {
    "kpair": "1. one k-pair dropped in one phase",
    "phase_swap": "2. two phases' k-ranges exchanged",
    "tail_fill": "3. the tail pass filled from block rb0 + g for g >= gn (benign: must NOT be caught)",
    "half_tie": "4. the half-tile exchange keeps the higher index on a tie",
    "sum_rowmax": "5. cand_sum relative to the row maximum",
    "sum_half": "6. the partner's sum left out",
    "dead_rows": "7. a dead block's rows written",
    "col_minus_1": "8. the token recorded at column step - 1",
    "record_by_slot": "9. the record addressed by slot",
    "stop_twice": "10. a repeated stop counted twice",
    "live_at_1": "11. blk_live cleared when blk_left reaches 1",
    "dead_no_arrival": "12. a dead slot not counted as arrived",
    "arrive_kept": "13. arrive not reset",
    "gather_src_row": "14a. the gather from embed[row]",
    "gather_dst_row": "14b. the gather into the example's row",
    "unstable": "15. the repack unstable",
    "always_move": "16. the repack moves when it empties no block",
    "left_off_32": "17. blk_left off by 32",
    "no_low_clamp": "18. the load id unclamped on the low side",
}
BENIGN = ("tail_fill",)
_KIND_OF = {**{m: "head" for m in HEAD_MUTANTS}, **{m: "argmax" for m in ARGMAX_MUTANTS}, **{m: "pack" for m in PACK_MUTANTS},
            **{m: "load" for m in LOAD_MUTANTS}}


def emulate(c, mutant=None):
    """what the tap returns for case c when the launch computes the float32 evaluation of the reference (or of a mutant of it), or None
    where the mutant does not apply to the case"""
    if mutant is not None and _KIND_OF[mutant] != c.kind:
        return None
    return {"head": emulate_head, "argmax": emulate_argmax, "pack": emulate_pack, "load": emulate_load}[c.kind](c, mutant)


def check(c, out, twin=None):
    """judge the raw outputs of case c's launch -> dict name -> err / tol (exact statements and guards: 0 or inf).  A launch is right
    when every figure is <= 1."""
    if c.kind == "head":
        return check_head(c, out, twin)
    return {"argmax": check_argmax, "pack": check_pack, "load": check_load}[c.kind](c, out)


def worst(res):
    """the largest figure; a NaN figure counts as a miss"""
    return max(INF if v != v else v for v in res.values())


def head_args(c, x=None):
    """keyword arguments of Engine.debug_dec_tail for a head launch on the case's own rows, or on x [rows][576]"""
    x = head_inputs(c.V, c.B)["x"] if x is None else x
    kw = {"op": 0, "B": c.B, "form": c.form, "V": c.V, "W": head_weight(c.V), "want_logits": bool(c.want_logits), "want_sum": bool(c.want_sum),
          "blk_live": None if c.blk is None else torch.tensor(c.blk, dtype=torch.int32)}
    if c.form:
        kw["x_img"] = D.f3_encode(x, D.f3_32_index(c.rows))
    else:
        kw["x"] = x[:c.B]
    return kw


def tap_args(c):
    """the keyword arguments of Engine.debug_dec_tail for case c (host tensors)"""
    if c.kind == "head":
        return head_args(c)
    p = planted(c.id)
    if c.kind == "argmax":
        return {"op": 1, "B": c.B, "V": c.V, "cand_val": p["val"], "cand_idx": p["idx"], "cand_sum": p["sum"], "W": p["embed"] if p["write_x"] else None,
                "write_x": bool(p["write_x"]), "state": p["state"], "with_logprob": bool(p["with_logprob"]), "seen_stop": p["seen"],
                "blk_left": p["left"], "blk_live": p["live"], "blk_snap": p["snap"], "row_of_slot": p["ros"]}
    if c.kind == "pack":
        return {"op": 2, "B": c.B, "row_of_slot": p["ros"], "blk_live": p["live"], "blk_left": p["left"], "seen_stop": p["seen"], "x": p["x"],
                "n_compactions": p["ncomp"]}
    return {"op": 3, "B": c.B, "x": p["in"], "row_ids": p["ids"], "ld": p["ld"], "n_src": p["n_src"], "T_last": p["T_last"]}


if __name__ == "__main__":
    for c_ in CASES:
        print(c_.id)
