"""The debug_* methods of Engine: thin wrappers of the library's launch taps and GEMM / lm_head taps (include/mellow_hip.h,
csrc/engine_taps.cpp, csrc/engine_dev.cpp).  Not used by the product path.  DebugTaps is a mixin: it needs the lib, h, tdev, lm,
_chk, _need and _sync_inputs of the Engine that inherits it.  The descriptor structures live in engine.py (imported where they are
filled in, because engine.py imports this module)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch


# ---- what every wrapper does with its tensors ------------------------------------------------------------------------------------
def _host(t, dtype=None):
    """t (or None) as a contiguous host tensor, converted to dtype if one is given"""
    if t is None:
        return None
    t = torch.as_tensor(t).detach().cpu().contiguous()
    return t if dtype is None else t.to(dtype)


def _f32(t):
    return _host(t, torch.float32)


def _i32(t):
    return _host(t, torch.int32)


def _p(t):
    """the address of t, or None"""
    return None if t is None else C.c_void_p(t.data_ptr())


def _nb(t) -> int:
    """bytes of t, 0 for None"""
    return 0 if t is None else t.numel() * t.element_size()


def _check_shapes(*items):
    """items (name, tensor or None, shape or None): every tensor given has the shape given"""
    for name, t, shape in items:
        if t is not None and shape is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name} {tuple(t.shape)} is not {shape}")


def _outs(out: dict):
    """-> (o, nb): the address and the byte count of out.get(key)"""
    return (lambda k: _p(out.get(k))), (lambda k: _nb(out.get(k)))


def _alloc(*specs) -> dict:
    """specs (key, wanted, dtype, shape): the host tensors of the outputs the launch writes, by key"""
    return {key: torch.empty(shape, dtype=dtype) for key, wanted, dtype, shape in specs if wanted}


def _attn_out(M: int, width: int, out_form: int) -> torch.Tensor:
    """the host buffer an attention tap fills: fp32 [M + 32][width], or the APB image of roundup(M, 128) rows as int32 words"""
    if out_form == 0:
        return torch.empty((M + 32, width), dtype=torch.float32)
    return torch.empty(((M + 127) // 128 * 128 * width * 6 // 4,), dtype=torch.int32)


F32, I32, I16, U8 = torch.float32, torch.int32, torch.int16, torch.uint8


class DebugTaps:
    def _gemm_tap(self, fn, args_before, A, W, iters):
        A, W = _f32(A), _f32(W)
        (M, K), (N, K2) = A.shape, W.shape
        assert K == K2
        out = torch.empty((M, N), dtype=F32)
        ms = (C.c_float * 2)()
        self._chk(fn(self.h, *args_before, _p(A), M, K, _p(W), N, _p(out), int(iters), ms if iters > 0 else None))
        return out, ((ms[0], ms[1]) if iters > 0 else None)

    def debug_gemm_f32(self, A: torch.Tensor, W: torch.Tensor, mode: int = 0, iters: int = 0):
        """C = A . W^T through the exact fp32 MFMA kernel (mode 0) or one of the f32x3 kernels the default mode runs (16: A split in
        registers; 17: A pre-split in APB order, both operands by LDS-DMA); host tensors."""
        return self._gemm_tap(self.lib.mellow_debug_gemm_f32, (int(mode),), A, W, iters)

    def debug_gemm_fp8(self, A: torch.Tensor, W: torch.Tensor, iters: int = 0):
        """fp8 mode quantisation tap: (C = A . W^T through the e4m3 GEMM, (quant_ms, gemm_ms) or None); host tensors."""
        return self._gemm_tap(self.lib.mellow_debug_gemm_fp8, (), A, W, iters)

    def debug_gemm_epi(self, A, W, kernel: int = 0, epi: str = "linear", N: Optional[int] = None, act: str = "none", bias=None,
                       resid=None, in_place: bool = False, crow_map=None, rows_out: int = 0, ldc: Optional[int] = None,
                       want_c: bool = True, want_c3: bool = False, want_ssq: bool = False, rs_ssq=None, rs_dim: float = 1.0,
                       rs_eps: float = 0.0, splitk_max: int = 0, no_x3w: bool = False, T: int = 1, Tmax: int = 1, pos0: int = 0,
                       rope=None) -> dict:
        """One GEMM launch with the epilogue described (mellow_debug_gemm_epi): A [M][K], W [Nw][K] logical rows (swiglu: gate rows then
        up rows), host tensors.  epi "linear" | "swiglu" | "qkv_rope"; N stored columns (default: Nw rounded up to 4, Nw / 2 for
        swiglu); resid [C rows][N] with in_place choosing resid == C; crow_map int32 [rows_in] with rows_out; rope = (cos, sin)
        [Tmax][32] or None for the engine's own tables.  -> dict of the whole device outputs, which held 0xFF bytes before the launch:
        "c" f32 [C rows + 32][ldc], "c3" the raw APB image as int32 words, "ssq" f32 [M + 32][N / 64], "q" f32 [M + 32][576],
        "k" / "v" f32 [B + 1][3][Tmax][64]."""
        from .engine import GemmEpi
        self._need("mellow_debug_gemm_epi")
        A, W, bias, resid, rs_ssq, cmap = _f32(A), _f32(W), _f32(bias), _f32(resid), _f32(rs_ssq), _i32(crow_map)
        (M, K), Nw = A.shape, int(W.shape[0])
        assert W.shape[1] == K
        e = {"linear": 0, "swiglu": 1, "qkv_rope": 2}[epi]
        if N is None:
            N = Nw // 2 if e == 1 else (Nw + 3) // 4 * 4
        d = GemmEpi()
        d.size, d.kernel, d.epi, d.M, d.K, d.Nw, d.N = C.sizeof(GemmEpi), int(kernel), e, M, K, Nw, int(N)
        d.act, d.bias = {"none": 0, "gelu": 1, "sigmoid": 2}[act], 0 if bias is None else 1
        d.resid = 0 if resid is None else (2 if in_place else 1)
        c_rows = M
        if cmap is not None:
            d.rows_in, d.rows_out = int(cmap.numel()), int(rows_out)
            c_rows = M // max(1, d.rows_in) * d.rows_out
        d.ldc = int(N if ldc is None else ldc)
        d.want_c, d.want_c3, d.want_ssq = int(bool(want_c)), int(bool(want_c3)), int(bool(want_ssq))
        if rs_ssq is not None:
            d.rs_parts, d.rs_dim, d.rs_eps = int(rs_ssq.shape[1]), float(rs_dim), float(rs_eps)
        d.splitk_max, d.no_x3w, d.T, d.Tmax, d.pos0 = int(splitk_max), int(bool(no_x3w)), int(T), int(Tmax), int(pos0)
        cos, sin = (None, None) if rope is None else (_f32(rope[0]), _f32(rope[1]))
        pages = (M // max(1, d.T - d.pos0) + 1, 3, max(1, d.Tmax), 64)
        out = _alloc(("q", e == 2, F32, (M + 32, 576)), ("k", e == 2, F32, pages), ("v", e == 2, F32, pages),
                     ("c", e != 2 and want_c, F32, (c_rows + 32, max(1, d.ldc))),
                     ("c3", e != 2 and want_c3, I32, ((M + 127) // 128 * 128 * d.N * 6 // 4,)),
                     ("ssq", e != 2 and want_ssq, F32, (M + 32, max(1, d.N // 64))))
        o, nb = _outs(out)
        self._chk(self.lib.mellow_debug_gemm_epi(self.h, C.byref(d), _p(A), _p(W), _p(bias), _p(resid), _p(cmap), _p(rs_ssq), _p(cos), _p(sin),
                                                 o("c"), nb("c"), o("c3"), nb("c3"), o("ssq"), nb("ssq"), o("q"), nb("q"), o("k"), o("v"), nb("k")))
        return out

    def debug_norm(self, x, op: str = "layernorm", form: int = 0, w=None, b=None, eps: float = 1e-5, row_map=None, n: int = 0,
                   R: int = 0) -> dict:
        """One launch of a norm launcher or of a stand-alone hand-over producer on host rows (mellow_debug_norm).  op "layernorm"
        (x [M][C], optional row_map int32 [ntok]) | "merge" (x [n][R * R][C] -> n (R / 2)^2 rows of 4 C) | "rmsnorm" (eps) | "none"
        (launch_split_rows_apb / launch_quant_mx8 on x itself).  form 0 fp32 rows, 1 APB image, 2 AMX image + scale bytes.  -> dict
        of the whole device outputs, which held 0xFF bytes before the launch: "y" f32 [M + 32][columns], or "apb" the raw image as
        int32 words, or "amx" uint8 [roundup(M, 128) * roundup(C, 64)] plus "scales" uint8 [roundup(M, 128) * 8 * KQ]."""
        self._need("mellow_debug_norm")
        x, w, b, rmap = _f32(x), _f32(w), _f32(b), _i32(row_map)
        o, form = {"layernorm": 0, "merge": 1, "rmsnorm": 2, "none": 3}[op], int(form)
        Cc = int(x.shape[-1])
        if o == 1:
            if x.dim() != 3 or x.shape[0] != n or x.shape[1] != R * R:
                raise ValueError(f"x {tuple(x.shape)} is not [n = {n}][R * R = {R * R}][C]")
            M, width = int(n) * (int(R) // 2) ** 2, 4 * Cc
        else:
            if x.dim() != 2:
                raise ValueError(f"x {tuple(x.shape)} is not [M][C]")
            M, width = int(x.shape[0]), Cc
        for name, v in (("w", w), ("b", b)):
            if v is not None and v.numel() != width:
                raise ValueError(f"{name} has {v.numel()} elements for {width} columns")
        Mp, kt64, amx = (max(M, 0) + 127) // 128 * 128, (Cc + 63) // 64, form not in (0, 1)
        out = _alloc(("y", form == 0, F32, (max(M, 0) + 32, width)), ("apb", form == 1, I32, (Mp * Cc * 6 // 4,)),
                     ("amx", amx, U8, (Mp * kt64 * 64,)), ("scales", amx, U8, (Mp * 8 * ((kt64 + 3) // 4),)))
        main = out.get("y", out.get("apb", out.get("amx")))
        self._chk(self.lib.mellow_debug_norm(self.h, o, form, _p(x), M, Cc, _p(w), _p(b), float(eps), _p(rmap),
                                             0 if rmap is None else int(rmap.numel()), int(n), int(R), _p(main), _nb(main),
                                             _p(out.get("scales")), _nb(out.get("scales"))))
        return out

    def debug_dec_attn(self, slabs, x_res, k_pages, v_pages, pos: int, ctx_end: int, ts: int, fused: bool = False, kv16: bool = False,
                       ssq1=None, down=None, rope_cur=None, eps: float = 1e-5, blk_live=None, row_of_slot=None, Wo=None,
                       want_x3: bool = False) -> dict:
        """One launch of the decode attention and, with Wo, one of the o_proj that merges its key splits (mellow_debug_dec_attn), on host
        tensors: slabs [8 | 6][B][960], x_res [B][576] (fused: x_mid, else x_new), k / v pages [P][3][Tmax][64], ssq1 [B][8] (not fused),
        down [4][B][576] (fused), rope_cur [64] or None, blk_live int32 [RB], row_of_slot int32 [rows], Wo [576][576].  -> dict of the
        whole device outputs, which held 0xFF bytes before the launches: "gs" (4-key groups per split), "att" f32 [ts * rows * 576 + 32
        * 576] (F16-layout partials + one block), "ml" f32 [9][rows][ts][2], "k" / "v" the pages [P + 1][3][Tmax][64] (f32, or int16
        words with kv16), "xnew" f32 [rows + 32][576]; with Wo "xmid" f32 [rows * 576] (F32-layout), "x16" f32 [rows * 576] (F16-layout)
        or with want_x3 int16 [2][rows * 576 * 3] (F3-32 image, F3-16 image), "ssq" f32 [rows + 32][40]."""
        from .engine import DecAttn
        self._need("mellow_debug_dec_attn")
        slabs, x_res, k_pages, v_pages, ssq1, down, rope_cur, Wo = (_f32(t) for t in (slabs, x_res, k_pages, v_pages, ssq1, down, rope_cur, Wo))
        blk_live, row_of_slot = _i32(blk_live), _i32(row_of_slot)
        B = int(x_res.shape[0])
        if k_pages.dim() != 4 or k_pages.shape[1] != 3 or k_pages.shape[3] != 64 or v_pages.shape != k_pages.shape:
            raise ValueError(f"k {tuple(k_pages.shape)} / v {tuple(v_pages.shape)} are not pages [P][3][Tmax][64]")
        Pn, Tmax = int(k_pages.shape[0]), int(k_pages.shape[2])
        if tuple(slabs.shape) != (6 if fused else 8, B, 960) or tuple(x_res.shape) != (B, 576):
            raise ValueError(f"slabs {tuple(slabs.shape)} / x_res {tuple(x_res.shape)} are not [{6 if fused else 8}][B][960] / [B][576]")
        _check_shapes(("ssq1", ssq1, (B, 8)), ("down", down, (4, B, 576)), ("rope_cur", rope_cur, (64,)), ("Wo", Wo, (576, 576)))
        rows = (max(B, 1) + 31) // 32 * 32
        for name, t, n in (("blk_live", blk_live, rows // 32), ("row_of_slot", row_of_slot, rows)):
            if t is not None and t.numel() != n:
                raise ValueError(f"{name} has {t.numel()} entries for {n}")
        d = DecAttn()
        d.size, d.B, d.P, d.pos, d.Tmax, d.ctx_end = C.sizeof(DecAttn), B, Pn, int(pos), Tmax, int(ctx_end)
        d.ts, d.fused, d.kv16, d.want_x3, d.eps = int(ts), int(bool(fused)), int(bool(kv16)), int(bool(want_x3)), float(eps)
        n_x, tsn = rows * 576, max(int(ts), 1)
        kv, o_proj = (I16 if kv16 else F32, (Pn + 1, 3, Tmax, 64)), Wo is not None
        out = _alloc(("att", True, F32, (tsn * n_x + 32 * 576,)), ("ml", True, F32, (9, rows, tsn, 2)), ("k", True) + kv, ("v", True) + kv,
                     ("xnew", True, F32, (rows + 32, 576)), ("xmid", o_proj, F32, (n_x,)),
                     ("x16", o_proj) + ((I16, (2, n_x * 3)) if want_x3 else (F32, (n_x,))), ("ssq", o_proj, F32, (rows + 32, 40)))
        o, nb = _outs(out)
        gs = C.c_int32(0)
        self._chk(self.lib.mellow_debug_dec_attn(self.h, C.byref(d), _p(slabs), _p(ssq1), _p(x_res), _p(down), _p(rope_cur), _p(k_pages),
                                                 _p(v_pages), _p(blk_live), _p(row_of_slot), _p(Wo), C.cast(C.byref(gs), C.c_void_p),
                                                 o("att"), nb("att"), o("ml"), nb("ml"), o("k"), o("v"), nb("k"), o("xnew"), nb("xnew"),
                                                 o("xmid"), nb("xmid"), o("x16"), nb("x16"), o("ssq"), nb("ssq")))
        out["gs"] = int(gs.value)
        return out

    def debug_dec_gemv(self, op: int, B: int, W, W2=None, form: int = 0, x=None, down=None, h=None, x_img=None, h_img=None, ssq=None,
                       kcd: int = 0, first: bool = False, inc_pos: bool = False, pos: int = 0, Tmax: int = 0, rope_cos=None, rope_sin=None,
                       blk_live=None, want_x3: bool = False, eps: float = 1e-5) -> dict:
        """One launch of a decode layer's q/k/v (op 0), gate/up (1), down (2), fused down + q/k/v (3) launcher or of the final norm (4)
        on host tensors (mellow_debug_dec_gemv; form 1 = the f32x3 kernel of ops 1 and 3).  Weights logical row-major: op 0 W = W'
        [960][576]; op 1 W / W2 = gate / up [1536][576]; op 2 W = Wd [576][1536]; op 3 W = W', W2 = Wd; op 4 W = the norm vector.  x
        [B][576], down [8][B][576] (kcd 8), h [B][1536] row-major; x_img / h_img / ssq raw images of all rows (int16 words for the
        F3 triples).  -> dict of the whole device outputs, which held 0xFF bytes before the launch: "pq" f32 [8 * rows + 32][960],
        "down" f32 [8 * rows * 576 + 32 * 576] (F32-layout slabs), "ssq1" [rows + 32][8], "xnew" [rows + 32][576], "rope" [128], "pos",
        "gu" f32 [(rows + 32) * 1536] (F32-layout, 192 k-tiles), "h3" int16 [(rows + 32) * 1536 * 3], "xn" f32 [(rows + 32) * 576] or
        with want_x3 int16 [(rows + 32) * 576 * 3], "snap" int32 [64], "q" f32 [960][1536] -- those the op writes."""
        from .engine import DecGemv
        self._need("mellow_debug_dec_gemv")
        W, W2, x, down, h, ssq, rope_cos, rope_sin = (_f32(t) for t in (W, W2, x, down, h, ssq, rope_cos, rope_sin))
        x_img, h_img, blk_live = _host(x_img), _host(h_img), _i32(blk_live)
        op, form, B = int(op), int(form), int(B)
        rows = (max(B, 1) + 31) // 32 * 32
        wshape = {0: ((960, 576), None), 1: ((1536, 576), (1536, 576)), 2: ((576, 1536), None), 3: ((960, 576), (576, 1536)), 4: ((576,), None)}
        _check_shapes(("W", W, wshape.get(op, (None, None))[0]), ("W2", W2, wshape.get(op, (None, None))[1]), ("x", x, (B, 576)),
                      ("down", down, (8, B, 576)), ("h", h, (B, 1536)), ("ssq", ssq, (rows, 40)), ("rope_cos", rope_cos, (int(Tmax), 32)),
                      ("rope_sin", rope_sin, (int(Tmax), 32)), ("blk_live", blk_live, (rows // 32,)))
        d = DecGemv()
        d.size, d.op, d.form, d.B, d.kcd, d.first, d.inc_pos = C.sizeof(DecGemv), op, form, B, int(kcd), int(bool(first)), int(bool(inc_pos))
        d.pos, d.Tmax, d.want_x3, d.eps = int(pos), int(Tmax), int(bool(want_x3)), float(eps)
        n_x, n_h = (rows + 32) * 576, (rows + 32) * 1536
        out = _alloc(("pq", op in (0, 3), F32, (8 * rows + 32, 960)), ("down", op in (2, 3), F32, (8 * rows * 576 + 32 * 576,)),
                     ("ssq1", op == 0, F32, (rows + 32, 8)), ("xnew", op == 0, F32, (rows + 32, 576)), ("rope", op == 0, F32, (128,)),
                     ("pos", op == 0, I32, (1,)), ("gu", op == 1, F32, (n_h,)), ("h3", op == 1 and form, I16, (n_h * 3,)),
                     ("q", op == 3, F32, (960, 1536)), ("xn", op == 4) + ((I16, (n_x * 3,)) if want_x3 else (F32, (n_x,))),
                     ("snap", op == 4 and blk_live is not None, I32, (64,)))
        o, nb = _outs(out)
        self._chk(self.lib.mellow_debug_dec_gemv(self.h, C.byref(d), _p(W), _p(W2), _p(x), _p(down), _p(h), _p(x_img), _nb(x_img), _p(h_img),
                                                 _nb(h_img), _p(ssq), _p(rope_cos), _p(rope_sin), _p(blk_live), o("pq"), nb("pq"), o("down"),
                                                 nb("down"), o("ssq1"), nb("ssq1"), o("xnew"), nb("xnew"), o("rope"), o("pos"), o("gu"), nb("gu"),
                                                 o("h3"), nb("h3"), o("xn"), nb("xn"), o("snap"), o("q"), nb("q")))
        if "pos" in out:
            out["pos"] = int(out["pos"][0])
        return out

    def debug_dec_tail(self, op: int, B: int, form: int = 0, V: int = 0, W=None, x=None, x_img=None, blk_live=None, want_logits: bool = False,
                       want_sum: bool = False, cand_val=None, cand_idx=None, cand_sum=None, write_x: bool = False, state=None,
                       with_logprob: bool = False, seen_stop=None, blk_left=None, blk_snap=None, row_of_slot=None, n_compactions: int = 0,
                       row_ids=None, ld: int = 0, n_src: int = 0, T_last: int = 0) -> dict:
        """One launch of the decode step's lm_head (op 0; form 1 = the streaming f32x3 kernel), arg-max (1), row repack (2) or row load
        (3) launcher on host tensors (mellow_debug_dec_tail).  op 0: W [V][576] logical, x [B][576] (form 0) or x_img the raw F3-32
        image of all rows (form 1, int16 words), blk_live [RB].  op 1: cand_val / cand_idx / cand_sum [B][V / 32], W = the embedding
        table with write_x, state = None (LoopArgs()) or a dict {max_len, stop_id, T0, pos, n_seen, arrive, ticket} with seen_stop
        [rows], blk_left / blk_live / blk_snap [RB], row_of_slot [rows].  op 2: row_of_slot, blk_live, blk_left, seen_stop, x [B][576],
        n_compactions.  op 3: x = the source rows [n_src][ld], row_ids [B] or T_last.  -> dict of the whole device outputs, which held
        0xFF bytes before the launch: "logits" f32 [rows + 32][V], "cand_val" f32 / "cand_idx" i32 / "cand_sum" f32 [rows + 32][V / 32];
        "tokens" i32 [rows + 32], "record" i32 / "logprob" f32 [rows][max_len], "progress" (the published word as an int); "seen_stop"
        [rows + 32], "n_seen", "arrive", "ticket", "n_compactions", "scalars" [32], "blk_left" / "blk_live" [64], "row_of_slot"
        [rows + 32]; "x" f32 [(rows + 32) * 576] (F32-layout) -- those the op writes."""
        from .engine import DecTail
        self._need("mellow_debug_dec_tail")
        W, x, cand_val, cand_sum, x_img = _f32(W), _f32(x), _f32(cand_val), _f32(cand_sum), _host(x_img)
        blk_live, cand_idx, seen_stop, blk_left, blk_snap, row_of_slot, row_ids = (_i32(t) for t in (blk_live, cand_idx, seen_stop, blk_left,
                                                                                                    blk_snap, row_of_slot, row_ids))
        op, form, B, V = int(op), int(form), int(B), int(V)
        rows = (max(B, 1) + 31) // 32 * 32
        n = max(V, 0) // 32
        src_shape = (int(n_src), int(ld)) if op == 3 else (B, 576)
        _check_shapes(("W", W, (V, 576)), ("x", x, src_shape), ("cand_val", cand_val, (B, n)), ("cand_idx", cand_idx, (B, n)),
                      ("cand_sum", cand_sum, (B, n)), ("blk_live", blk_live, (rows // 32,)), ("blk_left", blk_left, (rows // 32,)),
                      ("blk_snap", blk_snap, (rows // 32,)), ("seen_stop", seen_stop, (rows,)), ("row_of_slot", row_of_slot, (rows,)),
                      ("row_ids", row_ids, (B,)))
        st = dict(state or {})
        d = DecTail()
        d.size, d.op, d.form, d.B, d.V = C.sizeof(DecTail), op, form, B, V
        d.want_logits, d.want_sum, d.write_x = int(bool(want_logits)), int(bool(want_sum)), int(bool(write_x))
        d.with_state, d.with_logprob = int(state is not None), int(bool(with_logprob))
        for k in ("max_len", "stop_id", "T0", "pos", "n_seen", "arrive", "ticket"):
            setattr(d, k, int(st.pop(k, 0)))
        if st:
            raise ValueError(f"state has unknown keys {sorted(st)}")
        d.n_compactions, d.ld, d.n_src, d.T_last = int(n_compactions), int(ld), int(n_src), int(T_last)
        max_len = max(int(d.max_len), 0)
        loop = op == 1 and state is not None
        out = _alloc(("logits", op == 0, F32, (rows + 32, max(V, 0))), ("cand_val", op == 0, F32, (rows + 32, n)),
                     ("cand_idx", op == 0, I32, (rows + 32, n)), ("cand_sum", op == 0, F32, (rows + 32, n)),
                     ("x", op != 0, F32, ((rows + 32) * 576,)), ("tokens", op == 1, I32, (rows + 32,)), ("record", loop, I32, (rows, max_len)),
                     ("progress", loop, torch.int64, (1,)), ("logprob", loop and with_logprob, F32, (rows, max_len)))
        words = torch.empty((2 * (rows + 32) + 32 + 128,), dtype=I32) if loop or op == 2 else None
        o, nb = _outs(out)
        self._chk(self.lib.mellow_debug_dec_tail(self.h, C.byref(d), _p(W), _p(x), _p(x_img), _nb(x_img), _p(blk_live), _p(cand_val),
                                                 _p(cand_idx), _p(cand_sum), _p(seen_stop), _p(blk_left), _p(blk_snap), _p(row_of_slot),
                                                 _p(row_ids), o("logits"), nb("logits"), o("cand_val"), o("cand_idx"), o("cand_sum"),
                                                 nb("cand_val"), o("tokens"), nb("tokens"), o("record"), o("logprob"), nb("record"), _p(words),
                                                 _nb(words), o("progress"), o("x"), nb("x")))
        if "progress" in out:
            out["progress"] = int(out["progress"][0])
        if words is not None:
            at = rows + 32
            out["seen_stop"], out["scalars"] = words[:at], words[at:at + 32]
            out["n_seen"], out["arrive"], out["ticket"], out["n_compactions"] = (int(v) for v in words[at:at + 4])
            out["blk_left"], out["blk_live"], out["row_of_slot"] = words[at + 32:at + 96], words[at + 96:at + 160], words[at + 160:]
        return out

    def debug_prefill_attn(self, q, k, v, T: int, variant: int = 0, qpos0: int = 0, out_form: int = 0) -> torch.Tensor:
        """One launch of a causal GQA prefill attention kernel on host data (mellow_debug_prefill_attn): q [B][T - qpos0][576], k / v
        pages [B][3][Tmax][64].  variant 0 exact fp32, 1 f32x3, 2 bf16 once on fp32 pages, 3 bf16 once on bf16 pages.  -> the whole
        device output, which held 0xFF bytes before the launch: out_form 0 fp32 [B * (T - qpos0) + 32][576] (real rows first),
        out_form 1 the raw APB image of roundup(rows, 128) rows as int32 words."""
        self._need("mellow_debug_prefill_attn")
        q, k, v = _f32(q), _f32(k), _f32(v)
        B, T, qpos0 = int(k.shape[0]), int(T), int(qpos0)
        if k.dim() != 4 or k.shape[1] != 3 or k.shape[3] != 64 or v.shape != k.shape:
            raise ValueError(f"k {tuple(k.shape)} / v {tuple(v.shape)} are not pages [B][3][Tmax][64]")
        if q.dim() != 3 or q.shape[0] != B or q.shape[1] != T - qpos0 or q.shape[2] != 576:
            raise ValueError(f"q {tuple(q.shape)} is not [B = {B}][T - qpos0 = {T - qpos0}][576]")
        out = _attn_out(B * q.shape[1], 576, int(out_form))
        self._chk(self.lib.mellow_debug_prefill_attn(self.h, int(variant), _p(q), _p(k), _p(v), B, T, int(k.shape[2]), qpos0,
                                                     int(out_form), _p(out), _nb(out)))
        return out

    def debug_window_attn(self, qkv, bias, mask=None, in16: bool = False, out_form: int = 0) -> torch.Tensor:
        """One launch of the Swin window attention kernel on host data (mellow_debug_window_attn): qkv [M][3 C] rows in window order,
        bias [nH][64][64], mask [nW][64][64] or None; in16: qkv rounded to bf16 rows on the device, the bf16-input kernel.  -> the
        whole device output as debug_prefill_attn returns it (width C)."""
        self._need("mellow_debug_window_attn")
        qkv, bias, mask = _f32(qkv), _f32(bias), _f32(mask)
        if qkv.dim() != 2 or qkv.shape[1] % 3 or bias.dim() != 3 or tuple(bias.shape[1:]) != (64, 64):
            raise ValueError(f"qkv {tuple(qkv.shape)} / bias {tuple(bias.shape)} are not [M][3 C] / [nH][64][64]")
        if mask is not None and (mask.dim() != 3 or tuple(mask.shape[1:]) != (64, 64)):
            raise ValueError(f"mask {tuple(mask.shape)} is not [nW][64][64]")
        M, Cw, nH = int(qkv.shape[0]), int(qkv.shape[1]) // 3, int(bias.shape[0])
        out = _attn_out(M, Cw, int(out_form))
        self._chk(self.lib.mellow_debug_window_attn(self.h, _p(qkv), M, Cw, nH, _p(bias), _p(mask), 0 if mask is None else int(mask.shape[0]),
                                                    1 if in16 else 0, int(out_form), _p(out), _nb(out)))
        return out

    def debug_dec_head(self, x: torch.Tensor, act_fp8: bool = False) -> torch.Tensor:
        """The decode step's lm_head kernel on the rows x [B, hidden] (device tensor) -> logits [B, vocab]."""
        x = x.to(self.tdev).contiguous().float()
        out = torch.empty((x.shape[0], self.lm.vocab_size), dtype=torch.float32, device=self.tdev)
        self._chk(self.lib.mellow_debug_dec_head(self.h, _p(x), x.shape[0], 1 if act_fp8 else 0, _p(out)))
        return out

    def debug_dec_head_lse(self, x: torch.Tensor, act_fp8: bool = False) -> dict:
        """The same kernel in the variant a generate(return_logprobs=True) step runs, plus the merge of its per-tile partials
        (mellow_debug_dec_head_lse): x [B, hidden] -> {"logits" [B, vocab] f32, "lse" [B] f32, "max" [B] f32, "argmax" [B] i32}."""
        self._need("mellow_debug_dec_head_lse")
        x = x.to(self.tdev).contiguous().float()
        B = x.shape[0]
        out = {"logits": torch.empty((B, self.lm.vocab_size), dtype=torch.float32, device=self.tdev),
               "lse": torch.empty((B,), dtype=torch.float32, device=self.tdev),
               "max": torch.empty((B,), dtype=torch.float32, device=self.tdev),
               "argmax": torch.empty((B,), dtype=torch.int32, device=self.tdev)}
        self._sync_inputs()
        self._chk(self.lib.mellow_debug_dec_head_lse(self.h, _p(x), B, 1 if act_fp8 else 0, _p(out["logits"]), _p(out["lse"]),
                                                     _p(out["max"]), _p(out["argmax"])))
        return out
