"""GPU (-m gpu): the three GEMM families and their shared epilogue, ONE launch at a time on data this module chose, through the tap
mellow_debug_gemm_epi (include/mellow_hip.h) of an engine without weights: kernel 0 = launch_gemm (exact fp32 MFMA), 16 =
launch_gemm_bf16x3_fused (f32x3, A split in registers), 17 = launch_split_rows_apb + launch_gemm_bf16x3_apb (both operands by LDS-DMA).

Yardsticks (tests/gemm_ref.py; tests/test_gemm_ref_cpu.py checks them and shows what they would catch):
  A. the float64 definition, per element within tol = L delta + 8 * 2^-24 * max(|ref|, |largest intermediate|),
     delta = (K + 8) * 2^-24 * r * (|A| . |W|^T): derived from the reference alone, never from the kernel; ssq_out within 2^-18
     relative of the float64 sum of squares of the stored values;
  B. bit identities stated from the code: kernel 17 == kernel 16 (the same bf16 pieces, the same per-accumulator MFMA order, the
     same split-K partition); the APB image decoded == C; in-place residual == separate residual; rows [0, M1) of an M2-row launch
     == the M1-row launch; EPI_QKV_ROPE_AT == rows and page slots [pos0, T) of the whole launch; gemm_x3w_kernel == the tile kernel;
     a call == its repetitions;
  C. split-K against float64 and against the whole launch within 2 tol (two summation orders are no identity);
  D. guards: every output is filled with 0xFF bytes first, so what no row owns must still hold them, and what a row owns must not;
  E. refusals by name.
Every case prints max err / tol (DESIGN.md 6p is where the figures belong)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from mellow_amd import engine as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R  # noqa: E402
import gemm_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4, 32), (33, 68, 64), (127, 128, 96), (129, 132, 160), (129, 128, 192), (257, 576, 576), (70, 527, 64), (65, 64, 208),
          # k16 steps against the six-step unroll of the LDS-DMA loop: three (kernel 17 at its minimum K, every look-ahead issue
          # clamped), seven (one past a full trip, two row panels), fourteen (all three kernels; x3p off a multiple of six)
          (33, 68, 48), (129, 132, 112), (65, 64, 224)]
QKV_CASES = [(1, 1, 1, 0), (2, 33, 40, 0), (3, 129, 160, 0), (2, 97, 128, 64), (2, 389, 453, 256)]          # (B, T, Tmax, pos0)


def kernels_for(K):
    return [k for k in (0, 16, 17) if (K % 32 == 0 if k != 17 else (K % 16 == 0 and K >= 48))]


def stored_n(Nw, wide=False):
    if Nw == 527:
        return 544
    n4 = (Nw + 3) // 4 * 4
    return min(n4 + 8, (Nw + 127) // 128 * 128) if wide else n4


@pytest.fixture(scope="module")
def engine():
    e = E.Engine(device=0)          # no weights: the tap works on an engine that is not finalised
    yield e
    e.close()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _ndiff(a, b):
    return f"{int((_bits(a) != _bits(b)).sum())} of {a.numel()} words differ"


# ---- D: the guards, applied to every launch of this module ----------------------------------------------------------------------------------
def unpack_c(out, crow, n_c, N):
    """the tap's C [n_c + 32][ldc] -> [n_c][N] after the guard checks.  Rows no GEMM row maps to come back as NaN."""
    c = out["c"]
    assert c.shape[0] == n_c + 32 and c.shape[1] >= N
    b = _bits(c)
    assert bool((b[n_c:] == -1).all()), "C rows behind the last mapped row were written"
    assert bool((b[:, N:] == -1).all()), "C columns [N, ldc) were written"
    own = torch.zeros(n_c, dtype=torch.bool)
    own[crow] = True
    assert bool((b[:n_c][~own] == -1).all()), "a C row no GEMM row maps to was written"
    assert bool(torch.isfinite(c[:n_c, :N][own]).all()), "an owned word of C was not written (or is not finite)"
    return c[:n_c, :N]


def unpack_c3(out, M, N):
    x, unowned, halves = R.apb_decode(out["c3"].numpy(), M, N)
    assert np.all(halves[unowned] == 0xFFFF), "an APB slot no row < M owns was written"
    assert np.all(halves[~unowned] != 0xFFFF), "an APB slot of a real row was not written"
    # the decode sums the three pieces, and -0.0 + 0.0 + 0.0 is +0.0: a stored -0.0 (GELU of x < -5.6 is 0.5 x * 0) keeps its sign in the
    # leading piece only, so that is where the sign of a zero is read
    Mp = (M + 127) // 128 * 128
    hi = halves[R._apb_slots(Mp, N)[:M, :, 0]].reshape(M, N)
    neg_zero = torch.from_numpy((hi == 0x8000) & (x.numpy() == 0))
    return torch.where(neg_zero, torch.tensor(-0.0), x)


def unpack_ssq(out, M):
    s = out["ssq"]
    assert bool((_bits(s[M:]) == -1).all()), "ssq rows >= M were written"
    assert bool(torch.isfinite(s[:M]).all()), "an ssq word of a real row was not written"
    return s[:M]


def unpack_qkv(out, B, T, Tmax, pos0):
    M = B * (T - pos0)
    q, k, v = out["q"], out["k"], out["v"]
    assert q.shape == (M + 32, 576) and k.shape == (B + 1, 3, Tmax, 64) and v.shape == k.shape
    assert bool((_bits(q[M:]) == -1).all()), "q_out rows >= M were written"
    assert bool(torch.isfinite(q[:M]).all()), "a q_out word of a real row was not written"
    for name, p in (("K", k), ("V", v)):
        b = _bits(p)
        assert bool((b[B] == -1).all()), f"a {name} page of no example was written"
        assert bool((b[:B, :, :pos0] == -1).all()) and bool((b[:B, :, T:] == -1).all()), f"{name} page positions outside [pos0, T) were written"
        assert bool(torch.isfinite(p[:B, :, pos0:T]).all()), f"a {name} page slot in [pos0, T) was not written"
    return q[:M], k[:B], v[:B]


def _ratio(what, got, ref, tol):
    r = G.miss(torch.nan_to_num(got, nan=0.0), ref, tol)
    print(f"GEMM {what}: max err / tol {r:.3f}")
    return r


# ---- linear cases -------------------------------------------------------------------------------------------------------------------------
VARIANTS = {
    "plain": dict(),
    "bias": dict(bias=True),
    "bias_gelu": dict(bias=True, act="gelu"),
    "bias_sigmoid_wide": dict(bias=True, act="sigmoid", wide=True, pad=4),
    "resid": dict(bias=True, act="gelu", resid=1),
    "resid_in_place": dict(bias=True, act="gelu", resid=2, pad=8),
    "row_scale": dict(bias=True, rs=True),
}


@functools.lru_cache(maxsize=None)
def linear_case(M, Nw, K, variant, cmap_name=None):
    v = VARIANTS[variant]
    A, W, bias = G.operands(M, Nw, K)
    N = stored_n(Nw, v.get("wide", False))
    cmap, rows_out = {None: (None, 0), "emb": G.emb_map(), "window": G.window_map()}[cmap_name]
    crow, n_c = G.crows(M, cmap, rows_out)
    resid = None
    if v.get("resid"):
        resid = G.residual(n_c, N).clone()
        own = torch.zeros(n_c, dtype=torch.bool)
        own[crow] = True
        _bits(resid)[~own] = -1          # rows no GEMM row maps to: 0xFF bytes, so that an in-place launch leaves them as the fill
    rs = G.row_ssq(M) if v.get("rs") else None
    ref, tol, crow = G.linear_ref(A, W, N, bias=bias if v.get("bias") else None, act=v.get("act", "none"), resid=resid, crow_map=cmap,
                                  rows_out=rows_out, rs=rs)
    return dict(A=A, W=W, bias=bias if v.get("bias") else None, act=v.get("act", "none"), N=N, resid=resid, in_place=v.get("resid") == 2,
                cmap=cmap, rows_out=rows_out, crow=crow, n_c=n_c, rs=rs, ldc=N + v.get("pad", 0), ref=ref, tol=tol, M=M, K=K)


def run_linear(engine, c, kernel, **kw):
    rs = c["rs"]
    args = dict(kernel=kernel, epi="linear", N=c["N"], act=c["act"], bias=c["bias"], resid=c["resid"], in_place=c["in_place"],
                crow_map=c["cmap"], rows_out=c["rows_out"], ldc=c["ldc"])
    if rs is not None:
        args.update(rs_ssq=rs[0], rs_dim=rs[1], rs_eps=rs[2])
    args.update(kw)
    return engine.debug_gemm_epi(c["A"], c["W"], **args)


# ---- A: linear against float64 (+ B: 17 == 16, a call == its repetition) -------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("M,Nw,K", SHAPES)
def test_linear_epilogue_against_float64(engine, M, Nw, K, variant):
    c = linear_case(M, Nw, K, variant)
    got = {}
    for kernel in kernels_for(K):
        got[kernel] = unpack_c(run_linear(engine, c, kernel), c["crow"], c["n_c"], c["N"])
        r = _ratio(f"linear {variant} kernel {kernel} (M, Nw, K) = ({M}, {Nw}, {K}) N = {c['N']}", got[kernel], c["ref"], c["tol"])
        assert _same_bits(unpack_c(run_linear(engine, c, kernel), c["crow"], c["n_c"], c["N"]), got[kernel]), "a repetition differs"
        assert r <= 1.0
    if 16 in got and 17 in got:
        assert _same_bits(got[17], got[16]), "kernel 17 != kernel 16: " + _ndiff(got[17], got[16])


@pytest.mark.parametrize("M,Nw,K", SHAPES)
def test_in_place_residual_equals_separate_residual(engine, M, Nw, K):
    """the epilogue fetches the residual up front, before any store of the launch can alias it: one buffer or two, the same bits"""
    sep, inp = linear_case(M, Nw, K, "resid"), linear_case(M, Nw, K, "resid_in_place")
    for kernel in kernels_for(K):
        a = unpack_c(run_linear(engine, sep, kernel), sep["crow"], sep["n_c"], sep["N"])
        b = unpack_c(run_linear(engine, inp, kernel), inp["crow"], inp["n_c"], inp["N"])
        assert _same_bits(a, b), f"kernel {kernel}: " + _ndiff(a, b)


@pytest.mark.parametrize("cmap_name,M", [("emb", 160), ("window", 512)])
def test_row_maps_with_in_place_residual(engine, cmap_name, M):
    """crow_map: 32 -> 33 rows (the gap row of every 33 stays 0xFF) and the 256-row shifted-window permutation"""
    c = linear_case(M, 68, 64, "resid_in_place", cmap_name)
    got = {}
    for kernel in (0, 16, 17):
        got[kernel] = unpack_c(run_linear(engine, c, kernel), c["crow"], c["n_c"], c["N"])
        assert _ratio(f"linear {cmap_name} map, in-place residual, kernel {kernel} M = {M}", got[kernel], c["ref"], c["tol"]) <= 1.0
    assert _same_bits(got[17], got[16]), _ndiff(got[17], got[16])


def _check_ssq(what, ssq, stored):
    want = G.ssq_ref(stored)
    rel = float(((ssq.double() - want).abs() / want).max())
    print(f"GEMM {what}: ssq max relative error {rel:.3e} = {rel / G.SSQ_RTOL:.3f} x 2^-18")
    assert rel <= G.SSQ_RTOL


@pytest.mark.parametrize("M,Nw,K,variant", [(65, 64, 208, "bias"), (129, 64, 64, "resid_in_place"), (257, 576, 576, "resid_in_place"),
                                            (257, 576, 576, "row_scale")])
def test_c_c3_and_ssq_hand_over(engine, M, Nw, K, variant):
    """as o_proj and down: C, its APB copy and the RMS partials of the next norm from one launch.  The image decodes to C bit for bit
    (split8 is exact), and ssq is the sum of squares of what was stored"""
    c = linear_case(M, Nw, K, variant)
    got = {}
    for kernel in [k for k in kernels_for(K) if k != 0]:
        out = run_linear(engine, c, kernel, want_c3=True, want_ssq=True)
        cc = unpack_c(out, c["crow"], c["n_c"], c["N"])
        c3 = unpack_c3(out, M, c["N"])
        what = f"C + C3 + ssq {variant} kernel {kernel} (M, N, K) = ({M}, {Nw}, {K})"
        assert _ratio(what, cc, c["ref"], c["tol"]) <= 1.0
        assert _same_bits(c3, cc), "the APB image does not decode to C: " + _ndiff(c3, cc)
        _check_ssq(what, unpack_ssq(out, M), cc)
        plain = unpack_c(run_linear(engine, c, kernel), c["crow"], c["n_c"], c["N"])
        assert _same_bits(plain, cc), "C differs when the hand-over is also written"
        got[kernel] = cc
    if len(got) == 2:
        assert _same_bits(got[17], got[16])


def test_c3_alone_bias_gelu(engine):
    """as the encoder's fc1: only the APB copy is wanted (C null)"""
    M, Nw, K = 129, 384, 96
    c = linear_case(M, Nw, K, "bias_gelu")
    got = {}
    for kernel in (16, 17):
        out = run_linear(engine, c, kernel, want_c=False, want_c3=True)
        assert set(out) == {"c3"}
        got[kernel] = unpack_c3(out, M, 384)
        assert _ratio(f"C3 alone bias + GELU kernel {kernel} (129, 384, 96)", got[kernel], c["ref"], c["tol"]) <= 1.0
        full = unpack_c(run_linear(engine, c, kernel), c["crow"], c["n_c"], 384)
        assert _same_bits(got[kernel], full)
    assert _same_bits(got[17], got[16])


@pytest.mark.parametrize("kernel", [0, 16, 17])
def test_rows_of_a_longer_launch_equal_the_shorter_launch(engine, kernel):
    """a row's accumulators depend on its own A row only: rows [0, 97) of a 161-row launch (two 128-row panels) == the 97-row launch"""
    A, W, bias = G.operands(161, 132, 160)
    long_ = engine.debug_gemm_epi(A, W, kernel=kernel, bias=bias, act="gelu")["c"]
    short = engine.debug_gemm_epi(A[:97], W, kernel=kernel, bias=bias, act="gelu")["c"]
    assert _same_bits(long_[:97], short[:97]), _ndiff(long_[:97], short[:97])
    assert bool((_bits(short[97:]) == -1).all()) and bool((_bits(long_[161:]) == -1).all())


def test_narrow_output_tile_of_the_fp32_kernel(engine):
    """launch_gemm takes a 256 x 64 tile (one wave column) when Nw <= 64 and M >= 256: another lane-to-column layout of the epilogue"""
    c = linear_case(257, 64, 64, "bias_gelu")
    got = unpack_c(run_linear(engine, c, 0), c["crow"], 257, 64)
    assert _ratio("linear bias + GELU kernel 0, 256 x 64 tile (257, 64, 64)", got, c["ref"], c["tol"]) <= 1.0


# ---- SwiGLU -------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def swiglu_case(M, Nw, K, rs):
    A, W, _ = G.operands(M, Nw, K)
    rs = G.row_ssq(M) if rs else None
    ref, tol = G.swiglu_ref(A, W[:Nw // 2], W[Nw // 2:], rs=rs)
    return dict(A=A, W=W, rs=rs, ref=ref, tol=tol)


@pytest.mark.parametrize("rs", [False, True])
@pytest.mark.parametrize("M,Nw,K", [(33, 128, 64), (129, 128, 192), (130, 3072, 64), (129, 3072, 576)])
def test_swiglu_against_float64(engine, M, Nw, K, rs):
    """fp32 form on all three kernels, APB hand-over form on the f32x3 kernels (Nw = 3072: 24 column tiles, the XCD-ownership tile
    order of gemm_x3q_kernel); the image decodes to the fp32 form bit for bit"""
    c = swiglu_case(M, Nw, K, rs)
    N = Nw // 2
    kw = {} if c["rs"] is None else dict(rs_ssq=c["rs"][0], rs_dim=c["rs"][1], rs_eps=c["rs"][2])
    crow = torch.arange(M)
    got = {}
    for kernel in (0, 16, 17):
        out = engine.debug_gemm_epi(c["A"], c["W"], kernel=kernel, epi="swiglu", **kw)
        got[kernel] = unpack_c(out, crow, M, N)
        assert _ratio(f"swiglu fp32 form kernel {kernel} rs {int(rs)} (M, Nw, K) = ({M}, {Nw}, {K})", got[kernel], c["ref"], c["tol"]) <= 1.0
        if kernel:
            o3 = engine.debug_gemm_epi(c["A"], c["W"], kernel=kernel, epi="swiglu", want_c=False, want_c3=True, **kw)
            c3 = unpack_c3(o3, M, N)
            assert _ratio(f"swiglu APB form kernel {kernel} rs {int(rs)} (M, Nw, K) = ({M}, {Nw}, {K})", c3, c["ref"], c["tol"]) <= 1.0
            assert _same_bits(c3, got[kernel]), "the APB form does not decode to the fp32 form: " + _ndiff(c3, got[kernel])
    assert _same_bits(got[17], got[16]), _ndiff(got[17], got[16])


# ---- QKV + RoPE ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def qkv_case(B, T, Tmax, pos0, K, rs):
    """the rows of positions [pos0, T) of the whole-sequence inputs (so that the launch with a past can be held against the whole one)"""
    A, W, _ = G.operands(B * T, 960, K)
    ssq = G.row_ssq(B * T) if rs else None
    A = A.view(B, T, K)[:, pos0:].reshape(-1, K).contiguous()
    if ssq is not None:
        ssq = (ssq[0].view(B, T, 9)[:, pos0:].reshape(-1, 9).contiguous(), ssq[1], ssq[2])
    cos, sin = G.rope_tables(Tmax)
    ref = G.qkv_rope_ref(A, W, B, T, Tmax, pos0, cos, sin, rs=ssq)
    return dict(A=A, W=W, rs=ssq, cos=cos, sin=sin, ref=ref)


def run_qkv(engine, c, kernel, B, T, Tmax, pos0, rope=True):
    kw = {} if c["rs"] is None else dict(rs_ssq=c["rs"][0], rs_dim=c["rs"][1], rs_eps=c["rs"][2])
    out = engine.debug_gemm_epi(c["A"], c["W"], kernel=kernel, epi="qkv_rope", N=960, T=T, Tmax=Tmax, pos0=pos0,
                                rope=(c["cos"], c["sin"]) if rope else None, **kw)
    return unpack_qkv(out, B, T, Tmax, pos0)


@pytest.mark.parametrize("rs", [False, True])
@pytest.mark.parametrize("K", [64, 576])
@pytest.mark.parametrize("B,T,Tmax,pos0", QKV_CASES)
def test_qkv_rope_against_float64(engine, B, T, Tmax, pos0, K, rs):
    c = qkv_case(B, T, Tmax, pos0, K, rs)
    got = {}
    for kernel in (0, 16, 17):
        q, k, v = got[kernel] = run_qkv(engine, c, kernel, B, T, Tmax, pos0)
        what = f"qkv-rope kernel {kernel} rs {int(rs)} K {K} (B, T, Tmax, pos0) = ({B}, {T}, {Tmax}, {pos0})"
        rq = _ratio(what + " q", q, c["ref"]["q"], c["ref"]["q_tol"])
        rk = _ratio(what + " k", k, c["ref"]["k"], c["ref"]["k_tol"])
        rv = _ratio(what + " v", v, c["ref"]["v"], c["ref"]["v_tol"])
        assert max(rq, rk, rv) <= 1.0
    for a, b in zip(got[17], got[16]):
        assert _same_bits(a, b), _ndiff(a, b)


@pytest.mark.parametrize("kernel", [0, 16, 17])
@pytest.mark.parametrize("B,T,Tmax,pos0", [c for c in QKV_CASES if c[3] > 0])
def test_qkv_rope_at_equals_the_rows_of_the_whole_launch(engine, B, T, Tmax, pos0, kernel):
    """EPI_QKV_ROPE_AT differs from EPI_QKV_ROPE in qkv_pos alone: the same A rows give the same q rows and the same page slots"""
    K = 64
    part, whole = qkv_case(B, T, Tmax, pos0, K, True), qkv_case(B, T, Tmax, 0, K, True)
    qp, kp, vp = run_qkv(engine, part, kernel, B, T, Tmax, pos0)
    qw, kw_, vw = run_qkv(engine, whole, kernel, B, T, Tmax, 0)
    qw = qw.view(B, T, 576)[:, pos0:].reshape(-1, 576)
    assert _same_bits(qp, qw), _ndiff(qp, qw)
    assert _same_bits(kp[:, :, pos0:T], kw_[:, :, pos0:T]) and _same_bits(vp[:, :, pos0:T], vw[:, :, pos0:T])


def test_qkv_rope_with_the_engines_own_tables(engine):
    """rope_cos / rope_sin NULL: the tables of mellow_host_rope_tables, positions counted from 0"""
    import ctypes as C
    B, T, Tmax, pos0, K = 2, 33, 40, 0, 64
    c = dict(qkv_case(B, T, Tmax, pos0, K, False))
    cos, sin = np.empty((Tmax, 32), dtype=np.float32), np.empty((Tmax, 32), dtype=np.float32)
    fp = C.POINTER(C.c_float)
    assert engine.lib.mellow_host_rope_tables(float(engine.lm.rope_theta), 64, Tmax, cos.ctypes.data_as(fp), sin.ctypes.data_as(fp)) == 0
    ref = G.qkv_rope_ref(c["A"], c["W"], B, T, Tmax, pos0, torch.from_numpy(cos), torch.from_numpy(sin))
    q, k, v = run_qkv(engine, c, 17, B, T, Tmax, pos0, rope=False)
    assert max(_ratio("qkv-rope own tables q", q, ref["q"], ref["q_tol"]), _ratio("qkv-rope own tables k", k, ref["k"], ref["k_tol"])) <= 1.0


# ---- the weight-stationary K = 96 kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "bias", "bias_gelu"])
@pytest.mark.parametrize("M,Nw", [(8192, 288), (8229, 384)])
def test_x3w_kernel_is_bit_identical_to_the_tile_kernel(engine, M, Nw, variant):
    """gemm_x3w_kernel (K = 96, M >= 8192) issues the same six piece products per k16 step in the same order as gemm_x3q_kernel, so
    no_x3w changes no bit (kernels.h and the engine option "x3w" say so)"""
    c = linear_case(M, Nw, 96, variant)
    w = unpack_c(run_linear(engine, c, 17), c["crow"], M, Nw)
    t = unpack_c(run_linear(engine, c, 17, no_x3w=True), c["crow"], M, Nw)
    assert _ratio(f"x3w {variant} (M, Nw) = ({M}, {Nw})", w, c["ref"], c["tol"]) <= 1.0
    assert _same_bits(w, t), "x3w != tile kernel: " + _ndiff(w, t)


# ---- C: split-K -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,Nw,K,variant", [(33, 128, 1024, "plain"), (130, 544, 4608, "bias_sigmoid_wide"), (64, 768, 3072, "resid_in_place")])
def test_split_k_against_float64_and_the_whole_launch(engine, M, Nw, K, variant):
    c = linear_case(M, Nw, K, variant)
    got = {}
    for kernel in (16, 17):
        sp = unpack_c(run_linear(engine, c, kernel, splitk_max=8), c["crow"], M, c["N"])
        whole = unpack_c(run_linear(engine, c, kernel), c["crow"], M, c["N"])
        what = f"split-K {variant} kernel {kernel} (M, Nw, K) = ({M}, {Nw}, {K})"
        assert _ratio(what, sp, c["ref"], c["tol"]) <= 1.0
        assert _ratio(what + " vs whole / (2 tol)", sp, whole.double(), 2 * c["tol"]) <= 1.0
        assert not _same_bits(sp, whole), "the launch was not split: this case checks nothing"
        for _ in range(2):
            assert _same_bits(unpack_c(run_linear(engine, c, kernel, splitk_max=8), c["crow"], M, c["N"]), sp), "a repetition differs"
        got[kernel] = sp
    assert _same_bits(got[17], got[16]), _ndiff(got[17], got[16])


def test_split_k_leaves_a_half_full_short_launch_whole(engine):
    """splitk_for: more than 128 tiles and fewer than 128 k16 steps stay whole.  (300, 5504, 1024) is 3 x 43 = 129 tiles of 64 steps
    (the 99 tiles of (300, 4224, 1024) are split in two: 99 <= 128); with the workspace or without it, the same bits"""
    A, W, _ = G.operands(300, 5504, 1024)
    rows = torch.arange(300)
    for kernel in (16, 17):
        a = unpack_c(engine.debug_gemm_epi(A, W, kernel=kernel, splitk_max=8), rows, 300, 5504)
        b = unpack_c(engine.debug_gemm_epi(A, W, kernel=kernel), rows, 300, 5504)
        assert _same_bits(a, b), _ndiff(a, b)
    a = unpack_c(engine.debug_gemm_epi(A, W[:4224], kernel=17, splitk_max=8), rows, 300, 4224)
    b = unpack_c(engine.debug_gemm_epi(A, W[:4224], kernel=17), rows, 300, 4224)
    assert not _same_bits(a, b), "99 tiles x 64 steps were expected to split in two"


# ---- E: refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument(engine):
    A32, W32, b32 = G.operands(33, 68, 64)
    A48 = torch.zeros(8, 48)
    A16 = torch.zeros(8, 32)
    Aq, Wq = torch.zeros(66, 64), torch.zeros(960, 64)
    bad = [
        (dict(A=A48, W=torch.zeros(8, 48), kernel=0), "K = 48"),
        (dict(A=A48, W=torch.zeros(8, 48), kernel=16), "K = 48"),
        (dict(A=torch.zeros(8, 56), W=torch.zeros(8, 56), kernel=17), "K = 56"),
        (dict(A=A16, W=torch.zeros(8, 32), kernel=17), "K = 32"),
        (dict(kernel=3), "kernel"),
        (dict(N=66), "N = 66"),
        (dict(N=64), "N = 64"),
        (dict(N=132), "N = 132"),
        (dict(kernel=16, want_c3=True), "want_c3"),
        (dict(A=A32, W=torch.zeros(136, 64), kernel=16, epi="swiglu", want_c=False, want_c3=True), "want_c3"),
        (dict(kernel=0, want_c3=True), "want_c3"),
        (dict(kernel=0, splitk_max=8), "splitk_max"),
        (dict(A=A32, W=torch.zeros(64, 64), kernel=16, want_ssq=True), "want_ssq"),
        (dict(ldc=64), "ldc"),
        (dict(A=Aq, W=Wq, epi="qkv_rope", T=33, Tmax=40, pos0=33), "pos0"),
        (dict(A=Aq, W=Wq, epi="qkv_rope", T=33, Tmax=40, pos0=-1), "pos0"),
        (dict(A=Aq, W=Wq, epi="qkv_rope", T=33, Tmax=32), "Tmax"),
        (dict(A=Aq[:65], W=Wq, epi="qkv_rope", T=33, Tmax=40), "M = 65"),
        (dict(A=Aq, W=Wq[:896], epi="qkv_rope", T=33, Tmax=40), "Nw"),
    ]
    for kw, word in bad:
        args = dict(A=A32, W=W32, kernel=17)
        args.update(kw)
        A, W = args.pop("A"), args.pop("W")
        with pytest.raises(E.EngineError, match=word):
            engine.debug_gemm_epi(A, W, **args)
    # a capacity that is too small: the raw entry, C one float short
    import ctypes as C
    d = E.GemmEpi()
    d.size, d.kernel, d.M, d.K, d.Nw, d.N, d.ldc, d.want_c = C.sizeof(E.GemmEpi), 16, 33, 64, 68, 68, 68, 1
    out = torch.empty((33 + 32) * 68, dtype=torch.float32)
    vp = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    rc = engine.lib.mellow_debug_gemm_epi(engine.h, C.byref(d), vp(A32), vp(W32), None, None, None, None, None, None, vp(out), out.numel() * 4 - 4,
                                          None, 0, None, 0, None, 0, None, None, 0)
    assert rc != 0 and "c_capacity" in engine.lib.mellow_last_error().decode()
    # and the engine still works afterwards
    c = linear_case(33, 68, 64, "plain")
    assert _ratio("after the refusals", unpack_c(run_linear(engine, c, 17), c["crow"], 33, 68), c["ref"], c["tol"]) <= 1.0
