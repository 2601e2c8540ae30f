"""CPU: the float64 references of tests/gemm_ref.py are what they claim to be -- against torch float32 modules (an fp32 evaluation
must itself sit inside the derived tolerance), against a longhand loop on a tiny case -- and the tolerance is tight enough to mean
something: every mutant of an epilogue misses the reference by >= 100 x tol on the inputs the GPU tests use."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as G  # noqa: E402

M0, NW0, K0 = 160, 68, 64            # the emb-map case of the GPU module: 5 groups of 32 rows across a 128-row panel edge


def _lin_inputs(N=68):
    A, W, bias = G.operands(M0, NW0, K0)
    cmap, rows_out = G.emb_map()
    resid = G.residual(M0 // 32 * rows_out, N)
    return A, W, bias, resid, cmap, rows_out


# ---- the references against torch float32 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["none", "gelu", "sigmoid"])
def test_linear_ref_against_torch_float32(act):
    A, W, bias, _, _, _ = _lin_inputs()
    N = 72                           # stored columns beyond Nw = 68: act(0 + 0) + resid
    resid = G.residual(M0, N)
    ref, tol, crow = G.linear_ref(A, W, N, bias=bias, act=act, resid=resid)
    assert torch.equal(crow, torch.arange(M0)) and not torch.isnan(ref).any()
    y = F.linear(A, W, bias)
    y = {"none": lambda v: v, "gelu": F.gelu, "sigmoid": torch.sigmoid}[act](y)
    pad = {"none": 0.0, "gelu": 0.0, "sigmoid": 0.5}[act]
    got = torch.cat([y, torch.full((M0, N - NW0), pad)], dim=1) + resid
    r = G.miss(got, ref, tol)
    print(f"linear {act}: torch float32 / tol {r:.3f}")
    assert r <= 1.0


def test_swiglu_and_row_scale_against_torch_float32():
    """(x W'^T) r is RMSNorm(x) W'^T: the row scale from the per-64-column partial sums of squares of x"""
    A, W, _ = G.operands(130, 128, 576, seed=3)
    Wg, Wu = W[:64], W[64:]
    ssq = (A.double() ** 2).view(130, 9, 64).sum(dim=2).float()
    ref, tol = G.swiglu_ref(A, Wg, Wu, rs=(ssq, 576.0, 1e-5))
    xn = A * torch.rsqrt(A.pow(2).mean(dim=1, keepdim=True) + 1e-5)
    got = F.silu(F.linear(xn, Wg)) * F.linear(xn, Wu)
    r = G.miss(got, ref, tol)
    print(f"swiglu + row scale: torch float32 / tol {r:.3f}")
    assert r <= 1.0
    ref0, tol0 = G.swiglu_ref(A, Wg, Wu)
    assert G.miss(F.silu(F.linear(A, Wg)) * F.linear(A, Wu), ref0, tol0) <= 1.0


def _hf_rope(x, cos, sin):
    """transformers' apply_rotary_pos_emb on [M][heads][64] with cos / sin [M][32]"""
    c, s = torch.cat([cos, cos], dim=-1)[:, None, :], torch.cat([sin, sin], dim=-1)[:, None, :]
    rot = torch.cat([-x[..., 32:], x[..., :32]], dim=-1)
    return x * c + rot * s


@pytest.mark.parametrize("B,T,Tmax,pos0", [(2, 33, 40, 0), (2, 97, 128, 64)])
def test_qkv_rope_ref_against_torch_float32(B, T, Tmax, pos0):
    M = B * (T - pos0)
    A, W, _ = G.operands(M, 960, 64)
    cos, sin = G.rope_tables(Tmax)
    ref = G.qkv_rope_ref(A, W, B, T, Tmax, pos0, cos, sin)
    y = F.linear(A, W).view(M, 15, 64)
    pos = pos0 + torch.arange(M) % (T - pos0)
    q = _hf_rope(y[:, :9], cos[pos], sin[pos]).reshape(M, 576)
    k = _hf_rope(y[:, 9:12], cos[pos], sin[pos])
    v = y[:, 12:]
    assert G.miss(q, ref["q"], ref["q_tol"]) <= 1.0
    kp = torch.full((B, 3, Tmax, 64), float("nan"))
    vp = torch.full((B, 3, Tmax, 64), float("nan"))
    for m in range(M):
        kp[m // (T - pos0), :, pos[m]] = k[m]
        vp[m // (T - pos0), :, pos[m]] = v[m]
    for got, name in ((kp, "k"), (vp, "v")):
        own = ~torch.isnan(ref[name + "_tol"])
        assert torch.equal(own, ~torch.isnan(got)), "the reference owns other page slots than positions [pos0, T) of every example"
        assert int(own.sum()) == M * 192
        assert G.miss(torch.nan_to_num(got), ref[name], ref[name + "_tol"]) <= 1.0


# ---- longhand -----------------------------------------------------------------------------------------------------------------------------
def test_references_against_a_longhand_loop():
    g = torch.Generator().manual_seed(1)
    M, N, K = 4, 4, 8
    A, W, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    res = torch.randn(6, N, generator=g)
    ssq = torch.rand(M, 3, generator=g) + 0.5
    cmap = torch.tensor([2, 0], dtype=torch.int32)            # rows_in 2 -> rows_out 3
    ref, tol, crow = G.linear_ref(A, W, N, bias=b, act="gelu", resid=res, crow_map=cmap, rows_out=3, rs=(ssq, 5.0, 0.25))
    assert crow.tolist() == [2, 0, 5, 3] and torch.isnan(ref[1]).all() and torch.isnan(ref[4]).all()
    for m in range(M):
        r = 1.0 / math.sqrt(sum(float(ssq[m, p]) for p in range(3)) / 5.0 + 0.25)
        for n in range(N):
            acc = sum(float(A[m, k]) * float(W[n, k]) for k in range(K))
            sab = sum(abs(float(A[m, k]) * float(W[n, k])) for k in range(K))
            pre = acc * r + float(b[n])
            y = 0.5 * pre * (1.0 + math.erf(pre / math.sqrt(2.0)))
            c = [2, 0, 5, 3][m]
            assert abs(float(ref[c, n]) - (y + float(res[c, n]))) < 1e-12
            want = 1.13 * (K + 8) * 2.0 ** -24 * r * sab + 8 * 2.0 ** -24 * max(abs(y + float(res[c, n])), abs(acc * r), abs(pre), abs(y), abs(float(res[c, n])))
            assert abs(float(tol[c, n]) - want) < 1e-15
    out, _ = G.swiglu_ref(A, W[:2], W[2:])
    for m in range(M):
        for n in range(2):
            gt = sum(float(A[m, k]) * float(W[n, k]) for k in range(K))
            up = sum(float(A[m, k]) * float(W[2 + n, k]) for k in range(K))
            assert abs(float(out[m, n]) - gt / (1.0 + math.exp(-gt)) * up) < 1e-12
    st = torch.randn(3, 128, generator=g)
    s = G.ssq_ref(st)
    assert s.shape == (3, 2)
    assert abs(float(s[1, 1]) - sum(float(st[1, 64 + j]) ** 2 for j in range(64))) < 1e-10


def test_rope_longhand_at_one_element():
    B, T, Tmax, pos0 = 2, 5, 9, 2
    M = B * (T - pos0)
    A, W, _ = G.operands(M, 960, 32, seed=2)
    cos, sin = G.rope_tables(Tmax)
    ref = G.qkv_rope_ref(A, W, B, T, Tmax, pos0, cos, sin)
    acc = A.double() @ W.double().T
    m, t, b = 4, 3, 1                  # row 4 = example 1, i = 1 -> position 2 + 1
    for i in (0, 7, 31):
        c, s = float(cos[t, i]), float(sin[t, i])
        x1, x2 = float(acc[m, 64 * 2 + i]), float(acc[m, 64 * 2 + 32 + i])               # q head 2
        assert abs(float(ref["q"][m, 128 + i]) - (x1 * c - x2 * s)) < 1e-12
        assert abs(float(ref["q"][m, 128 + 32 + i]) - (x2 * c + x1 * s)) < 1e-12
        k1, k2 = float(acc[m, 576 + 64 + i]), float(acc[m, 576 + 64 + 32 + i])             # k head 1
        assert abs(float(ref["k"][b, 1, t, i]) - (k1 * c - k2 * s)) < 1e-12
        assert abs(float(ref["v"][b, 2, t, 32 + i]) - float(acc[m, 768 + 128 + 32 + i])) < 1e-12
    assert torch.isnan(ref["k"][:, :, :pos0]).all() and torch.isnan(ref["k"][:, :, T:]).all()


def test_row_maps_are_real_permutations():
    cm, rows_out = G.emb_map()
    assert rows_out == 33 and sorted(cm.tolist()) == list(range(1, 33)) and cm.tolist() != list(range(1, 33))
    inv = torch.empty(32, dtype=torch.long)
    inv[cm.long() - 1] = torch.arange(32)
    assert not torch.equal(inv + 1, cm.long()), "an involution: the inverted-map mutant would be the map itself"
    wm, n = G.window_map()
    assert n == 256 and sorted(wm.tolist()) == list(range(256)) and wm.tolist() != list(range(256))
    from mellow_amd import engine as E
    assert np.array_equal(wm.numpy(), E.host_window_map(16, 4))
    cos, sin = G.rope_tables(453)
    assert len({tuple(r) for r in cos.numpy().round(6).tolist()}) == 453 and float(sin[0].abs().min()) > 0


# ---- sensitivity: what a pass on the GPU means ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant,act", [("bias_after_act", "gelu"), ("bias_after_act", "sigmoid"), ("resid_before_act", "gelu"),
                                        ("resid_before_act", "sigmoid"), ("crow_inverted", "none"), ("rs_after_bias", "none"),
                                        ("rs_after_bias", "gelu")])
def test_linear_mutants_miss_by_100_tol(mutant, act):
    A, W, bias, resid, cmap, rows_out = _lin_inputs()
    rs = G.row_ssq(M0)
    kw = dict(bias=bias, act=act, resid=resid, crow_map=cmap, rows_out=rows_out, rs=rs)
    ref, tol, _ = G.linear_ref(A, W, 68, **kw)
    bad, _, _ = G.linear_ref(A, W, 68, mutant=mutant, **kw)
    own = ~torch.isnan(tol)
    if mutant == "crow_inverted":
        assert torch.equal(own, ~torch.isnan(bad))
    r = G.miss(torch.nan_to_num(bad), ref, tol)
    print(f"mutant {mutant} ({act}): miss / tol {r:.0f}")
    assert r >= 100.0


def test_window_map_mutant_misses_by_100_tol():
    A, W, bias = G.operands(512, 68, 64)
    wm, n = G.window_map()
    resid = G.residual(512, 68)
    ref, tol, _ = G.linear_ref(A, W, 68, bias=bias, resid=resid, crow_map=wm, rows_out=n)
    bad, _, _ = G.linear_ref(A, W, 68, bias=bias, resid=resid, crow_map=wm, rows_out=n, mutant="crow_inverted")
    assert G.miss(bad, ref, tol) >= 100.0


def test_swiglu_mutant_misses_by_100_tol():
    for (M, Nw, K) in [(33, 128, 64), (130, 3072, 64)]:
        A, W, _ = G.operands(M, Nw, K)
        ref, tol = G.swiglu_ref(A, W[:Nw // 2], W[Nw // 2:])
        bad, _ = G.swiglu_ref(A, W[:Nw // 2], W[Nw // 2:], mutant="swap_gate_up")
        assert G.miss(bad, ref, tol) >= 100.0


@pytest.mark.parametrize("mutant", ["rot_sign", "no_pos0", "v_rotated", "kv_head_off"])
def test_rope_mutants_miss_by_100_tol(mutant):
    B, T, Tmax, pos0 = 2, 97, 128, 64
    M = B * (T - pos0)
    A, W, _ = G.operands(M, 960, 64)
    cos, sin = G.rope_tables(Tmax)
    ref = G.qkv_rope_ref(A, W, B, T, Tmax, pos0, cos, sin)
    bad = G.qkv_rope_ref(A, W, B, T, Tmax, pos0, cos, sin, mutant=mutant)
    worst = max(G.miss(torch.nan_to_num(bad[n]), ref[n], ref[n + "_tol"]) for n in ("q", "k", "v"))
    hit = {"rot_sign": ("q", "k"), "no_pos0": ("q", "k"), "v_rotated": ("v",), "kv_head_off": ("k", "v")}[mutant]
    for n in hit:
        r = G.miss(torch.nan_to_num(bad[n]), ref[n], ref[n + "_tol"])
        print(f"mutant {mutant}: {n} miss / tol {r:.0f}")
        assert r >= 100.0
    assert worst >= 100.0


def test_ssq_over_the_neighbouring_group_misses_by_100_tol():
    A, W, bias = G.operands(129, 576, 64, seed=1)
    ref, _, _ = G.linear_ref(A, W, 576, bias=bias)
    stored = ref.float()
    good, bad = G.ssq_ref(stored), G.ssq_ref(stored, group_shift=1)
    rel = ((bad - good).abs() / good).min()
    print(f"ssq neighbour group: smallest relative miss {float(rel):.3e} = {float(rel) / G.SSQ_RTOL:.0f} x 2^-18")
    assert float(((bad - good).abs() / good).max()) >= 100.0 * G.SSQ_RTOL
    assert float((bad - good).abs().div(good).median()) >= 100.0 * G.SSQ_RTOL
