"""CPU: the references of tests/norm_ref.py checked against torch, the AMX codec against itself and against the layout text, the
tolerance rule against float32 emulations in four summation orders, the two ambiguity caps on the seeded inputs, and the mutants of
the sensitivity test: each must FAIL somewhere under the same comparison functions tests/test_gpu_norm.py calls."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R  # noqa: E402
import gemm_ref as G  # noqa: E402
import norm_ref as N  # noqa: E402


# ---- definitions ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", [(33, 96), (31, 576), (12, 1536)])
def test_layernorm_definition_is_torch_layer_norm_in_float64(M, C):
    x, w, b = N.rows(M, C)
    y, tol = N.layernorm_ref(x, w, b)
    want = torch.nn.functional.layer_norm(x.double(), (C,), w.double(), b.double(), eps=1e-5)
    # float64 itself cancels on the large-mean row (mean 1000, spread 1e-3: 1e6 * 2^-53): the two evaluations agree to a part in 1e5
    # of the float32 tolerance there and to 1e-12 everywhere
    assert bool(((y - want).abs() <= 1e-5 * tol + 1e-12).all())
    assert bool((tol >= 0).all()) and bool(torch.isfinite(tol).all())
    z = N.special_rows(M)[3]
    assert torch.equal(y[z], b.double()) and float(tol[z].max()) <= 2 * N.U * float(b.abs().max())      # the all-zero row: y = b


@pytest.mark.parametrize("M,C,eps", [(33, 64, 1e-5), (129, 576, 1e-5), (33, 576, 0.0)])
def test_rmsnorm_definition_is_the_hand_written_formula(M, C, eps):
    x, w, _ = N.rows(M, C, zero_row=eps > 0)
    y, tol = N.rmsnorm_ref(x, w, eps)
    for m in range(M):
        r = 1.0 / np.sqrt(float((x[m].double() ** 2).sum()) / C + eps)
        assert float((y[m] - w.double() * x[m].double() * r).abs().max()) <= 1e-12 * max(1.0, float(y[m].abs().max()))
    assert bool(torch.isfinite(y).all()) and torch.equal(tol, y.abs() * (((C + 2) / 2 + 5) * N.U))


@pytest.mark.parametrize("R_,shift,M", N.LN_MAPPED)
def test_row_map_is_a_gather_of_whole_token_groups(R_, shift, M):
    rm, ntok = G.window_map(R_, shift)
    src = N.src_rows(M, rm)
    assert ntok == R_ * R_ and torch.equal(torch.sort(src).values, torch.arange(M))
    tok = torch.arange(M).view(M // ntok, R_, R_)
    rolled = torch.roll(tok, shifts=(-shift, -shift), dims=(1, 2)) if shift else tok
    want = rolled.view(M // ntok, R_ // 8, 8, R_ // 8, 8).permute(0, 1, 3, 2, 4).reshape(-1)
    assert torch.equal(src, want)
    x, w, b = N.rows(M, 96)
    y, _ = N.layernorm_ref(x, w, b, rm)
    assert torch.equal(y, N.layernorm_ref(x[src], w, b)[0])


@pytest.mark.parametrize("n,R_,Cin", N.MERGE_CASES)
def test_merge_gather_is_the_2x2_patch_view(n, R_, Cin):
    x, w, b = N.merge_tokens(n, R_, Cin)
    v = x.view(n, R_ // 2, 2, R_ // 2, 2, Cin)                       # [clip][i][di][j][dj][c]: token (2i + di, 2j + dj)
    want = torch.cat([v[:, :, 0, :, 0], v[:, :, 1, :, 0], v[:, :, 0, :, 1], v[:, :, 1, :, 1]], dim=-1).reshape(-1, 4 * Cin)
    got = N.merge_gather(x, n, R_)
    assert torch.equal(got, want)
    assert torch.equal(got, N.rows(n * (R_ // 2) ** 2, 4 * Cin, seed=R_)[0])      # the special rows are special OUTPUT rows


def test_inputs_are_finite_without_denormals_and_hold_the_special_rows():
    for M, C in [(200, 96), (33, 768), (389, 576)]:
        x, w, b = N.rows(M, C)
        assert bool(torch.isfinite(x).all()) and not bool(((x != 0) & (x.abs() < 2.0 ** -126)).any())
        sp = N.special_rows(M)
        assert len(sp) == 5 and len(set(sp)) == 5
        big, near, const, zero, hot = (x[i].double() for i in sp)
        assert abs(float(big.mean())) > 50 and float(big.std()) < 0.02
        assert 1e-6 < float(near.var(unbiased=False)) < 1e-4
        assert float(const.std()) == 0 and float(const[0]) != 0
        assert not bool(zero.any())
        assert int((hot != 0).sum()) == 1
        assert int((w == 0).sum()) == 1 and int((w < 0).sum()) == 1 and 0.69 < float(w.abs()[w != 0].min()) and float(w.abs().max()) < 1.31
        assert len({float(x[i].abs().mean()) for i in range(M)}) == M
    assert N.special_rows(1) == []
    p = N.plain_rows(389, 576)
    assert bool(torch.isfinite(p).all()) and not bool(((p != 0) & (p.abs() < 2.0 ** -126)).any())
    blk = p.view(389, 18, 32)
    amax = blk.abs().amax(dim=2)
    for n in (-20, 0, 20):
        a = torch.tensor(448.0 * 2.0 ** n)
        for v in (torch.nextafter(a, torch.tensor(0.0)), a, torch.nextafter(a, torch.tensor(float("inf")))):
            assert bool((amax == v).any()), (n, float(v))
    assert bool(((amax == 0) & (blk.view(torch.int32) == -2 ** 31).all(dim=2)).any())                     # the block of -0.0
    assert bool((amax > 1e29).any()) and bool(((amax < 1e-29) & (amax > 0)).any())
    assert bool(((blk == 2.0 ** -10).any(dim=2) & (blk == 3 * 2.0 ** -10).any(dim=2) & (amax == 448)).any())


# ---- AMX codec ---------------------------------------------------------------------------------------------------------------------------
def test_amx_layout_against_the_formulas_spelled_out():
    """amx_decode against a scalar transcription of the two address formulas"""
    M, C = 200, 224
    KT64, KQ = N.amx_dims(C)
    assert (KT64, KQ) == (4, 1) and N.amx_dims(384) == (6, 2) and N.amx_dims(768) == (12, 3) and N.amx_dims(96) == (2, 1)
    g = torch.Generator().manual_seed(1)
    data = torch.randint(0, 120, (256 * KT64 * 64,), generator=g, dtype=torch.uint8)
    sc = torch.randint(100, 150, (256 * 8 * KQ,), generator=g, dtype=torch.uint8)
    val, E, byt, d_un, s_un = N.amx_decode(data, sc, M, C)
    lut = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double()
    for m, k in [(0, 0), (1, 17), (31, 63), (32, 64), (127, 255), (128, 0), (199, 223), (160, 100), (77, 48)]:
        s, j, h = k // 64, (k // 32) % 2, (k // 16) % 2
        slot = ((((m >> 7) * KT64 + s) * 4 + ((m >> 5) & 3)) * 2 + j) * 64 + (m & 31) + 32 * h
        sb = ((((m >> 7) * KQ + (s >> 2)) * 4 + ((m >> 5) & 3)) * 64 + (m & 31) + 32 * j) * 4 + (s & 3)
        assert int(byt[m, k]) == int(data[slot * 16 + k % 16]) and int(E[m, k // 32]) == int(sc[sb])
        assert float(val[m, k]) == float(lut[int(data[slot * 16 + k % 16])] * 2.0 ** (int(sc[sb]) - 127))
    assert int(d_un.sum()) == 56 * KT64 * 64 and int(s_un.sum()) == 56 * 2 * KT64          # KT64 = 4: every byte of a scale word is a step


@pytest.mark.parametrize("M,C", [(1, 64), (70, 96), (70, 100), (129, 224), (200, 384), (33, 768)])
@pytest.mark.parametrize("pad_rows", ["ff", "zero"])
def test_amx_encode_decode_round_trip(M, C, pad_rows):
    x = N.plain_rows(M, C)
    data, sc = N.amx_encode(x, pad_rows)
    KT64, KQ = N.amx_dims(C)
    assert data.numel() == N.rup(M, 128) * KT64 * 64 and sc.numel() == N.rup(M, 128) * 8 * KQ
    assert N.amx_guards(data, sc, M, C, pad_rows) == []
    assert N.amx_guards(data, sc, M, C, "zero" if pad_rows == "ff" else "ff") != [] or M % 128 == 0
    val, E, byt, _, _ = N.amx_decode(data, sc, M, C)
    # the decoded value is the e4m3 rounding of x at the block's scale: within half a step, never clipped, zero pads
    blk = torch.zeros(M, KT64 * 64)
    blk[:, :C] = x
    amax = blk.view(M, -1, 32).abs().amax(dim=2)
    Ew = N.mx8_exponent(amax)
    assert torch.equal(E.to(torch.int64), Ew) and torch.equal(Ew, N.mx8_exponent_kernel_f32(amax))
    scale = torch.exp2((Ew - 127).double())
    assert bool((amax.double() <= 448 * scale).all()) and bool(((amax.double() > 224 * scale) | (amax == 0) | (Ew == 1)).all())
    want = N.e4m3_rne(blk.double().view(M, -1, 32) / scale[:, :, None]) * scale[:, :, None]
    assert torch.equal(val.double().view(M, -1, 32), want)                       # the float64 rounding is torch's float8 conversion
    assert torch.equal(byt[blk == 0] & 0x7F, torch.zeros_like(byt[blk == 0]))
    neg0 = (blk.view(torch.int32) == -2 ** 31)
    assert bool((byt[neg0] == 0x80).all())
    assert N.amx_same(data, sc, x, pad_rows) == []
    # exact zero tolerance: the bracket is the value itself
    bad, far, off = N.amx_bracket(data, sc, M, C, x.double(), torch.zeros(M, C, dtype=torch.float64))
    assert bad == [] and far == 0 and off == 0


def test_e4m3_ties_and_subnormals():
    t = torch.tensor([2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -9, 5 * 2.0 ** -10, 448.0, 460.0, 1e9, -0.0, 17.0, 19.0, 0.9 * 2.0 ** -10], dtype=torch.float64)
    want = torch.tensor([0.0, 2.0 ** -8, 2.0 ** -9, 2.0 ** -8, 448.0, 448.0, 448.0, -0.0, 16.0, 20.0, 0.0], dtype=torch.float64)
    assert torch.equal(N.e4m3_rne(t), want) and torch.equal(N.e4m3_rne(-t), -want)
    x = torch.randn(20000, generator=torch.Generator().manual_seed(3)) * torch.exp2(torch.randint(-12, 9, (20000,), generator=torch.Generator().manual_seed(4)).float())
    x = x.clamp(-448, 448)
    assert torch.equal(N.e4m3_rne(x.double()), x.to(torch.float8_e4m3fn).double())


def test_exponent_rule_at_the_edges():
    f = lambda v: int(N.mx8_exponent(torch.tensor([v], dtype=torch.float32))[0])      # noqa: E731
    a = torch.tensor(448.0)
    assert f(448.0) == 127 and f(float(torch.nextafter(a, torch.tensor(1e9)))) == 128 and f(float(torch.nextafter(a, torch.tensor(0.0)))) == 127
    assert f(224.0) == 126 and f(224.5) == 127 and f(0.0) == 127 and f(1.0) == 119 and f(1e-38) == 1 and f(3.4e38) == 247
    for n in (-20, 0, 20):
        for v in (torch.nextafter(a * 2.0 ** n, torch.tensor(0.0)), a * 2.0 ** n, torch.nextafter(a * 2.0 ** n, torch.tensor(float("inf")))):
            assert int(N.mx8_exponent(v[None])[0]) == int(N.mx8_exponent_kernel_f32(v[None])[0])


# ---- tolerance against float32 emulations --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [96, 768, 1536])
def test_layernorm_tolerance_holds_float32_in_four_orders_and_the_mutant_table(C):
    x, w, b = N.rows(33, C)
    y, tol = N.layernorm_ref(x, w, b)
    worst = max(N.miss(N.layernorm_f32(x, w, b, o), y, tol) for o in N.ORDERS)
    ratios = {m: N.miss(N.layernorm_ref(x, w, b, mutant=m)[0], y, tol) for m in ("eps", "unbiased")}
    ratios["one_pass"] = max(N.miss(N.layernorm_f32(x, w, b, o, mutant="one_pass"), y, tol) for o in N.ORDERS)
    print(f"NORM-REF LayerNorm C = {C}: float32 in four orders max err / tol {worst:.3f}; mutants " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert worst <= 1.0
    assert ratios["eps"] > 1.0 and ratios["unbiased"] > 1.0
    # what the rule does and does not catch: the any-order bound grows with C, a one-pass variance hides under it at wide rows
    if C == 96:
        assert ratios["one_pass"] > 1.0


@pytest.mark.parametrize("C", [64, 576])
def test_rmsnorm_tolerance_holds_float32_in_four_orders(C):
    for eps, zero in ((1e-5, True), (0.0, False)):
        x, w, _ = N.rows(33, C, zero_row=zero)
        y, tol = N.rmsnorm_ref(x, w, eps)
        worst = max(N.miss(N.rmsnorm_f32(x, w, eps, o), y, tol) for o in N.ORDERS)
        wrong = N.miss(N.rmsnorm_ref(x, w, 1e-6 if eps else 1e-5)[0], y, tol)
        print(f"NORM-REF RMSNorm C = {C} eps = {eps}: float32 max err / tol {worst:.3f}; another eps {wrong:.3g}")
        assert worst <= 1.0 and wrong > 1.0


# ---- the ambiguity caps: a condition on the inputs, from the reference alone -----------------------------------------------------------------
def _ln_family(C):
    for M in N.LN_M:
        x, w, b = N.rows(M, C)
        yield N.layernorm_ref(x, w, b)
    for R_, shift, M in N.LN_MAPPED:
        x, w, b = N.rows(M, C)
        yield N.layernorm_ref(x, w, b, G.window_map(R_, shift)[0])


def _rms_family(C):
    for M in N.RMS_M:
        x, w, _ = N.rows(M, C)
        yield N.rmsnorm_ref(x, w, 1e-5)
    x, w, _ = N.rows(33, C, zero_row=False)
    yield N.rmsnorm_ref(x, w, 0.0)


@pytest.mark.parametrize("family,C", [("ln", c) for c in N.LN_C] + [("rms", c) for c in N.RMS_C])
def test_ambiguity_of_the_amx_yardstick_stays_under_its_caps(family, C):
    el = n_el = bl = n_bl = 0
    for y, tol in (_ln_family(C) if family == "ln" else _rms_family(C)):
        a, b, c, d = N.ambiguity(y, tol, C)
        el, n_el, bl, n_bl = el + a, n_el + b, bl + c, n_bl + d
    print(f"NORM-REF ambiguity {family} C = {C}: {100.0 * el / n_el:.3f} % of elements, {100.0 * bl / n_bl:.3f} % of blocks")
    assert el / n_el < 0.02 and bl / n_bl < 0.01


# ---- the mutants: every one fails under the comparison the GPU module makes ------------------------------------------------------------------
def test_definition_mutants_fail_the_float64_comparison():
    x, w, b = N.rows(129, 96)
    y, tol = N.layernorm_ref(x, w, b)
    assert N.miss(y.float(), y, tol) <= 1.0
    for m in ("eps", "unbiased"):
        assert N.miss(N.layernorm_ref(x, w, b, mutant=m)[0].float(), y, tol) > 1.0, m
    # (window_map(8, 0) is the identity: one window, no shift -- only the shifted 16 x 16 map can tell a map from its inverse)
    rm, _ = G.window_map(16, 4)
    x, w, b = N.rows(512, 96)
    y, tol = N.layernorm_ref(x, w, b, rm)
    assert N.miss(N.layernorm_ref(x, w, b, rm, mutant="map_inverted")[0].float(), y, tol) > 1.0
    for n, R_, Cin in N.MERGE_CASES:
        x, w, b = N.merge_tokens(n, R_, Cin)
        y, tol = N.merge_layernorm_ref(x, n, R_, w, b)
        assert N.miss(N.merge_layernorm_ref(x, n, R_, w, b, mutant="swap12")[0].float(), y, tol) > 1.0, (n, R_, Cin)


@pytest.mark.parametrize("C", [96, 384, 768])
def test_image_mutants_fail_the_image_comparisons(C):
    M = 33
    x, w, b = N.rows(M, C)
    y, tol = N.layernorm_ref(x, w, b)
    y32 = y.float()
    good = N.amx_encode(y32)
    assert N.amx_guards(*good, M, C, "ff") == [] and N.amx_bracket(*good, M, C, y, tol)[0] == [] and N.amx_same(*good, y32, "ff") == []
    # scale exponent + 1: the bytes differ, and the exponent leaves the admissible range of (nearly) every block
    d, s = N.amx_encode(y32, mutant="exp_plus1")
    assert N.amx_same(d, s, y32, "ff") != [] and any("scale bytes outside" in t for t in N.amx_bracket(d, s, M, C, y, tol)[0])
    # scale byte at position s instead of s % 4: the same address while KT64 <= 4, so it can show from C = 384 (KT64 = 6) on
    d, s = N.amx_encode(y32, mutant="scale_pos")
    if C == 96:
        assert N.amx_same(d, s, y32, "ff") == []
    else:
        assert N.amx_same(d, s, y32, "ff") != []
        assert N.amx_guards(d, s, M, C, "ff") != [] or N.amx_bracket(d, s, M, C, y, tol)[0] != []
    # non-zero pad columns (C = 96: the last 32-column block is all padding)
    if C == 96:
        d, s = N.amx_encode(y32, mutant="pad_nonzero")
        bad = N.amx_guards(d, s, M, C, "ff")
        assert any("pad column" in t for t in bad) and any("all-pad block" in t for t in bad) and N.amx_same(d, s, y32, "ff") != []
    # a value mutant under the bracket: the eps = 1e-6 definition, encoded
    d, s = N.amx_encode(N.layernorm_ref(x, w, b, mutant="eps")[0].float())
    assert N.amx_bracket(d, s, M, C, y, tol)[0] != []
    # a row >= M written, and a real row left unwritten
    d, s = N.amx_encode(torch.cat([y32, y32[:1]]))
    assert N.amx_guards(d, s, M, C, "ff") != []
    d, s = N.amx_encode(y32[:M - 1])
    assert N.amx_guards(d, s, M, C, "ff") != []


def test_apb_unpack_holds_the_two_guard_conventions_and_the_sign_of_zero():
    x = N.plain_rows(70, 96)
    img = R.apb_encode(x)
    got, bad = N.apb_unpack(img, 70, 96, "ff")
    assert bad == [] and N.same_bits(got, x)
    assert N.apb_unpack(img, 70, 96, "zero")[1] != []
    z = R.apb_encode(torch.cat([x, torch.zeros(58, 96)]))
    got, bad = N.apb_unpack(z, 70, 96, "zero")
    assert bad == [] and N.same_bits(got, x) and N.apb_unpack(z, 70, 96, "ff")[1] != []
    assert N.apb_unpack(R.apb_encode(x[:69]), 70, 96, "ff")[1] != []
