"""CPU: the references of tests/attn_ref.py are themselves checked -- against torch's scaled_dot_product_attention, against loops
written out longhand, and the APB codec against its inverse -- and a sensitivity test shows that the comparisons of
tests/test_gpu_attention.py, at that module's own inputs and tolerances, would see each of the ways an attention kernel goes wrong
quietly: every mutant of the float64 reference misses the true one by at least 100 x the case's tolerance in every 32-query tile the
mutation touches."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R  # noqa: E402


# ---- 1. the definitions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,Tmax", [(1, 1, 1), (2, 33, 40), (2, 97, 128)])
def test_causal_gqa_ref_is_sdpa_on_the_expanded_heads(B, T, Tmax):
    q, k, v = R.prefill_inputs(B, T, Tmax)
    got = R.causal_gqa_ref(q, k, v, T)
    qq = q.double().view(B, T, 9, 64).permute(0, 2, 1, 3)
    kk = k[:, :, :T].double().repeat_interleave(3, dim=1)
    vv = v[:, :, :T].double().repeat_interleave(3, dim=1)
    want = torch.nn.functional.scaled_dot_product_attention(qq, kk, vv, is_causal=True).permute(0, 2, 1, 3).reshape(B, T, 576)
    assert got.dtype == torch.float64 and torch.isfinite(got).all()
    assert float((got - want).abs().max()) <= 1e-12
    # the rows of a launch with a past are the rows of the whole sequence
    if T > 32:
        past = R.causal_gqa_ref(q[:, 32:], k, v, T, qpos0=32)
        assert float((past - got[:, 32:]).abs().max()) <= 1e-12


@pytest.mark.parametrize("windows,nH,nW", [(3, 4, 0), (5, 4, 4), (2, 8, 2)])
def test_window_ref_is_the_longhand_loop(windows, nH, nW):
    c = R.window_case(windows, nH, nW)
    qkv, bias, mask = c["qkv"].double(), c["bias"].double(), c["mask"]
    C = 24 * nH
    scale = float(np.float32(24 ** -0.5))
    want = torch.zeros(windows * 64, C, dtype=torch.float64)
    for w in range(windows):
        rows = slice(64 * w, 64 * w + 64)
        for h in range(nH):
            qh = qkv[rows, h * 24:h * 24 + 24] * scale
            kh = qkv[rows, C + h * 24:C + h * 24 + 24]
            vh = qkv[rows, 2 * C + h * 24:2 * C + h * 24 + 24]
            s = qh @ kh.T + bias[h]
            if mask is not None:
                s = s + mask[w % nW].double()
            s = s - s.max(dim=1, keepdim=True).values
            p = torch.exp(s)
            want[rows, h * 24:h * 24 + 24] = (p / p.sum(dim=1, keepdim=True)) @ vh
    assert float((c["ref"] - want).abs().max()) <= 1e-12


# ---- 2. the APB codec ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [96, 576])
@pytest.mark.parametrize("M", [1, 97, 128, 389, 3 * 389])
def test_apb_decode_inverts_apb_encode(M, K):
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M + K)) * torch.logspace(-6, 3, K)[None, :]
    img = R.apb_encode(x)
    Mp = (M + 127) // 128 * 128
    assert img.dtype == torch.int32 and img.numel() * 4 == Mp * K * 6
    got, unowned, halves = R.apb_decode(img.numpy(), M, K)
    assert np.array_equal(got.numpy().view(np.int32), x.numpy().view(np.int32))
    # the unowned slots are exactly those of the rows >= M: three pieces per column octet each, and the encoder left them 0xFF
    assert int(unowned.sum()) == (Mp - M) * (K // 8) * 3
    whole, _, _ = R.apb_decode(img.numpy(), Mp, K)
    assert np.all(halves[unowned] == 0xFFFF) and np.all(halves[~unowned] != 0xFFFF)
    assert np.array_equal(whole[:M].numpy().view(np.int32), x.numpy().view(np.int32)) and bool(torch.isnan(whole[M:]).all())


def test_apb_slot_formula_spot_values():
    """the formula of common.h by hand at a few (m, k8, piece): K = 576 has 36 k16 steps"""
    s = R._apb_slots(256, 576)
    assert s[0, 0, 0] == 0 and s[0, 1, 0] == 32 and s[31, 1, 0] == 63 and s[32, 0, 0] == 64
    assert s[0, 0, 1] == 4 * 64 and s[0, 0, 2] == 8 * 64 and s[0, 2, 0] == 12 * 64
    assert s[128, 0, 0] == 36 * 12 * 64 and s[255, 71, 2] == 2 * 36 * 12 * 64 - 1


# ---- 3. sensitivity: what the GPU comparisons would catch ---------------------------------------------------------------------------
def _tiles_ok(diff, applies, tol, what):
    """diff [B][rows][cols]; applies bool [rows]: every 32-row tile with a row the mutation touches must differ by >= 100 tol"""
    worst = float("inf")
    for t0 in range(0, diff.shape[1], 32):
        a = applies[t0:t0 + 32]
        if not bool(a.any()):
            continue
        d = float(diff[:, t0:t0 + 32][:, a].max())
        worst = min(worst, d / tol)
        assert d >= 100 * tol, f"{what}: tile at row {t0} differs by {d:.3e} = {d / tol:.0f} x tol"
    return worst


@pytest.mark.parametrize("B,T,Tmax", R.PREFILL_SHAPES)
def test_prefill_mutants_are_far_from_the_reference(B, T, Tmax):
    c = R.prefill_case(B, T, Tmax)
    q, k, v, ref, tol = c["q"], c["k"], c["v"], c["ref"], c["tol"]
    assert 2.0 ** -20 * c["vmax"] <= tol <= 5e-5, tol
    t = torch.arange(T)
    causal = t[None, :] <= t[:, None]
    mutants = {
        "diagonal key dropped": (causal & ~((t[None, :] == t[:, None]) & (t[:, None] >= 1)), t >= 1),
        "key t + 1 admitted": (causal | (t[None, :] == t[:, None] + 1), t <= T - 2),
        "first key of a 32-key tile dropped": (causal & ~((t[None, :] % 32 == 0) & (t[None, :] < t[:, None])), t >= 1),
    }
    report = {}
    for what, (keep, applies) in mutants.items():
        if bool(applies.any()):
            mut = R.causal_gqa_ref(q, k, v, T, keep=keep)
            report[what] = _tiles_ok((mut - ref).abs(), applies, tol, what)
    swapped = R.causal_gqa_ref(q, k, v, T, kv_of=[1, 1, 1, 0, 0, 0, 2, 2, 2])
    report["two kv heads swapped"] = _tiles_ok((swapped - ref).abs(), t >= 0, tol, "kv heads swapped")
    print(f"B = {B}, T = {T}: tol {tol:.2e} (e_ref {c['e_ref']:.2e}); worst tile / tol: " + ", ".join(f"{k_} {v_:.0f}" for k_, v_ in report.items()))


@pytest.mark.parametrize("T,qpos0", R.PAST_CASES)
def test_past_rows_shifted_by_one_are_far_from_the_reference(T, qpos0):
    c = R.prefill_case(2, T, T + 7)
    ref = c["ref"]
    shifted = ref[:, qpos0 - 1:T - 1]              # row i of the past launch holding position qpos0 + i - 1
    worst = _tiles_ok((shifted - ref[:, qpos0:]).abs(), torch.ones(T - qpos0, dtype=torch.bool), c["tol"], "rows shifted by one")
    print(f"T = {T}, qpos0 = {qpos0}: worst tile / tol {worst:.0f}")


@pytest.mark.parametrize("windows,nH,nW", R.WINDOW_SHAPES)
def test_window_mutants_are_far_from_the_reference(windows, nH, nW):
    c = R.window_case(windows, nH, nW)
    ref, tol = c["ref"], c["tol"]
    assert 2.0 ** -20 * c["vmax"] <= tol <= 5e-5, tol
    rows = torch.ones(windows * 64, dtype=torch.bool)
    no_bias = R.window_ref(c["qkv"], c["bias"], c["mask"], nW, nH, use_bias=False)
    worst = {"bias omitted": _tiles_ok((no_bias - ref).abs()[None], rows, tol, "bias omitted")}
    if nW:
        other = R.window_ref(c["qkv"], c["bias"], c["mask"], nW, nH, mask_shift=1)
        worst["neighbouring window's mask"] = _tiles_ok((other - ref).abs()[None], rows, tol, "neighbouring mask")
        plain = R.window_ref(c["qkv"], c["bias"], None, 0, nH)
        worst["mask omitted"] = _tiles_ok((plain - ref).abs()[None], rows, tol, "mask omitted")
    print(f"windows = {windows}, nH = {nH}, nW = {nW}: tol {tol:.2e}; worst tile / tol: " + ", ".join(f"{k_} {v_:.0f}" for k_, v_ in worst.items()))
