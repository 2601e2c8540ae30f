"""GPU (-m gpu): the prefill and window attention kernels, ONE launch at a time on data this module chose, through the taps
mellow_debug_prefill_attn / mellow_debug_window_attn (include/mellow_hip.h) of an engine without weights.

Yardsticks (tests/attn_ref.py; tests/test_attn_ref_cpu.py checks them and shows what they would catch):
  * the float64 definition, within tol = max(16 * e_ref, 2^-20 * max|v|) per case, e_ref = |float32 - float64 evaluation| of the
    reference on the same inputs (the reference sets the tolerance, never the kernel).  The bf16-once variants add 2^-9 * max|v|:
    P is rounded once to bf16 before P . V while the denominator sums the unrounded P -- a bound, not a measurement;
  * bit identities derived from the code: bf16 pages == fp32 pages on bf16 values, APB form decoded == plain form, the launch with
    a past == the rows of the whole-sequence launch, an example of a batch == the same example alone, a call == its repetition;
  * causality by bits: changing keys at positions >= t0 changes no bit of the rows < t0;
  * guards: the taps fill the output with 0xFF bytes first, so rows / APB slots no real row owns must still hold them.
The pages hold NaN at every position >= T (Tmax > T): the kernels must never read them.  Every test prints max error / tol
(DESIGN.md 6l is where the figures belong)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from mellow_amd import engine as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = E.Engine(device=0)          # no weights: the taps work on an engine that is not finalised
    yield e
    e.close()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _unpack(out, M, width, out_form):
    """the tap's whole output -> the M real rows [M][width], after the guard check: nothing but the real rows was written"""
    if out_form == 0:
        assert out.shape == (M + 32, width)
        assert bool((_bits(out[M:]) == -1).all()), "rows after M were written"
        return out[:M]
    x, unowned, halves = R.apb_decode(out.numpy(), M, width)
    assert np.all(halves[unowned] == 0xFFFF), "an APB slot no real row owns was written"
    assert np.all(halves[~unowned] != 0xFFFF), "an APB slot of a real row was not written (or holds a NaN)"
    return x


def prefill(engine, q, k, v, T, variant, qpos0=0, out_form=0):
    B = k.shape[0]
    out = engine.debug_prefill_attn(q, k, v, T, variant=variant, qpos0=qpos0, out_form=out_form)
    return _unpack(out, B * (T - qpos0), 576, out_form).view(B, T - qpos0, 576)


def window(engine, c, in16=False, out_form=0):
    qkv = c["qkv"]
    out = engine.debug_window_attn(qkv, c["bias"], c["mask"], in16=in16, out_form=out_form)
    return _unpack(out, qkv.shape[0], qkv.shape[1] // 3, out_form)


def _ratio(what, got, ref, tol):
    assert bool(torch.isfinite(got).all()), f"{what}: a non-finite output (a page position >= T was read?)"
    err = float((got.double() - ref).abs().max())
    print(f"ATTN {what}: max|err| {err:.3e}, tol {tol:.3e}, err / tol {err / tol:.3f}")
    return err


# ---- prefill: against float64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("B,T,Tmax", R.PREFILL_SHAPES)
def test_prefill_fp32_variants_against_float64(engine, B, T, Tmax, variant):
    """exact fp32 MFMA kernel (0) and f32x3 kernel (1), plain form, within the fp32 tolerance; three calls give equal bits (a missed
    barrier in the loader ring would show as a flaky row)"""
    c = R.prefill_case(B, T, Tmax)
    got = prefill(engine, c["q"], c["k"], c["v"], T, variant)
    err = _ratio(f"prefill variant {variant} (B, T, Tmax) = ({B}, {T}, {Tmax})", got, c["ref"], c["tol"])
    for _ in range(2):
        assert _same_bits(prefill(engine, c["q"], c["k"], c["v"], T, variant), got)
    assert err <= c["tol"]


@pytest.mark.parametrize("B,T,Tmax", R.PREFILL_SHAPES)
def test_prefill_bf16_once_variants(engine, B, T, Tmax):
    """variants 2 (fp32 pages) and 3 (bf16 pages, bf16 q rows) on bf16-representable inputs: within 2^-9 max|v| + the fp32
    tolerance of the float64 reference of those inputs, and equal to each other bit for bit (same staging indices and MFMA order,
    only the loads differ)"""
    c = R.prefill_case(B, T, Tmax, True)
    tol = 2.0 ** -9 * c["vmax"] + c["tol"]
    got2 = prefill(engine, c["q"], c["k"], c["v"], T, 2)
    got3 = prefill(engine, c["q"], c["k"], c["v"], T, 3)
    e2 = _ratio(f"prefill variant 2 (B, T, Tmax) = ({B}, {T}, {Tmax})", got2, c["ref"], tol)
    e3 = _ratio(f"prefill variant 3 (B, T, Tmax) = ({B}, {T}, {Tmax})", got3, c["ref"], tol)
    for variant, got in ((2, got2), (3, got3)):
        for _ in range(2):
            assert _same_bits(prefill(engine, c["q"], c["k"], c["v"], T, variant), got)
    assert e2 <= tol and e3 <= tol
    assert _same_bits(got3, got2), f"bf16 pages differ from fp32 pages in {int((_bits(got3) != _bits(got2)).sum())} words"


# ---- prefill: bit identities --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("B,T,Tmax", R.PREFILL_SHAPES)
def test_prefill_apb_form_decodes_to_the_plain_form(engine, B, T, Tmax, variant):
    """split8 is exact: the three bf16 pieces of every element sum to the fp32 value the plain form stores"""
    c = R.prefill_case(B, T, Tmax)
    plain = prefill(engine, c["q"], c["k"], c["v"], T, variant)
    apb = prefill(engine, c["q"], c["k"], c["v"], T, variant, out_form=1)
    assert _same_bits(apb, plain), f"{int((_bits(apb) != _bits(plain)).sum())} words differ"


@pytest.mark.parametrize("out_form", [0, 1])
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("T,qpos0", R.PAST_CASES)
def test_prefill_past_launch_equals_the_rows_of_the_whole_launch(engine, T, qpos0, variant, out_form):
    """a query visits the key tiles it visits in the whole-sequence launch, in the same order"""
    c = R.prefill_case(2, T, T + 7)
    whole = prefill(engine, c["q"], c["k"], c["v"], T, variant)
    past = prefill(engine, c["q"][:, qpos0:], c["k"], c["v"], T, variant, qpos0=qpos0, out_form=out_form)
    _ratio(f"prefill past variant {variant} form {out_form} (T, qpos0) = ({T}, {qpos0})", past, c["ref"][:, qpos0:], c["tol"])
    assert _same_bits(past, whole[:, qpos0:]), f"{int((_bits(past) != _bits(whole[:, qpos0:])).sum())} words differ"


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_prefill_example_of_a_batch_equals_the_example_alone(engine, variant):
    """B = 3, Tmax != T, every (example, kv head) page from its own seed: the b * 3 + g page stride and the row of (b, t), in the
    whole-sequence launch (plain and APB) and in the launch with a past"""
    B, T, Tmax = 3, 97, 128
    q, k, v = R.prefill_inputs(B, T, Tmax, variant >= 2)
    forms = [(0, 0)] + ([(0, 1), (64, 0), (64, 1)] if variant < 2 else [])
    for qpos0, out_form in forms:
        batch = prefill(engine, q[:, qpos0:], k, v, T, variant, qpos0=qpos0, out_form=out_form)
        for b in range(B):
            alone = prefill(engine, q[b:b + 1, qpos0:], k[b:b + 1], v[b:b + 1], T, variant, qpos0=qpos0, out_form=out_form)
            assert _same_bits(alone[0], batch[b]), (variant, qpos0, out_form, b)


# ---- prefill: causality by bits -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("B,T,Tmax", [s for s in R.PREFILL_SHAPES if s[1] > 1])
def test_prefill_rows_before_t0_ignore_the_keys_from_t0(engine, B, T, Tmax, variant):
    """k and v at positions >= t0 replaced by +-1024 (finite: 0 . NaN in the P . V MFMA would be NaN by construction, and the
    engine never has that): no bit of the rows < t0 may change"""
    q, k, v = R.prefill_inputs(B, T, Tmax, variant >= 2)
    base = prefill(engine, q, k, v, T, variant)
    big = torch.where(torch.randn(B, 3, T, 64, generator=torch.Generator().manual_seed(7)) < 0, -1024.0, 1024.0)
    for t0 in sorted({t for t in (1, 31, 32, 33, T - 1) if 1 <= t < T}):
        k2, v2 = k.clone(), v.clone()
        k2[:, :, t0:T] = big[:, :, t0:]
        v2[:, :, t0:T] = big[:, :, t0:]
        got = prefill(engine, q, k2, v2, T, variant)
        assert _same_bits(got[:, :t0], base[:, :t0]), f"t0 = {t0}: {int((_bits(got[:, :t0]) != _bits(base[:, :t0])).sum())} words of the rows before it changed"
        assert not _same_bits(got[:, t0:], base[:, t0:])          # (the change itself is seen by the rows that may see it)


# ---- prefill: refusals --------------------------------------------------------------------------------------------------------------
def _raw_prefill(engine, variant, B, T, Tmax, qpos0, out_form, capacity=None):
    """the C entry itself on zero-filled arrays large enough for any reading of the arguments -> (return code, message)"""
    rows = B * max(T, 1)
    q = torch.zeros(rows * 576)
    kv = torch.zeros(B * 3 * max(T, Tmax, 1) * 64)
    out = torch.zeros((rows + 160) * 576 * 2)
    cap = out.numel() * 4 if capacity is None else capacity
    rc = engine.lib.mellow_debug_prefill_attn(engine.h, variant, C.c_void_p(q.data_ptr()), C.c_void_p(kv.data_ptr()), C.c_void_p(kv.data_ptr()),
                                              B, T, Tmax, qpos0, out_form, C.c_void_p(out.data_ptr()), cap)
    return rc, engine.lib.mellow_last_error().decode()


def test_prefill_tap_refuses_what_the_engine_never_launches(engine):
    bad = {
        "Tmax < T": ((0, 2, 64, 63, 0, 0), "below T"),
        "qpos0 % 32 != 0": ((0, 2, 64, 64, 16, 0), "multiple of 32"),
        "qpos0 == T": ((0, 2, 64, 64, 64, 0), "multiple of 32 in"),
        "qpos0 > T": ((1, 2, 64, 64, 96, 0), "multiple of 32 in"),
        "past with variant 2": ((2, 2, 64, 64, 32, 0), "variants 0 and 1 only"),
        "past with variant 3": ((3, 2, 64, 64, 32, 0), "variants 0 and 1 only"),
        "APB with variant 2": ((2, 2, 64, 64, 0, 1), "variants 0 and 1 only"),
        "APB with variant 3": ((3, 2, 64, 64, 0, 1), "variants 0 and 1 only"),
        "variant 4": ((4, 2, 64, 64, 0, 0), "variant must be"),
    }
    for what, (args, text) in bad.items():
        rc, msg = _raw_prefill(engine, *args)
        assert rc != 0 and text in msg, (what, rc, msg)
    for out_form, need in ((0, (2 * 64 + 32) * 576 * 4), (1, 128 * 576 * 6)):
        rc, msg = _raw_prefill(engine, 0, 2, 64, 64, 0, out_form, capacity=need - 1)
        assert rc != 0 and "out_capacity" in msg, (out_form, rc, msg)
        assert _raw_prefill(engine, 0, 2, 64, 64, 0, out_form, capacity=need)[0] == 0
    with pytest.raises(E.EngineError, match="below T"):
        q, k, v = R.prefill_inputs(1, 33, 64)
        engine.debug_prefill_attn(q, k[:, :, :32], v[:, :, :32], 33)
    # the engine is still usable: a good call afterwards is still right
    c = R.prefill_case(1, 33, 64)
    got = prefill(engine, c["q"], c["k"], c["v"], 33, 1)
    assert float((got.double() - c["ref"]).abs().max()) <= c["tol"]


# ---- window attention ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("windows,nH,nW", R.WINDOW_SHAPES)
def test_window_against_float64(engine, windows, nH, nW):
    """fp32 input, plain form; nW mutually different masks over more windows than masks make `window % nW` observable"""
    c = R.window_case(windows, nH, nW)
    got = window(engine, c)
    err = _ratio(f"window (windows, nH, nW) = ({windows}, {nH}, {nW})", got, c["ref"], c["tol"])
    for _ in range(2):
        assert _same_bits(window(engine, c), got)
    assert err <= c["tol"]


@pytest.mark.parametrize("windows,nH,nW", R.WINDOW_SHAPES)
def test_window_bf16_input_equals_fp32_input_on_bf16_values(engine, windows, nH, nW):
    """the arithmetic after the load is unchanged"""
    c = R.window_case(windows, nH, nW, True)
    want = window(engine, c)
    got = window(engine, c, in16=True)
    err = _ratio(f"window in16 (windows, nH, nW) = ({windows}, {nH}, {nW})", got, c["ref"], c["tol"])
    assert err <= c["tol"]
    assert _same_bits(got, want), f"{int((_bits(got) != _bits(want)).sum())} words differ"


@pytest.mark.parametrize("windows,nH,nW", R.WINDOW_SHAPES)
def test_window_apb_form_decodes_to_the_plain_form(engine, windows, nH, nW):
    """K = C; at windows = 3 (M = 192) the rows 192..255 of the image stay untouched; covers the h == 0 store of columns 16..23"""
    c = R.window_case(windows, nH, nW)
    plain = window(engine, c)
    apb = window(engine, c, out_form=1)
    assert _same_bits(apb, plain), f"{int((_bits(apb) != _bits(plain)).sum())} words differ"


def _raw_window(engine, M, Cw, nH, with_mask, nW, in16, out_form, capacity=None):
    qkv = torch.zeros(max(M, 64) * 3 * max(Cw, 96))
    bias = torch.zeros(max(nH, 32) * 64 * 64)
    mask = torch.zeros(max(nW, 1) * 64 * 64)
    out = torch.zeros((max(M, 64) + 160) * max(Cw, 96) * 2)
    cap = out.numel() * 4 if capacity is None else capacity
    rc = engine.lib.mellow_debug_window_attn(engine.h, C.c_void_p(qkv.data_ptr()), M, Cw, nH, C.c_void_p(bias.data_ptr()),
                                             C.c_void_p(mask.data_ptr()) if with_mask else None, nW, in16, out_form,
                                             C.c_void_p(out.data_ptr()), cap)
    return rc, engine.lib.mellow_last_error().decode()


def test_window_tap_refuses_what_the_engine_never_launches(engine):
    bad = {
        "M % 64 != 0": ((96, 96, 4, False, 0, 0, 0), "multiple of 64"),
        "M == 0": ((0, 96, 4, False, 0, 0, 0), "multiple of 64"),
        "C != 24 nH": ((64, 128, 4, False, 0, 0, 0), "24 * nH"),
        "nH == 6": ((64, 144, 6, False, 0, 0, 0), "head count"),
        "nH == 64": ((64, 1536, 64, False, 0, 0, 0), "head count"),
        "mask with nW == 0": ((64, 96, 4, True, 0, 0, 0), "nW >= 1"),
        "mask with nW < 0": ((64, 96, 4, True, -2, 0, 0), "nW >= 1"),
        "in16 with APB": ((64, 96, 4, False, 0, 1, 1), "never launches"),
    }
    for what, (args, text) in bad.items():
        rc, msg = _raw_window(engine, *args)
        assert rc != 0 and text in msg, (what, rc, msg)
    for out_form, need in ((0, (64 + 32) * 96 * 4), (1, 128 * 96 * 6)):
        rc, msg = _raw_window(engine, 64, 96, 4, False, 0, 0, out_form, capacity=need - 1)
        assert rc != 0 and "out_capacity" in msg, (out_form, rc, msg)
        assert _raw_window(engine, 64, 96, 4, False, 0, 0, out_form, capacity=need)[0] == 0
    c = R.window_case(3, 4, 0)
    assert float((window(engine, c).double() - c["ref"]).abs().max()) <= c["tol"]
