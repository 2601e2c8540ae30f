"""GPU (-m gpu): the norm kernels and the producers of the APB / MXFP8 hand-over images, ONE launch at a time on data this module chose,
through the tap mellow_debug_norm (include/mellow_hip.h) of an engine without weights: layernorm_kernel<0> (plain and row-map gather),
layernorm_kernel<1> (patch merging), layernorm_apb_kernel<NQ, AMX>, rmsnorm_kernel, rmsnorm_apb_kernel<AMX>, split_rows_apb_kernel and
quant_mx8_kernel.

Yardsticks (tests/norm_ref.py; tests/test_norm_ref_cpu.py checks them and shows the mutants they catch):
  A. the float64 definition: fp32 rows and the decoded APB image per element within the tolerance derived there from the reference
     alone; the AMX image by the bracket Q(y - tol) <= g <= Q(y + tol) at the exponent the kernel chose, that exponent within the
     admissible range of the reference;
  B. bit identities stated by the code: the APB image decoded == the fp32 rows word for word; the AMX data and scale bytes ==
     amx_encode of the fp32 rows byte for byte; launch_split_rows_apb decoded == its input, launch_quant_mx8 == amx_encode(input); a
     launch == its repetition; rows [0, M1) of an M2-row launch == the M1-row launch;
  C. guards, per producer: the norm kernels leave rows >= M of the last 128-row panel untouched (0xFF data and scale bytes), the two
     stand-alone producers write them as zeros (scale byte 127); scale bytes of k64 steps >= KT64 inside a scale word stay 0xFF; pad
     columns [C, rup(C, 64)) are +0.0 and an all-pad block has scale 127; the fp32 rows [M, M + 32) stay 0xFF; every owned word is
     written and finite;
  D. refusals by name.
Every case prints max err / tol (DESIGN.md 6r is where the figures belong)."""
import ctypes
import os
import sys

import pytest
import torch

from mellow_amd import engine as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_ref as G  # noqa: E402
import norm_ref as N  # noqa: E402

pytestmark = pytest.mark.gpu

LN_CASES = [(M, None) for M in N.LN_M] + [(M, (R_, shift)) for R_, shift, M in N.LN_MAPPED]


@pytest.fixture(scope="module")
def engine():
    e = E.Engine(device=0)          # no weights: the tap works on an engine that is not finalised
    yield e
    e.close()


def _bits(t):
    return t.contiguous().view(torch.int32)


def unpack_y(out, M, width):
    """the tap's fp32 rows [M + 32][width] -> [M][width] after the guard checks"""
    y = out["y"]
    assert y.shape == (M + 32, width)
    assert bool((_bits(y[M:]) == -1).all()), "fp32 rows [M, M + 32) were written"
    assert bool(torch.isfinite(y[:M]).all()), "an owned word was not written (or is not finite)"
    return y[:M]


def check_forms(engine, what, op, x, M, C, y, tol, pad_rows="ff", **kw):
    """forms 0, 1 and 2 of one norm case: A, B, C of the module docstring, and each launch against its repetition"""
    f0 = engine.debug_norm(x, op=op, form=0, **kw)
    y0 = unpack_y(f0, M, C)
    r0 = N.miss(y0, y, tol)
    assert N.same_bits(engine.debug_norm(x, op=op, form=0, **kw)["y"], f0["y"]), "the fp32 launch differs from its repetition"
    f1 = engine.debug_norm(x, op=op, form=1, **kw)
    y1, bad = N.apb_unpack(f1["apb"], M, C, pad_rows)
    assert bad == [], bad
    r1 = N.miss(y1, y, tol)
    assert torch.equal(engine.debug_norm(x, op=op, form=1, **kw)["apb"], f1["apb"]), "the APB launch differs from its repetition"
    f2 = engine.debug_norm(x, op=op, form=2, **kw)
    bad = N.amx_guards(f2["amx"], f2["scales"], M, C, pad_rows)
    assert bad == [], bad
    bad, far, off = N.amx_bracket(f2["amx"], f2["scales"], M, C, y, tol)
    again = engine.debug_norm(x, op=op, form=2, **kw)
    assert torch.equal(again["amx"], f2["amx"]) and torch.equal(again["scales"], f2["scales"]), "the AMX launch differs from its repetition"
    ndiff = int((_bits(y1) != _bits(y0)).sum())
    same = N.amx_same(f2["amx"], f2["scales"], y0, pad_rows)
    print(f"NORM {what}: max err / tol fp32 {r0:.3f}, APB {r1:.3f}; AMX outside its bracket by {far:.3g}, {100 * off:.2f} % of blocks on "
          f"the neighbour exponent; APB words != fp32 {ndiff}, AMX vs encode(fp32) {same or 'identical'}")
    assert r0 <= 1.0 and r1 <= 1.0
    assert bad == [], bad
    assert ndiff == 0, f"{ndiff} of {y0.numel()} decoded APB words differ from the fp32 rows"
    assert same == [], same
    return y0


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,mapped", LN_CASES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("C", N.LN_C)
def test_layernorm_three_forms(engine, C, M, mapped):
    x, w, b = N.rows(M, C)
    rm = None if mapped is None else G.window_map(*mapped)[0]
    y, tol = N.layernorm_ref(x, w, b, rm)
    check_forms(engine, f"layernorm C={C} M={M} map={mapped}", "layernorm", x, M, C, y, tol, w=w, b=b, row_map=rm)


@pytest.mark.parametrize("M,mapped", LN_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_layernorm_projection_width_fp32(engine, M, mapped):
    C = 576
    x, w, b = N.rows(M, C)
    rm = None if mapped is None else G.window_map(*mapped)[0]
    y, tol = N.layernorm_ref(x, w, b, rm)
    f0 = engine.debug_norm(x, op="layernorm", form=0, w=w, b=b, row_map=rm)
    r = N.miss(unpack_y(f0, M, C), y, tol)
    print(f"NORM layernorm C=576 M={M} map={mapped}: max err / tol fp32 {r:.3f}")
    assert r <= 1.0
    assert N.same_bits(engine.debug_norm(x, op="layernorm", form=0, w=w, b=b, row_map=rm)["y"], f0["y"])


@pytest.mark.parametrize("n,R_,Cin", N.MERGE_CASES)
def test_merge_layernorm(engine, n, R_, Cin):
    x, w, b = N.merge_tokens(n, R_, Cin)
    M = n * (R_ // 2) ** 2
    y, tol = N.merge_layernorm_ref(x, n, R_, w, b)
    f0 = engine.debug_norm(x, op="merge", form=0, w=w, b=b, n=n, R=R_)
    r = N.miss(unpack_y(f0, M, 4 * Cin), y, tol)
    swapped = N.miss(f0["y"][:M], *N.merge_layernorm_ref(x, n, R_, w, b, mutant="swap12")[:1], tol)
    print(f"NORM merge n={n} R={R_} Cin={Cin}: max err / tol fp32 {r:.3f} (against segments 1 and 2 swapped: {swapped:.3g})")
    assert r <= 1.0
    assert N.same_bits(engine.debug_norm(x, op="merge", form=0, w=w, b=b, n=n, R=R_)["y"], f0["y"])


# ---- RMSNorm ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", N.RMS_M)
@pytest.mark.parametrize("C", N.RMS_C)
def test_rmsnorm_three_forms(engine, C, M):
    x, w, _ = N.rows(M, C)
    y, tol = N.rmsnorm_ref(x, w, 1e-5)
    check_forms(engine, f"rmsnorm C={C} M={M}", "rmsnorm", x, M, C, y, tol, w=w, eps=1e-5)


@pytest.mark.parametrize("C", N.RMS_C)
def test_rmsnorm_eps_zero(engine, C):
    M = 33
    x, w, _ = N.rows(M, C, zero_row=False)
    y, tol = N.rmsnorm_ref(x, w, 0.0)
    check_forms(engine, f"rmsnorm C={C} M={M} eps=0", "rmsnorm", x, M, C, y, tol, w=w, eps=0.0)


# ---- no norm: the two stand-alone producers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", N.PLAIN_CASES + N.PLAIN_AMX_ONLY)
def test_split_rows_apb_and_quant_mx8_are_exact(engine, M, C):
    x = N.plain_rows(M, C)
    if C % 16 == 0:
        f1 = engine.debug_norm(x, op="none", form=1)
        got, bad = N.apb_unpack(f1["apb"], M, C, "zero")
        assert bad == [], bad
        nd = int((_bits(got) != _bits(x)).sum())
        assert nd == 0, f"{nd} of {x.numel()} decoded APB words differ from the input"
        assert torch.equal(engine.debug_norm(x, op="none", form=1)["apb"], f1["apb"])
    f2 = engine.debug_norm(x, op="none", form=2)
    bad = N.amx_guards(f2["amx"], f2["scales"], M, C, "zero")
    same = N.amx_same(f2["amx"], f2["scales"], x, "zero")
    bad2, far, off = N.amx_bracket(f2["amx"], f2["scales"], M, C, x.double(), torch.zeros(M, C, dtype=torch.float64))
    print(f"NORM none M={M} C={C}: APB decoded == input; AMX vs encode(input) {same or 'identical'}, outside the exact bracket by {far:.3g}")
    assert bad == [], bad
    assert same == [], same
    assert bad2 == [] and off == 0, bad2
    again = engine.debug_norm(x, op="none", form=2)
    assert torch.equal(again["amx"], f2["amx"]) and torch.equal(again["scales"], f2["scales"])


# ---- B: a prefix of the rows gives the same rows ----------------------------------------------------------------------------------------------
def _images(engine, op, x, **kw):
    M, C = x.shape
    pad = "zero" if op == "none" else "ff"
    out = {}
    if op != "none":
        out["y"] = engine.debug_norm(x, op=op, form=0, **kw)["y"][:M]
    out["apb"] = N.apb_unpack(engine.debug_norm(x, op=op, form=1, **kw)["apb"], M, C, pad)[0]
    f2 = engine.debug_norm(x, op=op, form=2, **kw)
    _, out["E"], out["bytes"], _, _ = N.amx_decode(f2["amx"], f2["scales"], M, C)
    return out


@pytest.mark.parametrize("op,C,sizes", [("layernorm", 96, (33, 129, 200)), ("layernorm", 768, (33, 129, 200)), ("rmsnorm", 576, (33, 129, 389)),
                                        ("none", 224, (70, 129, 200))])
def test_rows_of_a_shorter_launch_are_the_rows_of_a_longer_one(engine, op, C, sizes):
    big = sizes[-1]
    x, w, b = N.rows(big, C)
    kw = {"layernorm": dict(w=w, b=b), "rmsnorm": dict(w=w, eps=1e-5), "none": {}}[op]
    whole = _images(engine, op, x, **kw)
    for M1 in sizes[:-1]:
        part = _images(engine, op, x[:M1], **kw)
        for k, v in part.items():
            raw = (lambda t: t) if v.dtype == torch.uint8 else _bits
            assert torch.equal(raw(v), raw(whole[k][:M1])), (op, C, M1, k)


# ---- D: refusals by name, nothing launched ----------------------------------------------------------------------------------------------------
def test_refusals_by_name(engine):
    x96, w96, b96 = N.rows(33, 96)
    ok = dict(op="layernorm", form=0, w=w96, b=b96)

    def refused(match, x=x96, **kw):
        with pytest.raises(E.EngineError, match=match):
            engine.debug_norm(x, **{**ok, **kw})

    z = lambda M, C: torch.zeros(M, C)          # noqa: E731
    refused("multiple of 4", x=z(4, 98), w=torch.ones(98), b=torch.ones(98))
    refused(r"1536 \(LN_MAXV\)", x=z(4, 1540), w=torch.ones(1540), b=torch.ones(1540))
    refused(r"1536 \(LN_MAXV\)", x=z(4, 1540), op="rmsnorm", w=torch.ones(1540), b=None)
    refused(r"1536 \(LN_MAXV\)", x=torch.zeros(1, 4, 388), op="merge", n=1, R=2, w=torch.ones(1552), b=torch.ones(1552))
    for form in (1, 2):
        refused("C % 16 == 0 and C <= 768", x=z(4, 104), form=form, w=torch.ones(104), b=torch.ones(104))
        refused("C <= 768", x=z(4, 784), form=form, w=torch.ones(784), b=torch.ones(784))
        refused("C <= 768", x=z(4, 784), op="rmsnorm", form=form, w=torch.ones(784), b=None)
        refused("C % 16 == 0", x=z(4, 104), op="rmsnorm", form=form, w=torch.ones(104), b=None)
        refused(r"96 KiB of LDS .*C <= 752", x=z(4, 768), op="rmsnorm", form=form, w=torch.ones(768), b=None)
        refused("fp32 form only", x=torch.zeros(1, 4, 96), op="merge", form=form, n=1, R=2, w=torch.ones(384), b=torch.ones(384))
    refused("multiple of 16 for launch_split_rows_apb", x=z(4, 100), op="none", form=1, w=None, b=None)
    refused("form 0 would launch nothing", op="none", w=None, b=None)
    refused("even R", x=torch.zeros(1, 9, 96), op="merge", n=1, R=3, w=torch.ones(384), b=torch.ones(384))
    refused("w is null", w=None)
    refused("b is null", b=None)
    refused("w is null", op="rmsnorm", w=None, b=None)
    refused("not a permutation", row_map=torch.tensor([0, 1, 1], dtype=torch.int32))
    refused("not a permutation", row_map=torch.tensor([0, 1, 3], dtype=torch.int32))
    refused("M % ntok == 0", row_map=torch.tensor([1, 0], dtype=torch.int32))
    refused("row_map goes with op 0", op="rmsnorm", b=None, row_map=torch.tensor([1, 2, 0], dtype=torch.int32))
    refused("finite and >= 0", op="rmsnorm", b=None, eps=-1.0)
    refused("form must be", form=3)
    # M < 1 and M above the taps' 2^22, and capacities: through the C entry point itself (nothing is read before the refusal)
    fn, p = engine.lib.mellow_debug_norm, lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    buf = torch.empty(64 * 96, dtype=torch.float32)

    def raw(match, M, C=96, op=0, form=0, cap=buf.numel() * 4, sc_cap=0, n=0, R_=0):
        assert fn(engine.h, op, form, p(x96), M, C, p(w96), p(b96), 1e-5, None, 0, n, R_, p(buf), cap, p(buf) if sc_cap else None, sc_cap) != 0
        assert match in engine.lib.mellow_last_error().decode(), engine.lib.mellow_last_error().decode()

    raw("1 <= M <=", 0)
    raw("1 <= M <=", -5)
    raw("1 <= M <=", (1 << 22) + 1, C=4)
    raw("is not n * (R / 2)^2", 5, op=1, n=1, R_=4)
    raw("out_capacity", 33, cap=(33 + 32) * 96 * 4 - 1)
    raw("out_capacity", 33, form=1, cap=128 * 96 * 6 - 1)
    raw("out_capacity", 33, form=2, cap=128 * 128 - 1, sc_cap=128 * 8)
    raw("scales_capacity", 33, form=2, cap=128 * 128, sc_cap=128 * 8 - 1)
    raw("scales_capacity", 33, form=2, cap=128 * 128, sc_cap=0)
    # the engine still runs a launch after all those refusals
    y, tol = N.layernorm_ref(x96, w96, b96)
    assert N.miss(unpack_y(engine.debug_norm(x96, **ok), 33, 96), y, tol) <= 1.0
