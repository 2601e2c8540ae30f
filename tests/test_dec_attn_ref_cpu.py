"""CPU: the yardsticks of tests/test_gpu_dec_attn.py (tests/dec_attn_ref.py) checked without a GPU -- the float32 evaluation of the
reference stays inside the tolerance it sets, the layout codecs round-trip and address every element exactly once, the merge of
exactly split partials is the direct softmax, and every mutant of the reference the GPU test is meant to catch exceeds the
tolerance on every case it is claimed for (err / tol is printed; > 1 is the condition, no figure is fixed in advance)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dec_attn_ref as R  # noqa: E402

OUTPUTS = ("att", "k", "v", "x_mid", "ssq")


def _fused_of(cid):
    """both producers over the case list: the fused one on every other case"""
    return bool(R.CASE_IDS.index(cid) % 2)


def test_case_list_covers_what_it_is_derived_for():
    for c in R.CASES:
        print(c)
    by = {g: [c for c in R.CASES if c.group == g] for g in "abcdef"}
    V, M = R.chunk_groups(False), R.chunk_groups(True)
    assert (V, M) == (56, 64)
    assert sorted(c.pos for c in by["a"]) == [1, 2, 3, 4, 5] and all(c.gs == 1 and c.ts == 2 for c in by["a"])
    assert {c.pos for c in by["b"] if c.ctx_end == 449} == {223, 224, 225} and all(c.gs == V and not c.kv16 for c in by["b"])
    pulled = [c for c in by["b"] if c.ctx_end != 449]
    assert len(pulled) == 1 and ((pulled[0].ctx_end + 2) // 4 + 1) // 2 > V and R.chunks_of(pulled[0].pos, V, 2, False) == 2
    assert all(c.gs >= 2 * V and R.chunks_of(c.pos, c.gs, 2, False) >= 2 for c in by["c"])
    assert any(c.ts == 1 and c.RB == 2 for c in by["d"]) and any(c.ts == 2 and c.RB == 2 and not c.kv16 for c in by["d"])
    assert {31, 32, 33, 255, 256, 257, 511, 512, 513} <= {c.pos for c in by["e"]} and all(c.kv16 for c in by["e"])
    assert any(c.RB == 2 for c in by["e"])
    assert all(c.pos == c.Tmax - 1 for c in by["f"]) and any(c.Tmax % 4 for c in by["f"]) and {c.kv16 for c in by["f"]} == {False, True}
    assert {c.B for c in R.CASES if c.RB == 1} == {1, 3, 32} and {c.B for c in R.CASES if c.RB == 2} == {33, 64}
    assert all(c.Tmax <= 1024 and 1 <= c.pos < c.ctx_end <= c.Tmax for c in R.CASES)
    # what the tap accepts as ts: 2 always, 1 from two row blocks on with fp32 pages
    assert all(c.ts == 2 or (c.ts == 1 and c.RB >= 2 and not c.kv16) for c in R.CASES)
    assert max(R.chunks_of(c.pos, c.gs, c.ts, c.kv16) for c in R.CASES) == 3       # c = 8 * (n + 2) was derived for n <= 3


def test_split_rule():
    assert R.split_groups(8, 2, False) == 1 and R.split_groups(2, 2, False) == 1
    assert R.split_groups(449, 2, False) == 56 and R.split_groups(465, 2, False) == 56 and R.split_groups(485, 2, False) == 61
    assert R.split_groups(453, 1, False) == 112 and R.split_groups(520, 2, True) == 64 and R.split_groups(552, 2, True) == 69
    assert R.split_ranges(5, 1, 2) == [(0, 4), (4, 5)] and R.split_ranges(3, 1, 2) == [(0, 3), (3, 3)] and R.split_ranges(9, 5, 1) == [(0, 9)]


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("cid", R.CASE_IDS)
def test_float32_evaluation_stays_inside_the_tolerance(cid, fused):
    r = R.reference(cid, fused)
    inp = R.inputs(cid, fused)
    assert bool(torch.isnan(inp["K"][:, :, inp["pos"] + 1:]).all()) and bool(torch.isfinite(inp["V"]).all())
    for name in OUTPUTS:
        m = R.miss(r["ref32"][name], r["ref"][name], r["tol"][name])
        print(f"DECATTN ref32 {cid} fused {int(fused)} {name}: e_ref {r['e_ref'][name]:.3e}, tol {r['tol'][name]:.3e}, c {r['c']:.0f}")
        assert m <= 1.0 and bool(torch.isfinite(r["ref"][name]).all())


@pytest.mark.parametrize("rows", [32, 64])
def test_codecs_round_trip(rows):
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(2, rows, R.HID, generator=g)
    for enc, dec, index in ((R.f16_encode, R.f16_decode, R.f16_index), (R.f32_encode, R.f32_decode, R.f32_index)):
        assert np.array_equal(np.sort(index(rows).reshape(-1)), np.arange(rows * R.HID))       # every element has exactly one owner
        raw = enc(x)
        assert raw.shape == (2 * rows * R.HID,) and torch.equal(dec(raw, rows, 2), x)
    assert not np.array_equal(R.f16_index(rows), R.f32_index(rows))
    # spot values of the two formulas, worked by hand from the layout comments
    assert R.f16_index(64)[37, 70] == ((((1 * 36 + 4) * 2 + 0) * 64 + 5 + 16 * 1) * 4 + 2)
    assert R.f32_index(64)[37, 70] == (((1 * 72 + 8) * 64 + 5 + 32 * 1) * 4 + 2)
    for index in (R.f3_32_index, R.f3_16_index):
        assert np.array_equal(np.sort(index(rows).reshape(-1)), np.arange(rows * R.HID * 3))
        raw = R.f3_encode(x[0], index)
        assert raw.dtype == torch.int16 and raw.numel() == rows * R.HID * 3
        assert torch.equal(R.f3_decode(raw, rows, index).view(torch.int32), x[0].view(torch.int32))      # the triple is exact
    assert R.f3_32_index(64)[1, 37, 70] == ((((1 * 36 + 4) * 3 + 1) * 64 + 5 + 32 * 0) * 8 + 6)
    assert R.f3_16_index(64)[2, 37, 70] == (((((1 * 18 + 2) * 2 + 0) * 3 + 2) * 64 + 5 + 16 * 0) * 8 + 6)
    m, l = torch.randn(2, rows, 9, generator=g), torch.rand(2, rows, 9, generator=g)
    raw = R.ml_encode(m, l)
    assert raw.shape == (9, rows, 2, 2) and raw[4, 7, 1, 0] == m[1, 7, 4] and raw[4, 7, 1, 1] == l[1, 7, 4]
    m2, l2 = R.ml_decode(raw.reshape(-1), rows, 2)
    assert torch.equal(m2, m) and torch.equal(l2, l)
    assert torch.equal(R.bf16_bits(torch.tensor([1.0, 1.00390625, 1.01171875])), torch.tensor([0x3F80, 0x3F80, 0x3F82], dtype=torch.int16))


@pytest.mark.parametrize("cid", R.CASE_IDS)
def test_merge_of_exact_split_partials_is_the_direct_softmax(cid):
    c, fused = R.case(cid), _fused_of(cid)
    inp, r = R.inputs(cid, fused), R.reference(cid, fused)
    O, m, l = R.split_partials(inp, c.gs, c.ts)
    got = R.merge(O, m, l)
    err = float((got - r["ref"]["att"]).abs().max())
    print(f"DECATTN merge {cid}: max|err| {err:.3e} (float64)")
    assert err <= 1e-12 * max(1.0, float(r["ref"]["att"].abs().max()))
    # through the codecs as well: what the GPU test does with the raw outputs
    rows = c.rows
    Op = torch.zeros(c.ts, rows, R.HID)
    Op[:, :c.B] = O.float()
    mp, lp = torch.zeros(c.ts, rows, 9), torch.ones(c.ts, rows, 9)
    mp[:, :c.B], lp[:, :c.B] = m.float(), l.float()
    O2 = R.f16_decode(R.f16_encode(Op), rows, c.ts)
    m2, l2 = R.ml_decode(R.ml_encode(mp, lp), rows, c.ts)
    assert R.miss(R.merge(O2, m2, l2)[:c.B], r["ref"]["att"], r["tol"]["att"]) <= 1.0


def _mutants(c, inp):
    """name -> (claimed for this case, the mutant's outputs)"""
    pos, gs, ts, ch = c.pos, c.gs, c.ts, R.chunk_groups(c.kv16)
    ranges = R.split_ranges(pos, gs, ts)
    second = [lo + 4 * ch for lo, hi in ranges if lo + 4 * ch < hi]           # first key of a second chunk, any split
    out = {
        "key pos - 1 dropped": (True, lambda: R.dec_attn_ref(inp, drop=(pos - 1,))),
        "key pos + 1 included": (pos + 1 < c.Tmax, lambda: R.dec_attn_ref(inp, include_next=True)),
        "the new key dropped": (True, lambda: R.dec_attn_ref(inp, drop_new=True)),
        "first key of split 1 dropped": (ts == 2 and 4 * gs < pos, lambda: R.dec_attn_ref(inp, drop=(4 * gs,))),
        "first key of a second chunk dropped": (bool(second), lambda: R.dec_attn_ref(inp, drop=(second[0],))),
        "head map h % 3": (True, lambda: R.dec_attn_ref(inp, kv_of=[h % 3 for h in range(9)])),
        "RoPE sign flipped": (True, lambda: R.dec_attn_ref(inp, rope_sign=-1.0)),
        "1 / 8 scale missing": (True, lambda: R.dec_attn_ref(inp, scale=1.0)),
        "rscale of the wrong row": (c.B >= 2, lambda: R.dec_attn_ref(inp, rscale_shift=1)),
        "residual row of another slot": (c.B >= 2, lambda: R.dec_attn_ref(inp, resid_shift=1)),
    }

    def swapped():
        O, m, l = R.split_partials(inp, gs, ts)
        att = R.merge(O, m, l, swap_m=True)
        return {"att": att, **R.oproj_ref(att, R.projected(inp)["x_new"], inp["Wo"])}
    out["m of two splits swapped in the merge"] = (ts == 2, swapped)
    return out


MUTANTS = ["key pos - 1 dropped", "key pos + 1 included", "the new key dropped", "first key of split 1 dropped",
           "first key of a second chunk dropped", "head map h % 3", "RoPE sign flipped", "1 / 8 scale missing", "rscale of the wrong row",
           "m of two splits swapped in the merge", "residual row of another slot"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutant_exceeds_the_tolerance_on_every_case_it_is_claimed_for(mutant):
    claimed = 0
    for cid in R.CASE_IDS:
        c, fused = R.case(cid), _fused_of(cid)
        inp, r = R.inputs(cid, fused), R.reference(cid, fused)
        ok, run = _mutants(c, inp)[mutant]
        if not ok:
            continue
        claimed += 1
        got = run()
        worst = max(R.miss(torch.nan_to_num(got[name], nan=float("inf")), r["ref"][name], r["tol"][name]) for name in OUTPUTS if name in got)
        print(f"DECATTN mutant '{mutant}' {cid} fused {int(fused)}: err / tol {worst:.3g}")
        assert worst > 1.0, (mutant, cid, worst)
    assert claimed >= 4, (mutant, claimed)
