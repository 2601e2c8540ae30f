"""CPU: the yardsticks of tests/test_gpu_dec_gemv.py (tests/dec_gemv_ref.py) checked without a GPU -- the float32 evaluation of the
reference, laid out as the tap lays its outputs out, passes the check the GPU test applies (tolerances, bit statements, guards) on
every case; the codecs round-trip and address every element exactly once; the case list reaches the paths it was chosen for; and
every mutant of the reference the GPU test is meant to catch exceeds the tolerance on every case it applies to (err / tol is
printed; > 1 is the condition, no figure is fixed in advance)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dec_attn_ref as A  # noqa: E402
import dec_gemv_ref as R  # noqa: E402


def test_case_list_covers_what_it_is_derived_for():
    def rbm(rb):
        return rb if rb in (1, 2) else 4
    fp32 = [c for c in R.CASES if c.form == 0 and c.blk is None]
    x3 = [c for c in R.CASES if c.form == 1 and c.blk is None]
    for op in range(5):
        assert {c.B for c in fp32 if c.op == op} >= {1, 32, 33, 70}
    # dec_qkv2: 4 waves at one row block, 12 otherwise
    assert {c.RB == 1 for c in fp32 if c.op == 3} == {True, False}
    for op in (1, 3):
        cs = [c for c in x3 if c.op == op]
        assert {c.B for c in cs} == {20, 33, 70, 130}
        assert [(rbm(c.RB), c.RB % rbm(c.RB), c.RB > rbm(c.RB)) for c in sorted(cs, key=lambda c: c.B)] == \
            [(1, 0, False), (2, 0, False), (4, 3, False), (4, 1, True)]      # RBM 1; RBM 2; RBM 4, a partial pass; RBM 4, a second pass of one block
    # op 0: both instantiations of KCD and FIRST, inc_pos on and off; op 4: both KCD, both outputs
    assert {(c.kcd, c.first, c.inc_pos) for c in fp32 if c.op == 0} == {(0, 1, 1), (0, 1, 0), (R.KC_DOWN, 0, 0)}
    assert {(c.kcd, c.want_x3) for c in fp32 if c.op == 4} == {(0, 0), (0, 1), (R.KC_DOWN, 0), (R.KC_DOWN, 1)}
    assert any(c.eps == R.BIG_EPS for c in fp32 if c.op == 1) and any(c.eps == R.BIG_EPS for c in fp32 if c.op == 4) and any(c.eps == R.BIG_EPS for c in x3)
    blk = [c for c in R.CASES if c.blk is not None]
    assert {(c.op, c.form, c.blk) for c in blk} == {(op, f, b) for op, f in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (1, 1), (3, 1))
                                                    for b in ((1, 0, 1), (1, 1, 1, 1, 0))}


def test_inputs_make_the_faults_visible():
    w = R.weights()
    for B in (1, 33, 130):
        inp = R.inputs(B)
        rms = inp["x"][:B].pow(2).mean(1).sqrt()
        assert float(rms.min()) > 1.8 and float(rms.max()) < 4.2                      # well away from 1
        assert 2.0 < float(inp["down"][:, :B].pow(2).mean().sqrt()) < 4.0             # slabs of the size of x_mid (its row rms: 2 .. 4)
        assert bool(torch.isnan(inp["ssq"][:, 36:]).all()) and bool((inp["x"][B:] == 0).all())
    for name in ("Wq", "Wg", "Wu", "Wd"):
        W = w[name]
        assert float(W.abs().mean(1).max() / W.abs().mean(1).min()) > 1.5 and float(W.abs().mean(0).max() / W.abs().mean(0).min()) > 1.5
    cos, sin = w["rope"]
    assert len({tuple(r.tolist()) for r in cos}) == R.TMAX and float((w["wn"] - 1).abs().mean()) > 0.2


@pytest.mark.parametrize("cid", R.CASE_IDS)
def test_float32_evaluation_passes_the_check(cid):
    c = R.case(cid)
    res = R.check(c, R.emulate(c))
    print(f"DECGEMV ref32 {cid}: " + ", ".join(f"{k} {v:.3g}" for k, v in res.items()))
    assert R.worst(res) <= 1.0, res


def test_codecs_round_trip():
    g = torch.Generator().manual_seed(3)
    for rows in (32, 96):
        x, h = torch.randn(rows, R.HID, generator=g), torch.randn(rows, R.INTER, generator=g)
        assert np.array_equal(R.f32_index(rows), A.f32_index(rows)) and np.array_equal(R.f3_32_index(rows), A.f3_32_index(rows))
        for t, K in ((x, R.HID), (h, R.INTER)):
            idx, idx3 = R.f32_index(rows, K), R.f3_32_index(rows, K)
            assert np.array_equal(np.sort(idx.reshape(-1)), np.arange(rows * K))            # every element has exactly one owner
            assert np.array_equal(np.sort(idx3.reshape(-1)), np.arange(rows * K * 3))
            assert torch.equal(R.decode(R.encode(t, idx), idx), t)
            assert torch.equal(R.f3_decode(R.f3_encode(t, idx3), idx3).view(torch.int32), t.view(torch.int32))      # the triple is exact
        assert torch.equal(R.f3_decode(R.f3_encode(x, A.f3_16_index(rows)), A.f3_16_index(rows)), x)
        assert torch.equal(A.f16_decode(A.f16_encode(x[None]), rows)[0], x)
    # spot values worked by hand from the layout comments: row 37 (block 1, m = 5), column 1000 of h
    assert R.f32_index(64, R.INTER)[37, 1000] == (((1 * 192 + 125) * 64 + 5 + 32 * 0) * 4 + 0)
    assert R.f3_32_index(64, R.INTER)[2, 37, 1000] == ((((1 * 96 + 62) * 3 + 2) * 64 + 5 + 32 * 1) * 8 + 0)


MUTANTS = {
    "swap": "1a. two slabs' k-ranges exchanged",
    "ktile": "1b. one k-tile dropped",
    "slab_out": "2. one down slab left out of x_new",
    "swap_gate_up": "3. gate and up exchanged",
    "r2_one_factor": "4. r2 missing on one factor",
    "r2_after_silu": "5. r2 applied after the silu only",
    "no_eps": "6. eps omitted",
    "rope_row": "7. RoPE row pos instead of pos + inc_pos",
    "q_other": "8. Q with Wd of another layer",
    "side_q": "9. the side tiles fed Q's rows",
    "no_weight": "10. the final norm without its weight",
    "dead_rows": "11. a dead block's rows written",
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_exceeds_the_tolerance_on_every_case_it_applies_to(mutant):
    claimed = 0
    for cid in R.CASE_IDS:
        c = R.case(cid)
        out = R.emulate(c, mutant)
        if out is None:
            continue
        claimed += 1
        res = R.check(c, out)
        bad = {k: v for k, v in res.items() if not v <= 1.0}
        print(f"DECGEMV mutant '{MUTANTS[mutant]}' {cid}: " + ", ".join(f"{k} {v:.3g}" for k, v in bad.items()))
        assert bad, (mutant, cid, res)
    assert claimed >= 3, (mutant, claimed)
