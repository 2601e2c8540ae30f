"""CPU: the yardsticks of tests/test_gpu_dec_tail.py (tests/dec_tail_ref.py) checked without a GPU -- the float32 evaluation of every
reference, laid out as the tap lays its outputs out, passes the check the GPU test applies (tolerances, exact statements, guards) on
every case; the case list reaches the paths it was chosen for; the inputs make the faults visible (planted rows, the arg-max gap on
EVERY plain row); and every mutant of the reference the GPU test is meant to catch exceeds the tolerance on every case it applies to,
except the one that documents a benign guard, which must pass (err / tol is printed; > 1 is the condition, no figure is fixed in
advance)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dec_tail_ref as R  # noqa: E402

HEAD = [c for c in R.CASES if c.kind == "head"]


@pytest.fixture(scope="module")
def emulated():
    """the float32 evaluation of every case, formed once"""
    return {c.id: R.emulate(c) for c in R.CASES}


def test_case_list_covers_what_it_is_derived_for():
    plain = [c for c in HEAD if c.blk is None]
    assert {c.B for c in plain if c.form == 0} >= {1, 32, 33, 70}
    assert {c.V for c in plain if c.form == 0} == {96, 256, 768, 8448} and {c.V for c in plain if c.form == 1} == {256, 768, 8448}
    x3 = sorted({c.B for c in plain if c.form == 1})
    assert x3 == [1, 20, 33, 70, 128, 130]
    # G 1; G 1; G 2; G 4 with gn = 3; G 4 full; G 4 and a second pass of one block
    assert [(R.head_G((B + 31) // 32), ((B + 31) // 32) % R.head_G((B + 31) // 32), (B + 31) // 32 > 4) for B in x3] == \
        [(1, 0, False), (1, 0, False), (2, 0, False), (4, 3, False), (4, 0, False), (4, 1, True)]
    for form in (0, 1):
        assert {(c.want_logits, c.want_sum) for c in plain if c.form == form and c.B == 70} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert {(c.blk, c.want_sum) for c in HEAD if c.form == form and c.blk} == {(b, s) for b in ((1, 0, 1), (1, 1, 1, 1, 0)) for s in (0, 1)}
    assert all(c.V % 256 == 0 for c in HEAD if c.form == 1)                      # what dec_head3r_fits asks: whole workgroups of 8 tiles
    assert max(c.B * c.V for c in HEAD) == 130 * 8448 and 8448 // 32 > 256       # the stride loops of the arg-max run a second round
    am = [c for c in R.CASES if c.kind == "argmax"]
    assert {c.B for c in am} == {3, 33, 70} and {c.n for c in am} == {8, 264}
    st = [R.planted(c.id)["state"] for c in am]
    assert {s["pos"] - s["T0"] + 1 for s in st if s} >= {-1, 0, R.MAX_LEN - 1, R.MAX_LEN} and any(s is None for s in st)
    assert {(R.planted(c.id)["write_x"], R.planted(c.id)["with_logprob"]) for c in am} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(R.planted(c.id)["ros"] is not None and int((R.planted(c.id)["ros"] < 0).sum()) for c in am)
    packs = {c.name: R.pack_model(c, R.planted(c.id)) for c in R.CASES if c.kind == "pack"}
    assert [packs[n]["moved"] for n in R.PACK_NAMES] == [True, True, False, True, True, False, True]
    assert packs["B64-nact0"]["n_act"] == 0 and packs["B64-33-none"]["n_act"] == 33 and packs["B1024-40-scattered"]["n_act"] == 40
    # slots 1 .. 40 packed: every destination is one below its source
    assert all(torch.equal(packs["B96-slots1to40"]["x_rows"][d], R.planted("pack-B96-slots1to40")["x"][d + 1]) for d in range(40))
    ids = R.planted("load-B33-ids-clamped")
    assert int(ids["ids"].min()) == -3 and int(ids["ids"].max()) == ids["n_src"] + 5


def test_head_inputs_make_the_faults_visible():
    for V, B in sorted({(c.V, c.B) for c in HEAD}):
        inp, W = R.head_inputs(V, B), R.head_weight(V)
        plant = R.planted_rows(B)
        plain = [r for r in range(B) if r not in plant]
        rms = inp["x"][plain].pow(2).mean(1).sqrt()
        assert 0.2 < float(rms.min()) and float(rms.max()) < 4.5 and bool((inp["x"][B:] == 0).all())
        cols = R.tie_cols(V)
        assert all(torch.equal(W[cols[0]], W[k]) for k in cols) and cols == sorted(cols) and cols[-1] < V
        assert cols[1] - cols[0] == 3 and cols[0] % 8 < 4 <= cols[1] % 8 and cols[3] - cols[2] == 8      # the two h halves; 8 q apart
        if V >= 768:
            assert cols[4] // 256 != cols[0] // 256
        if V >= 8448:
            assert cols[5] // 32 - cols[0] // 32 > 256
        # no row is left out of the gap rule: every row that is neither a tie nor NaN (nor all zeros) is separated by > 2 tol
        ref, tol = inp["ref"], inp["tol"]
        checked = 0
        for r in range(B):
            if plant.get(r) in ("tie", "nan", "zero"):
                continue
            top = torch.topk(ref[r], 2)
            assert float(top.values[0] - top.values[1]) > 2 * float(tol[r][top.indices].max()), (V, B, r)
            checked += 1
        assert checked == B - sum(1 for w in plant.values() if w in ("tie", "nan", "zero"))
        for r, what in plant.items():
            if what == "tie":
                top = torch.topk(ref[r], len(cols) + 1)
                assert sorted(top.indices[:len(cols)].tolist()) == cols and float(top.values[len(cols) - 1] - top.values[len(cols)]) > 2 * float(tol[r].max())
            if what == "peaked":
                assert int(ref[r].argmax()) == R.PEAK_COL
    assert float(W.abs().mean(1).max() / W.abs().mean(1).min()) > 1.5 and float(W.abs().mean(0).max() / W.abs().mean(0).min()) > 1.5


@pytest.mark.parametrize("cid", R.CASE_IDS)
def test_float32_evaluation_passes_the_check(emulated, cid):
    c = R.case(cid)
    twin = emulated[c.twin().id] if c.kind == "head" and not c.want_logits else None
    res = R.check(c, emulated[cid], twin)
    print(f"DECTAIL ref32 {cid}: " + ", ".join(f"{k} {v:.3g}" for k, v in res.items()))
    assert R.worst(res) <= 1.0, res


def test_duplicated_weight_rows_give_equal_bits_in_the_emulation():
    for V, B in ((96, 33), (8448, 33)):
        l32 = R.head_logits32(V, B)
        cols = R.tie_cols(V)
        assert all(torch.equal(l32[:, cols[0]].view(torch.int32), l32[:, k].view(torch.int32)) for k in cols)


@pytest.mark.parametrize("mutant", list(R.MUTANTS))
def test_mutant_exceeds_the_tolerance_on_every_case_it_applies_to(emulated, mutant):
    claimed, ratios = 0, []
    for cid in R.CASE_IDS:
        c = R.case(cid)
        out = R.emulate(c, mutant)
        if out is None:
            continue
        claimed += 1
        twin = emulated[c.twin().id] if c.kind == "head" and not c.want_logits else None
        res = R.check(c, out, twin)
        bad = {k: v for k, v in res.items() if not v <= 1.0}
        print(f"DECTAIL mutant '{R.MUTANTS[mutant]}' {cid}: " + (", ".join(f"{k} {v:.3g}" for k, v in bad.items()) or f"passes, worst {R.worst(res):.3g}"))
        if mutant in R.BENIGN:
            assert not bad, (mutant, cid, bad)
        else:
            assert bad, (mutant, cid, res)
            ratios.append(max(v if v == v else float("inf") for v in bad.values()))
    assert claimed >= 1, mutant
    if ratios:
        print(f"DECTAIL mutant '{R.MUTANTS[mutant]}': {claimed} cases, err / tol {min(ratios):.3g} ... {max(ratios):.3g}")
