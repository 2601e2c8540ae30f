"""GPU (-m gpu): the launches that end a decode step -- the lm_head in its fp32 and its streaming f32x3 form, the arg-max with the
step epilogue, the row repack and the row load -- ONE launch each on data this module chose, through the tap mellow_debug_dec_tail
(include/mellow_hip.h) of an engine without weights.

Yardsticks (tests/dec_tail_ref.py; tests/test_dec_tail_ref_cpu.py checks them and shows which mutants they catch):
  * the logits against the float64 product within the per-element tolerance of gemm_ref's rule (the reference sets it, never the
    kernel); cand_val / cand_idx bit for bit the arg_better winner of the logits the same launch stored; cand_sum against the float64
    sum over the stored logits; a launch without logits equal to its twin with them; the row arg-max against float64 where the gap
    allows it, and against the planted ties, zero and NaN rows;
  * an integer model of the step epilogue and of the repack: every token, record, counter, word and moved or gathered row exact, the
    log-prob within the tolerance of its chain;
  * guards: every output holds 0xFF bytes before the launch, so every word no live slot owns must still hold them;
  * bit identities that hold by construction on ONE kernel instantiation: a launch == its repetition, a row of a batch == the row
    alone at the same RB, the same 32 rows in block 0 and in block 2 (the fp32 head, whose grid indexes the block).  Across
    instantiations (G 1 / 2 / 4, BLK, LSE, fp32 against f32x3) each side is held to float64 above; whether they are bit-equal is
    printed, not asserted.
Every case prints err / tol (DESIGN.md 6za holds the figures)."""
import os
import sys

import numpy as np
import pytest
import torch

from mellow_amd import engine as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dec_tail_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = E.Engine(device=0)          # no weights: the tap works on an engine that is not finalised
    yield e
    e.close()


def _same(a, b):
    if not torch.is_tensor(a):
        return a == b
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _head(engine, c, x=None):
    return engine.debug_dec_tail(**R.head_args(c, x))


@pytest.mark.parametrize("cid", R.CASE_IDS)
def test_launch_against_the_reference_and_guards(engine, cid):
    c = R.case(cid)
    out = engine.debug_dec_tail(**R.tap_args(c))
    twin = _head(engine, c.twin()) if c.kind == "head" and not c.want_logits else None
    res = R.check(c, out, twin)
    print(f"DECTAIL {cid}: " + ", ".join(f"{k} {v:.3g}" for k, v in res.items()))
    assert R.worst(res) <= 1.0, {k: v for k, v in res.items() if not v <= 1.0}


REPEATED = ("head-f0-V768-B70-l1s1", "head-f1-V768-B70-l1s1", "argmax-B70-n264-blk-slots-lp-x", "pack-B96-101-holes", "load-B33-ids-clamped")


@pytest.mark.parametrize("cid", REPEATED)
def test_a_launch_equals_its_repetition(engine, cid):
    c = R.case(cid)
    a, b = engine.debug_dec_tail(**R.tap_args(c)), engine.debug_dec_tail(**R.tap_args(c))
    assert a.keys() == b.keys()
    for name in a:
        assert _same(a[name], b[name]), name


@pytest.mark.parametrize("form", (0, 1))
def test_a_row_of_a_batch_equals_the_row_alone_at_the_same_RB(engine, form):
    c, row = R.case(f"head-f{form}-V768-B70-l1s1"), 40
    x = R.head_inputs(768, 70)["x"]
    alone_x = torch.zeros_like(x)
    alone_x[row] = x[row]
    full, alone = _head(engine, c), _head(engine, c, alone_x)
    for name in full:
        assert _same(full[name][row], alone[name][row]), name
        assert not _same(full[name][row - 1], alone[name][row - 1]), name      # (the other rows did change)


def test_the_same_rows_in_block_0_and_in_block_2_give_the_same_bits(engine):
    c = R.Case("head", 96, 0, 768, 1, 1)       # the fp32 kernel: the grid indexes the row block, every block runs the same code
    x = torch.zeros(96, 576)
    x[:70] = R.head_inputs(768, 70)["x"][:70]
    x[64:96] = x[0:32]
    out = _head(engine, c, x)
    for name in out:
        assert _same(out[name][0:32], out[name][64:96]), name
        assert not _same(out[name][0:32], out[name][32:64]), name


def test_instantiations_against_each_other_are_reported(engine):
    """G 1 / 2 / 4, BLK on / off, LSE on / off and the two forms are different instantiations: nothing in the code or in DESIGN.md
    promises equal bits between them, so each side is held to float64 (test_launch_against_the_reference_and_guards) and this only
    reports"""
    x130 = R.head_inputs(768, 130)["x"]
    got = {}
    for B in (20, 33, 70, 130):
        x = torch.zeros((B + 31) // 32 * 32, 576)
        x[:B] = x130[:B]
        got[B] = _head(engine, R.Case("head", B, 1, 768, 1, 1), x)
    for B in (33, 70, 130):
        eq = all(_same(got[20][n][:20], got[B][n][:20]) for n in got[20])
        print(f"DECTAIL bits f1: rows 0 .. 19 at G 1 and at G {R.head_G((B + 31) // 32)} (B {B}): {eq}")
    for form in (0, 1):
        base = _head(engine, R.case(f"head-f{form}-V768-B70-l1s1"))
        cb = R.case(f"head-f{form}-V768-B70-l1s1-blk101")
        blk = _head(engine, cb)
        live = torch.cat([cb.live_rows, torch.zeros(32, dtype=torch.bool)])
        print(f"DECTAIL bits f{form}: BLK on == BLK off on the live rows: {all(_same(base[n][live], blk[n][live]) for n in base)}")
        nolse = _head(engine, R.case(f"head-f{form}-V768-B70-l1s0"))
        print(f"DECTAIL bits f{form}: LSE on == LSE off logits: {_same(base['logits'], nolse['logits'])}, partials: "
              f"{_same(base['cand_val'], nolse['cand_val']) and _same(base['cand_idx'], nolse['cand_idx'])}")
    f0, f1 = (_head(engine, R.case(f"head-f{form}-V768-B70-l1s1")) for form in (0, 1))
    d = (f0["logits"][:70].double() - f1["logits"][:70].double()).abs()
    ok = R.head_inputs(768, 70)["tol"][:70] > 0           # (not the NaN row, not the zero row)
    print(f"DECTAIL bits: form 0 == form 1 logits: {_same(f0['logits'], f1['logits'])}; largest difference {float(d[ok].max()):.3g} "
          f"({float((d / R.head_inputs(768, 70)['tol'][:70])[ok].max()):.3g} of the tolerance), cand_idx equal: {_same(f0['cand_idx'], f1['cand_idx'])}")


@pytest.mark.parametrize("form", (0, 1))
def test_the_arg_max_of_a_head_launch_is_the_arg_max_of_its_logits(engine, form):
    """op 1 on the partials an op 0 launch returned: the token is the arg_better arg-max of that launch's logits, and -log S agrees
    with the float64 log-sum-exp of those logits within the two tolerances added (cand_sum's and the merge's)"""
    c = R.case(f"head-f{form}-V8448-B33-l1s1")
    B, n = c.B, c.n
    head = _head(engine, c)
    logits = head["logits"][:B]
    state = {"max_len": 2, "stop_id": 0, "T0": 5, "pos": 4, "n_seen": 0, "arrive": 0, "ticket": 0}
    out = engine.debug_dec_tail(op=1, B=B, V=c.V, cand_val=head["cand_val"][:B], cand_idx=head["cand_idx"][:B], cand_sum=head["cand_sum"][:B],
                                state=state, with_logprob=True, seen_stop=torch.zeros(c.rows, dtype=torch.int32))
    L = logits.numpy()
    want = np.where(np.isnan(L).any(1), np.isnan(L).argmax(1), np.where(np.isnan(L), -np.inf, L).argmax(1))       # numpy: the first occurrence
    assert np.array_equal(out["tokens"][:B].numpy(), want.astype(np.int32))
    assert torch.equal(out["record"][:B, 0], out["tokens"][:B]) and bool((out["record"][:, 1] == -1).all())
    plain = [r for r in range(B) if R.planted_rows(B).get(r) != "nan"]
    l64 = logits[plain].double()
    M = l64.amax(1, keepdim=True)
    ref = -torch.log(torch.exp(l64 - M).sum(1))
    _, dmax = R.tile_sum64(logits[plain])
    tol = float((31 + 8 + dmax.max()) * R.U) + torch.from_numpy(R.lp_tolerance(c, None, ref.numpy()))
    ratio = float(((out["logprob"][plain, 0].double() - ref).abs() / tol).max())
    print(f"DECTAIL head + arg-max f{form}: logprob err / tol {ratio:.3g}")
    assert ratio <= 1.0
    assert bool(torch.isnan(out["logprob"][[r for r in range(B) if r not in plain], 0]).all())


def test_the_tap_refuses_by_name_and_launches_nothing(engine):
    c = R.case("head-f0-V768-B70-l1s1")
    good = R.tap_args(c)
    am = R.tap_args(R.case("argmax-B70-n8-blk-x"))
    ld = R.tap_args(R.case("load-B33-ids-clamped"))
    x3 = torch.zeros(96 * 576 * 3, dtype=torch.int16)
    for kw, msg in (({**good, "op": 4}, "op must be"), ({**good, "form": 2}, "form must be"), ({**am, "form": 1}, "one form only"),
                    ({**good, "B": 1025, "x": torch.zeros(1025, 576)}, "1 <= B <= 1024"),
                    ({**good, "V": 100, "W": torch.zeros(100, 576)}, "tile the vocabulary"),
                    ({"op": 0, "B": 70, "form": 1, "V": 96, "W": torch.zeros(96, 576), "x_img": x3}, "does not tile it"),
                    ({**R.tap_args(R.case("head-f0-V96-B1-l1s1")), "blk_live": torch.ones(1, dtype=torch.int32)}, "from two row blocks on"),
                    ({**am, "state": dict(am["state"]), "with_logprob": True}, "with_logprob without cand_sum"),
                    ({**good, "x": None}, "null argument: x"), ({**good, "cand_val": torch.zeros(70, 24)}, "cand_val is not an operand"),
                    ({**good, "x": None, "form": 1, "x_img": x3[:-2]}, "x_img: this launch takes"),
                    ({**am, "blk_left": None}, "go together"), ({**am, "row_of_slot": torch.zeros(96, dtype=torch.int32)}, "taken twice"),
                    ({**ld, "ld": 578, "x": torch.zeros(50, 578)}, "ld = 578"), ({**ld, "T_last": 1}, "with row_ids"),
                    ({**ld, "row_ids": None, "T_last": 2}, "must exist"), ({**good, "n_compactions": 1}, "goes with op 2 only")):
        with pytest.raises(E.EngineError, match=msg):
            engine.debug_dec_tail(**kw)
    # a capacity too small and a null output, straight at the C entry
    import ctypes as C
    d = E.DecTail()
    d.size, d.op, d.B, d.V = C.sizeof(E.DecTail), 3, 1, 0
    d.ld, d.n_src, d.T_last = 576, 1, 1
    src, out = torch.zeros(1, 576), torch.zeros(64 * 576)
    args = ([engine.h, C.byref(d), None, src.data_ptr(), None, 0] + [None] * 9 + [None, 0, None, None, None, 0, None, 0, None, None, 0, None, 0, None]
            + [out.data_ptr(), out.numel() * 4 - 4])
    assert engine.lib.mellow_debug_dec_tail(*args) != 0 and b"x_capacity" in engine.lib.mellow_last_error()
    args[-2] = None
    assert engine.lib.mellow_debug_dec_tail(*args) != 0 and b"out_x is null" in engine.lib.mellow_last_error()
    d.size -= 4
    assert engine.lib.mellow_debug_dec_tail(*args) != 0 and b"sizeof(mellow_dec_tail_t)" in engine.lib.mellow_last_error()
