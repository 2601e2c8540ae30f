"""GPU (-m gpu): the q/k/v, gate/up, down, fused down + q/k/v and final-norm launches of a decode step, ONE launch each on data this
module chose, through the tap mellow_debug_dec_gemv (include/mellow_hip.h) of an engine without weights.

Yardsticks (tests/dec_gemv_ref.py; tests/test_dec_gemv_ref_cpu.py checks them and shows which mutants they catch):
  * the float64 definition of every op and form, slab by slab and as the sum, within the per-element tolerance of gemm_ref's rule
    (the reference sets it, never the kernel); h3 decoded == guF and rope_cur == the table row bit for bit, xnewR == the float32
    sum in slab order, the position word, blk_snap, Q against the float64 product within one rounding, the algebra of the fusion;
  * guards: every output holds 0xFF bytes before the launch, so every word no live slot owns (slabs beyond Q2_NPQ / Q2_HC, rows
    beyond `rows`, every output of a stopped block) must still hold them, and every owned word is finite;
  * bit identities that hold by construction on ONE kernel instantiation: a launch == its repetition, a row of a batch == the row
    alone at the same RB, the same 32 rows in block 0 and in a later block (the kernels whose grid indexes the block).  Across
    instantiations (BLK on / off, RBM 1 / 2 / 4, 4 against 12 waves) each side is held to float64 above; whether they are
    bit-equal is printed, not asserted.
Every case prints err / tol (DESIGN.md 6z holds the figures)."""
import os
import sys

import pytest
import torch

from mellow_amd import engine as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dec_gemv_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (1, 1), (3, 1))
FORM_IDS = [f"op{op}-f{f}" for op, f in FORMS]


@pytest.fixture(scope="module")
def engine():
    e = E.Engine(device=0)          # no weights: the tap works on an engine that is not finalised
    yield e
    e.close()


def _case(op, form, B, blk=None):
    """a launch of (op, form) at B rows: the later q/k/v launch and the final norm on the down slabs"""
    return R.Case(op, form, B, kcd=R.KC_DOWN if op in (0, 4) else 0, blk=blk)


def _bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("cid", R.CASE_IDS)
def test_launch_against_float64_and_guards(engine, cid):
    c = R.case(cid)
    res = R.check(c, engine.debug_dec_gemv(**R.tap_args(c)))
    print(f"DECGEMV {cid}: " + ", ".join(f"{k} {v:.3g}" for k, v in res.items()))
    assert R.worst(res) <= 1.0, {k: v for k, v in res.items() if not v <= 1.0}


@pytest.mark.parametrize("op,form", FORMS, ids=FORM_IDS)
def test_a_launch_equals_its_repetition(engine, op, form):
    c = _case(op, form, 70)
    a, b = engine.debug_dec_gemv(**R.tap_args(c)), engine.debug_dec_gemv(**R.tap_args(c))
    for name in a:
        assert (a[name] == b[name]) if name == "pos" else _same(a[name], b[name]), name


@pytest.mark.parametrize("op,form", FORMS, ids=FORM_IDS)
def test_a_row_of_a_batch_equals_the_row_alone_at_the_same_RB(engine, op, form):
    c, row = _case(op, form, 70), 40
    inp = R.inputs(70)
    keep = torch.zeros(70, dtype=torch.bool)
    keep[row] = True
    full = R.decoded(c, engine.debug_dec_gemv(**R.tap_args(c)))
    alone = R.decoded(c, engine.debug_dec_gemv(**R.tap_args(c, R.sub_inputs(inp, 70, keep))))
    for name in full:
        assert _same(full[name][..., row, :], alone[name][..., row, :]), name
        assert not _same(full[name][..., row - 1, :], alone[name][..., row - 1, :]), name      # (the other rows did change)


@pytest.mark.parametrize("op,form", [f for f in FORMS if f[1] == 0], ids=[i for i in FORM_IDS if i.endswith("f0")])
def test_the_same_rows_in_block_0_and_in_block_2_give_the_same_bits(engine, op, form):
    c = _case(op, form, 96)                # the fp32 kernels: the grid indexes the row block, every block runs the same code
    inp = R.sub_inputs(R.inputs(130), 96)
    for name in ("x", "h", "ssq"):
        inp[name][64:96] = inp[name][0:32]
    inp["down"][:, 64:96] = inp["down"][:, 0:32]
    d = R.decoded(c, engine.debug_dec_gemv(**R.tap_args(c, inp)))
    for name in d:
        assert _same(d[name][..., 0:32, :], d[name][..., 64:96, :]), name
        assert not _same(d[name][..., 0:32, :], d[name][..., 32:64, :]), name


def test_instantiations_against_each_other_are_reported(engine):
    """BLK on / off, RBM 1 / 2 / 4 and 4 against 12 waves are different instantiations: nothing in the code or in DESIGN.md promises
    equal bits between them, so each side is held to float64 (test_launch_against_float64_and_guards) and this only reports"""
    inp130 = R.inputs(130)
    for op, form in FORMS:
        base = R.decoded(_case(op, form, 70), engine.debug_dec_gemv(**R.tap_args(_case(op, form, 70))))
        cb = _case(op, form, 70, blk=(1, 0, 1))
        blk = R.decoded(cb, engine.debug_dec_gemv(**R.tap_args(cb)))
        live = cb.live_rows
        eq = all(_same(base[n][..., live, :], blk[n][..., live, :]) for n in base)
        print(f"DECGEMV bits op{op}-f{form}: BLK on == BLK off on the live rows: {eq}")
    for op, form in ((1, 1), (3, 1), (3, 0)):
        got = {}
        for B in (20, 33, 70, 130):
            c = _case(op, form, B)
            got[B] = R.decoded(c, engine.debug_dec_gemv(**R.tap_args(c, R.sub_inputs(inp130, B))))
        for B in (33, 70, 130):
            eq = all(_same(got[20][n][..., :20, :], got[B][n][..., :20, :]) for n in got[20])
            what = "4 waves == 12 waves" if form == 0 else f"RBM 1 == RBM {2 if B == 33 else 4}"
            print(f"DECGEMV bits op{op}-f{form}: rows 0 .. 19 at RB 1 and at RB {(B + 31) // 32} ({what}): {eq}")
