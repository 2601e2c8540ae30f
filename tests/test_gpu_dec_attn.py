"""GPU (-m gpu): the decode attention (dec_attn_kernel) and the key-split merge of the o_proj (dec_oproj_kernel), ONE launch each on
data this module chose, through the tap mellow_debug_dec_attn (include/mellow_hip.h) of an engine without weights.

Yardsticks (tests/dec_attn_ref.py; tests/test_dec_attn_ref_cpu.py checks them and shows which mutants they catch):
  * the float64 definition, within tol = max(c * e_ref, 2^-20 * max|v|) per case, c = 8 * (chunks + 2) counted from the code
    (module docstring of dec_attn_ref; the reference sets the tolerance, never the kernel): merged decoded partials, appended
    k / v, x_mid' and ssq; and x_mid' against the float64 o_proj of the kernel's OWN decoded partials (merge + GEMV + residual);
  * bit identities the code states: a launch == its repetitions, a row of a batch == the row alone, two row blocks == one (fp32
    pages, two splits), xmidF16 / the F3 triples == xmidF, the fused x_new == the float32 sum in slab order, the bf16 append == the
    rounded fp32 append, page contents behind the context change no bit, a slot permutation moves whole rows;
  * guards: every output holds 0xFF bytes before the launches, so what no live slot owns must still hold them, and every page byte
    but position pos of the pages of the slots' examples must come back as sent.
The pages hold NaN in K and +-1e30 in V at every position > pos.  Every case prints err / tol (DESIGN.md 6w holds the figures)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from mellow_amd import engine as E

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dec_attn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = E.Engine(device=0)          # no weights: the tap works on an engine that is not finalised
    yield e
    e.close()


def _bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _all_ff(t):
    return bool((_bits(t) == -1).all())


def _page_values(p):
    """returned pages -> f32 values (bf16 pages arrive as int16 words)"""
    return p if p.dtype == torch.float32 else p.view(torch.bfloat16).float()


def launch(engine, c, inp, Wo=True, **kw):
    """one call of the tap on the inputs of a case -> the raw outputs"""
    fused = inp["fused"]
    args = dict(pos=inp["pos"], ctx_end=c.ctx_end, ts=c.ts, fused=fused, kv16=c.kv16, eps=inp["eps"], rope_cur=inp["rope_cur"],
                ssq1=None if fused else inp["ssq1"], down=inp["down"] if fused else None, Wo=inp["Wo"] if Wo else None)
    args.update(kw)
    return engine.debug_dec_attn(inp["slabs"], inp["x_mid"] if fused else inp["x_new"], inp["K"], inp["V"], **args)


def decode(out, rows, ts):
    """the raw outputs -> dict O [ts][rows][576], m / l [ts][rows][9], att [rows][576] (float64 merge) and, with the o_proj,
    x_mid / x16 [rows][576]"""
    d = {"O": R.f16_decode(out["att"], rows, ts)}
    d["m"], d["l"] = R.ml_decode(out["ml"], rows, ts)
    d["att"] = R.merge(d["O"], d["m"], d["l"])
    if "xmid" in out:
        d["x_mid"] = R.f32_decode(out["xmid"], rows)[0]
        if out["x16"].dtype == torch.float32:
            d["x16"] = R.f16_decode(out["x16"], rows)[0]
    return d


def check_guards(c, inp, out, live=None, page_of=None):
    """what a launch may and may not have written.  live: bool per slot (default: all); page_of: the example of every slot"""
    rows, ts, P, pos = c.rows, c.ts, c.P, inp["pos"]
    live = torch.ones(rows, dtype=torch.bool) if live is None else live
    page_of = torch.arange(rows) if page_of is None else page_of
    n_x = rows * R.HID
    assert out["gs"] == c.gs, f"the tap used gs = {out['gs']}, the rule gives {c.gs}"
    assert _all_ff(out["att"][ts * n_x:]), "the block after the partials was written"
    O, (m, l) = R.f16_decode(out["att"], rows, ts), R.ml_decode(out["ml"], rows, ts)
    for name, t in (("partials", O), ("att_ml m", m), ("att_ml l", l)):
        assert bool(torch.isfinite(t[:, live]).all()), f"{name}: an owned word is not written or not finite"
        assert _all_ff(t[:, ~live]), f"{name}: a word of a slot that does not run was written"
    # pages: every byte as sent, but position pos of the pages the live slots extend; the page set of no example untouched
    for name in ("k", "v"):
        sent = inp[name.upper()]
        sent = R.bf16_bits(sent) if c.kv16 else sent
        got = out[name]
        assert _all_ff(got[P]), f"{name}: the page set of no example was written"
        written = torch.zeros(P, dtype=torch.bool)
        written[page_of[live]] = True
        keep = torch.ones(P, c.Tmax, dtype=torch.bool)
        keep[written, pos] = False
        keep = keep[:, None, :, None].expand(P, 3, c.Tmax, 64)
        same = _bits(got[:P]) == _bits(sent)
        if c.kv16:          # (the device's fp32 -> bf16 conversion may hand back another NaN pattern than the host's: a NaN stays a NaN)
            same |= torch.isnan(_page_values(got[:P])) & torch.isnan(inp[name.upper()])
        assert bool(same[keep].all()), f"{name}: a page byte outside position pos of the owning examples changed"
        assert bool(torch.isfinite(_page_values(got[:P])[written][:, :, pos]).all()), f"{name}: the appended values are not finite"
    assert _all_ff(out["xnew"][rows:]), "xnewR rows [rows, rows + 32) were written"
    if "xmid" in out:
        assert _all_ff(out["ssq"][rows:]) and _all_ff(out["ssq"][:, 36:]), "ssq rows beyond `rows` or columns 36 .. 39 were written"
        x = R.f32_decode(out["xmid"], rows)[0]
        assert bool(torch.isfinite(x[live]).all()) and bool(torch.isfinite(out["ssq"][:rows, :36][live]).all()), "x_mid / ssq: an owned word is not finite"


def _ratio(what, got, ref, tol):
    m = R.miss(got, ref, tol)
    print(f"DECATTN {what}: err / tol {m:.3f} (tol {tol:.3e})")
    return m


# ---- A. against float64; the guards and the cheap identities ride on the same launches ------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("cid", R.CASE_IDS)
def test_against_float64(engine, cid, fused):
    c, inp, r = R.case(cid), R.inputs(cid, fused), R.reference(cid, fused)
    B, rows, pos = c.B, c.rows, c.pos
    out = launch(engine, c, inp)
    check_guards(c, inp, out)
    d = decode(out, rows, c.ts)
    ref, tol = r["ref"], r["tol"]
    worst = {"att": _ratio(f"{cid} fused {int(fused)} att", d["att"][:B], ref["att"], tol["att"])}
    for name in ("k", "v"):
        got = _page_values(out[name])[:B, :, pos]
        # the bf16 append is rounded once, to nearest: half an ulp of 8 significant bits, 2^-8 |x| (its bits: test_bf16_append_...)
        t = tol[name] + (2.0 ** -8 * float(ref[name].abs().max()) if c.kv16 else 0.0)
        worst[name] = _ratio(f"{cid} fused {int(fused)} appended {name}", got, ref[name], t)
    worst["x_mid"] = _ratio(f"{cid} fused {int(fused)} x_mid'", d["x_mid"][:B], ref["x_mid"], tol["x_mid"])
    worst["ssq"] = _ratio(f"{cid} fused {int(fused)} ssq", out["ssq"][:B, :36], ref["ssq"], tol["ssq"])
    own, own_tol = R.own_oproj(d["att"][:B], out["xnew"][:B], inp["Wo"])
    worst["own"] = _ratio(f"{cid} fused {int(fused)} x_mid' against the o_proj of its own partials", d["x_mid"][:B], own, own_tol)
    # identities that cost no launch
    assert _same(d["x16"], d["x_mid"]), "xmidF16 decoded differs from xmidF decoded"
    if fused:
        x = inp["x_mid"].clone()
        for s in range(R.N_DOWN):
            x = x + inp["down"][s]
        assert _same(out["xnew"][:B], x), "fused x_new is not the float32 sum ((x_mid + d0) + d1) + ..."
        assert bool((out["xnew"][B:rows] == 0).all())
    else:
        assert _same(out["xnew"][:B], inp["x_new"]) and bool((out["xnew"][B:rows] == 0).all())
    assert all(v <= 1.0 for v in worst.values()), worst


# ---- B. bit identities ---------------------------------------------------------------------------------------------------------------
def _assert_same_outputs(a, b, what, keys=("att", "ml", "k", "v", "xnew", "xmid", "x16", "ssq")):
    for k in keys:
        if k in a:
            assert _same(a[k], b[k]), f"{what}: {k} differs in {int((_bits(a[k]) != _bits(b[k])).sum())} words"


@pytest.mark.parametrize("cid", R.CASE_IDS)
def test_a_launch_equals_its_repetitions(engine, cid):
    """raw partials, pages and every other output of three launches (a missed barrier or a race on the new key shows as a flaky word)"""
    c, inp = R.case(cid), R.inputs(cid, bool(R.CASE_IDS.index(cid) % 2))
    first = launch(engine, c, inp)
    for _ in range(2):
        _assert_same_outputs(launch(engine, c, inp), first, cid)


def _row_alone(inp, r):
    """the inputs of slot r as a batch of one (its pages become example 0)"""
    one = dict(inp)
    for k in ("slabs", "down"):
        if k in inp:
            one[k] = inp[k][:, r:r + 1].contiguous()
    for k in ("x_new", "x_mid", "ssq1"):
        if k in inp:
            one[k] = inp[k][r:r + 1].contiguous()
    for k in ("K", "V"):
        one[k] = inp[k][:33].clone()
        one[k][0] = inp[k][r]
    return one


def _assert_rows_equal(c, out_a, rows_a, sel_a, out_b, rows_b, sel_b, pos, pages_a, pages_b, what):
    """slots sel_a of launch a == slots sel_b of launch b, in every per-slot output; their appends in pages_a / pages_b"""
    da, db = decode(out_a, rows_a, c.ts), decode(out_b, rows_b, c.ts)
    for k in ("O", "m", "l"):
        assert _same(da[k][:, sel_a], db[k][:, sel_b]), f"{what}: {k} differs"
    for k in ("x_mid", "x16"):
        assert _same(da[k][sel_a], db[k][sel_b]), f"{what}: {k} differs"
    assert _same(out_a["ssq"][sel_a], out_b["ssq"][sel_b]) and _same(out_a["xnew"][sel_a], out_b["xnew"][sel_b]), f"{what}: ssq / xnew differ"
    for k in ("k", "v"):
        assert _same(out_a[k][pages_a][:, :, pos], out_b[k][pages_b][:, :, pos]), f"{what}: the appended {k} differs"


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("cid", ["b-B3-T512-pos223-end449-ts2-fp32", "e-B3-T520-pos513-end520-ts2-bf16", "d-B33-T512-pos449-end512-ts1-fp32"])
def test_a_row_of_a_batch_equals_the_row_alone(engine, cid, fused):
    c, inp = R.case(cid), R.inputs(cid, fused)
    whole = launch(engine, c, inp)
    for r in (0, 1, c.B - 1):
        if c.RB == 1:
            one = R.Case(c.group, 1, c.Tmax, c.pos, c.ctx_end, c.ts, c.kv16, "a row alone")
            alone = launch(engine, one, _row_alone(inp, r))
            assert alone["gs"] == whole["gs"]
            _assert_rows_equal(c, whole, c.rows, [r], alone, 32, [0], c.pos, [r], [0], f"{cid} row {r}")
        else:           # two row blocks and one split: the row alone in a batch that keeps two row blocks (one row block runs two splits)
            sel = torch.tensor([r] + [s for s in range(c.B) if s != r])
            sub = dict(inp)
            for k in ("slabs", "down"):
                if k in inp:
                    sub[k] = inp[k][:, sel].contiguous()
            for k in ("x_new", "x_mid", "ssq1"):
                if k in inp:
                    sub[k] = inp[k][sel].contiguous()
            for k in ("K", "V"):
                sub[k] = inp[k].clone()
                sub[k][:len(sel)] = inp[k][sel]
            two = R.Case(c.group, len(sel), c.Tmax, c.pos, c.ctx_end, c.ts, c.kv16, "the row first in a reordered batch")
            other = launch(engine, two, sub)
            _assert_rows_equal(c, whole, c.rows, [r], other, 64, [0], c.pos, [r], [0], f"{cid} row {r}")


@pytest.mark.parametrize("fused", [False, True])
def test_fp32_pages_two_splits_two_row_blocks_equal_one(engine, fused):
    """the exact-fp32 promise of kernels.h (dec_key_splits): with two key splits a row's attention does not depend on the number of
    row blocks -- the peeled-first-chunk kernel of two row blocks against the plain loop of one, and the 16-row o_proj against the
    8-row one"""
    cid = "d-B33-T512-pos225-end449-ts2-fp32"
    c, inp = R.case(cid), R.inputs(cid, fused)
    whole = launch(engine, c, inp)
    one = R.Case(c.group, 32, c.Tmax, c.pos, c.ctx_end, c.ts, False, "the first row block alone")
    sub = dict(inp)
    for k in ("slabs", "down"):
        if k in inp:
            sub[k] = inp[k][:, :32].contiguous()
    for k in ("x_new", "x_mid", "ssq1"):
        if k in inp:
            sub[k] = inp[k][:32].contiguous()
    sub["K"], sub["V"] = inp["K"][:33], inp["V"][:33]
    first = launch(engine, one, sub)
    assert first["gs"] == whole["gs"]
    sel = list(range(32))
    _assert_rows_equal(c, whole, 64, sel, first, 32, sel, c.pos, sel, sel, "rows 0 .. 31 of B = 33 against B = 32")
    alone = launch(engine, R.Case(c.group, 1, c.Tmax, c.pos, c.ctx_end, c.ts, False, "row 32 alone"), _row_alone(inp, 32))
    _assert_rows_equal(c, whole, 64, [32], alone, 32, [0], c.pos, [32], [0], "row 32 of B = 33 against the row alone")


@pytest.mark.parametrize("cid", ["b-B1-T512-pos224-end449-ts2-fp32", "d-B64-T512-pos447-end512-ts1-fp32", "e-B33-T520-pos257-end520-ts2-bf16"])
def test_f3_triples_decode_to_the_words_of_xmid(engine, cid):
    c, inp = R.case(cid), R.inputs(cid, True)
    plain, x3 = launch(engine, c, inp), launch(engine, c, inp, want_x3=True)
    check_guards(c, inp, x3)
    _assert_same_outputs(x3, plain, cid, keys=("att", "ml", "k", "v", "xnew", "xmid", "ssq"))
    x = R.f32_decode(x3["xmid"], c.rows)[0]
    assert x3["x16"].dtype == torch.int16 and x3["x16"].shape == (2, c.rows * R.HID * 3)
    assert _same(R.f3_decode(x3["x16"][0], c.rows, R.f3_32_index), x), "the F3-32 triples do not decode to the words of xmidF"
    assert _same(R.f3_decode(x3["x16"][1], c.rows, R.f3_16_index), x), "the F3-16 triples do not decode to the words of xmidF"


@pytest.mark.parametrize("cid", [i for i in R.CASE_IDS if R.case(i).kv16 and R.case(i).Tmax <= 64])
def test_bf16_append_is_the_rounded_fp32_append(engine, cid):
    c, inp = R.case(cid), R.inputs(cid, False)
    o16 = launch(engine, c, inp, Wo=False)
    c32 = R.Case(c.group, c.B, c.Tmax, c.pos, c.ctx_end, c.ts, False, "the same launch on fp32 pages")
    o32 = launch(engine, c32, inp, Wo=False)
    for k in ("k", "v"):
        assert torch.equal(o16[k][:c.rows, :, c.pos], R.bf16_bits(o32[k][:c.rows, :, c.pos])), f"appended {k}: bf16 page != rne(fp32 page)"


@pytest.mark.parametrize("cid", ["a-B3-T64-pos4-end8-ts2-fp32", "b-B32-T512-pos225-end449-ts2-fp32", "d-B33-T512-pos223-end512-ts1-fp32",
                                 "e-B3-T64-pos32-end64-ts2-bf16", "e-B33-T520-pos257-end520-ts2-bf16", "f-B3-T62-pos61-end62-ts2-bf16"])
def test_pages_behind_the_context_change_no_bit(engine, cid):
    """other NaN patterns in K and other finite values in V at the positions > pos: every output keeps its bits"""
    c, inp = R.case(cid), R.inputs(cid, True)
    base = launch(engine, c, inp)
    alt = dict(inp)
    K, V = inp["K"].clone(), inp["V"].clone()
    n = c.Tmax - c.pos - 1
    if n > 0:
        # quiet with a payload, negative with every payload bit, signalling, negative quiet (bf16 pages: patterns a bf16 word holds)
        pat = torch.tensor([0x7FC10000, -0x10000, 0x7F810000, -0x400000] if c.kv16 else [0x7FC00001, -1, 0x7F800001, -0x400000], dtype=torch.int32)
        K.view(torch.int32)[:, :, c.pos + 1:] = pat[torch.arange(n * 64) % 4].view(n, 64)
        assert bool(torch.isnan(K[:, :, c.pos + 1:]).all())
        V[:, :, c.pos + 1:] = torch.where(inp["V"][:, :, c.pos + 1:] > 0, -3.0e38, 0.0)
        if c.kv16:
            V = V.to(torch.bfloat16).float()
    alt["K"], alt["V"] = K, V
    got = launch(engine, c, alt)
    _assert_same_outputs(got, base, cid, keys=("att", "ml", "xnew", "xmid", "x16", "ssq"))
    for k in ("k", "v"):
        assert _same(got[k][:, :, :c.pos + 1], base[k][:, :, :c.pos + 1])


@pytest.mark.parametrize("cid,fused", [("d-B64-T64-pos5-end8-ts2-fp32", False), ("d-B64-T512-pos225-end512-ts1-fp32", True), ("e-B64-T64-pos33-end64-ts2-bf16", True)])
def test_slot_permutation_and_dead_slots(engine, cid, fused):
    """row_of_slot a permutation: slot s computes example perm[s] -- its outputs are the unpermuted launch's for that example and its
    append lands in page perm[s], not in page s.  Then slots with row_of_slot -1 and a block with blk_live 0: what they own stays 0xFF
    (an empty slot: its partials, att_ml and page; a dead block: also xmidF, xmidF16, ssq and the fused x_new rows.  dec_oproj_kernel has
    no per-slot exit, so the x_mid row of an empty slot in a LIVE block is computed from the 0xFF partials and is not asserted)."""
    c, inp = R.case(cid), R.inputs(cid, fused)
    assert c.B == 64
    base = launch(engine, c, inp)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(11))
    assert bool((perm != torch.arange(64)).any()) and bool(((perm < 32) != (torch.arange(64) < 32)).any())     # rows change block too
    sub = dict(inp)
    for k in ("slabs", "down"):
        if k in inp:
            sub[k] = inp[k][:, perm].contiguous()
    for k in ("x_new", "x_mid", "ssq1"):
        if k in inp:
            sub[k] = inp[k][perm].contiguous()
    got = launch(engine, c, sub, row_of_slot=perm)
    check_guards(c, inp, got, page_of=perm)
    slots = list(range(64))
    _assert_rows_equal(c, got, 64, slots, base, 64, perm, c.pos, perm, perm, f"{cid} permuted")
    for k in ("k", "v"):       # the pages as a whole: the same launch result, wherever the slot sat
        assert _same(got[k], base[k]), f"{k} pages differ from the unpermuted launch"
    # empty slots in a live block, and a dead block
    ros = perm.clone()
    ros[[3, 17, 40]] = -1
    live = ros >= 0
    got = launch(engine, c, sub, row_of_slot=ros)
    check_guards(c, inp, got, live=live, page_of=ros)
    _assert_rows_equal(c, got, 64, [s for s in slots if live[s]], base, 64, perm[live], c.pos, perm[live], perm[live], f"{cid} with empty slots")
    got = launch(engine, c, sub, row_of_slot=perm, blk_live=[1, 0])
    live = torch.arange(64) < 32
    check_guards(c, inp, got, live=live, page_of=perm)
    x = R.f32_decode(got["xmid"], 64)[0]
    assert _all_ff(x[32:]) and _all_ff(R.f16_decode(got["x16"], 64)[0][32:]) and _all_ff(got["ssq"][32:64]), "a block with blk_live 0 wrote x_mid / ssq"
    assert not fused or _all_ff(got["xnew"][32:64]), "a block with blk_live 0 wrote x_new"
    _assert_rows_equal(c, got, 64, slots[:32], base, 64, perm[:32], c.pos, perm[:32], perm[:32], f"{cid} with a dead block")
    got = launch(engine, c, inp, blk_live=[0, 1])               # blk_live alone: slot == example
    check_guards(c, inp, got, live=~live)
    _assert_rows_equal(c, got, 64, slots[32:], base, 64, slots[32:], c.pos, slots[32:], slots[32:], f"{cid} with block 0 dead")


# ---- D. refusals by name --------------------------------------------------------------------------------------------------------------
def test_refusals_by_name_then_a_good_launch(engine):
    cid = "a-B3-T64-pos4-end8-ts2-fp32"
    c, inp, inpf = R.case(cid), R.inputs(cid, False), R.inputs(cid, True)
    c2, inp2 = R.case("d-B64-T64-pos5-end8-ts2-fp32"), R.inputs("d-B64-T64-pos5-end8-ts2-fp32", False)
    empty = dict(inp, slabs=inp["slabs"][:, :0], x_new=inp["x_new"][:0], ssq1=inp["ssq1"][:0])
    short = dict(inp, K=inp["K"][:, :, :1], V=inp["V"][:, :, :1])
    few = dict(inp, K=inp["K"][:31], V=inp["V"][:31])
    dup = torch.arange(64, dtype=torch.int32)
    dup[5] = 6
    far = torch.arange(64, dtype=torch.int32)
    far[5] = c2.P
    bad = [
        (c, empty, {}, "B = 0"),
        (c, inp, {"pos": 0}, r"pos = 0 must lie in \[1, Tmax"),
        (c, inp, {"pos": 64, "ctx_end": 64}, r"pos = 64 must lie in \[1, Tmax"),
        (c, inp, {"ctx_end": 4}, r"ctx_end = 4 must lie in \(pos = 4"),
        (c, inp, {"ctx_end": 65}, r"ctx_end = 65 must lie in \(pos = 4, Tmax = 64\]"),
        (c, short, {}, "Tmax = 1 is not a page length of the engine"),
        (c, few, {}, "P = 31 page sets"),
        (c, inp, {"ts": 1}, "ts = 1 is not a key split count of RB = 1"),
        (c, inp, {"ts": 3}, "ts = 3 is not a key split count"),
        (c2, inp2, {"ts": 1, "kv16": True}, "ts = 1 is not a key split count of RB = 2 row blocks with bf16 pages"),
        (c2, inp2, {"ts": 4}, "ts = 4 is not a key split count"),
        (c, inp, {"blk_live": [1]}, "blk_live / row_of_slot exist from two row blocks on"),
        (c, inp, {"row_of_slot": list(range(32))}, "blk_live / row_of_slot exist from two row blocks on"),
        (c2, inp2, {"row_of_slot": dup}, r"row_of_slot\[6\] = 6 is outside \[0, P = 65\) or taken twice"),
        (c2, inp2, {"row_of_slot": far}, r"row_of_slot\[5\] = 65 is outside"),
        (c2, inp2, {"row_of_slot": -2 * torch.ones(64, dtype=torch.int32)}, r"row_of_slot\[0\] = -2 is outside"),
        (c, inp, {"Wo": None, "want_x3": True}, "want_x3 without Wo"),
        (c, inp, {"ssq1": None}, "fused 0 needs ssq1"),
        (c, inpf, {"down": None}, "fused 1 needs the down slabs"),
        (c, inp, {"eps": float("nan")}, "eps = nan must be finite"),
        (c, inp, {"eps": float("inf")}, "eps = inf must be finite"),
        (c, inp, {"eps": -1e-5}, "must be finite and >= 0"),
    ]
    for cc, i, kw, msg in bad:
        with pytest.raises(E.EngineError, match=msg):
            launch(engine, cc, i, **kw)
    # the C entry point itself: the descriptor's size, fused, null pointers and every capacity
    fn, p = engine.lib.mellow_debug_dec_attn, lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    rows, n_x = 32, 32 * R.HID
    bufs = {"att": torch.empty(2 * n_x + 32 * R.HID), "ml": torch.empty(9 * rows * 2 * 2), "k": torch.empty(c.P + 1, 3, 64, 64), "v": torch.empty(c.P + 1, 3, 64, 64),
            "xnew": torch.empty(rows + 32, R.HID), "xmid": torch.empty(n_x), "x16": torch.empty(n_x), "ssq": torch.empty(rows + 32, 40)}
    gs = C.c_int32(-1)

    def call(desc=None, null=(), cut=None, x3=False):
        d = E.DecAttn()
        d.size, d.B, d.P, d.pos, d.Tmax, d.ctx_end, d.ts, d.fused, d.kv16, d.want_x3, d.eps = C.sizeof(E.DecAttn), 3, c.P, 4, 64, 8, 2, 0, 0, int(x3), 1e-5
        for k, v in (desc or {}).items():
            setattr(d, k, v)
        a = {k: (None if k in null else p(v)) for k, v in dict(slabs=inp["slabs"], ssq1=inp["ssq1"], x_res=inp["x_new"], K=inp["K"], V=inp["V"], Wo=inp["Wo"]).items()}
        o = {k: (None if k in null else p(v)) for k, v in bufs.items()}
        cap = {k: v.numel() * 4 - (1 if k == cut else 0) for k, v in bufs.items()}
        return fn(engine.h, C.byref(d), a["slabs"], a["ssq1"], a["x_res"], None, None, a["K"], a["V"], None, None, a["Wo"],
                  None if "gs" in null else C.cast(C.byref(gs), C.c_void_p), o["att"], cap["att"], o["ml"], cap["ml"], o["k"], o["v"], cap["k"],
                  o["xnew"], cap["xnew"], o["xmid"], cap["xmid"], o["x16"], cap["x16"], o["ssq"], cap["ssq"])

    def refused(msg, **kw):
        assert call(**kw) != 0
        assert msg in engine.lib.mellow_last_error().decode(), engine.lib.mellow_last_error().decode()

    refused("is not sizeof(mellow_dec_attn_t)", desc={"size": 40})
    refused("fused must be 0", desc={"fused": 2})
    for name in ("slabs", "x_res", "K", "V", "gs"):
        refused("null argument", null=(name,))
    for name in ("att", "ml", "k", "xnew", "xmid", "x16", "ssq"):
        refused(f"{'kv' if name == 'k' else name}_capacity", cut=name)
        refused(f"{'kv' if name == 'k' else name}_capacity", null=(name,))
    refused("kv_capacity", null=("v",))
    refused("x16_capacity", x3=True)                   # the two F3 images take 12 bytes per element: the plain capacity is too small
    assert gs.value == -1                               # nothing was computed, nothing launched
    assert call() == 0 and gs.value == 1
    # the engine is still usable, and a good launch is what it was
    r = R.reference(cid, False)
    out = launch(engine, c, inp)
    check_guards(c, inp, out)
    assert R.miss(decode(out, 32, 2)["x_mid"][:3], r["ref"]["x_mid"], r["tol"]["x_mid"]) <= 1.0
    # rope_cur NULL (as the C call above passed it): row pos of the engine's own tables
    cos, sin = np.empty((64, 32), dtype=np.float32), np.empty((64, 32), dtype=np.float32)
    fp = C.POINTER(C.c_float)
    assert engine.lib.mellow_host_rope_tables(float(engine.cfg.rope_theta), 64, 64, cos.ctypes.data_as(fp), sin.ctypes.data_as(fp)) == 0
    own = dict(inp, rope_cur=torch.from_numpy(np.concatenate([cos[c.pos], sin[c.pos]])))
    null = launch(engine, c, inp, rope_cur=None)
    assert _same(null["xmid"], bufs["xmid"]) and not _same(null["xmid"], out["xmid"])
    _assert_same_outputs(launch(engine, c, own), null, "rope_cur NULL against the table row passed explicitly")
    ref = R.dec_attn_ref(own)
    assert R.miss(decode(null, 32, 2)["x_mid"][:3], ref["x_mid"], r["tol"]["x_mid"]) <= 1.0
