"""CPU: what the debug_* wrappers of Engine hand to the C library, tap by tap, against a recording fake of libmellow_hip.so.  The
fake defines the nine mellow_debug_* symbols of the launch taps and the two GEMM taps, records every argument and returns 0; it
writes nothing, so nothing is computed.  Every case asserts the whole call -- the scalars, every descriptor field, which pointers
are None, the byte count of every capacity -- and the dtype and shape of every tensor returned, against values written out below."""
import ctypes as C

import pytest
import torch

from mellow_amd import engine as E

# the arguments of include/mellow_hip.h, by symbol
ARGS = {
    "mellow_debug_gemm_f32": "h mode A M K W N C_out iters ms2",
    "mellow_debug_gemm_fp8": "h A M K W N C_out iters ms_out",
    "mellow_debug_gemm_epi": "h d A W bias resid crow_map rs_ssq rope_cos rope_sin out_c c_capacity out_c3 c3_capacity out_ssq ssq_capacity "
                             "out_q q_capacity out_k out_v kv_capacity",
    "mellow_debug_norm": "h op form x M C w b eps row_map ntok n R out out_capacity out_scales scales_capacity",
    "mellow_debug_dec_attn": "h d slabs ssq1 x_res down rope_cur k_pages v_pages blk_live row_of_slot Wo out_gs out_att att_capacity out_ml "
                             "ml_capacity out_k out_v kv_capacity out_xnew xnew_capacity out_xmid xmid_capacity out_x16 x16_capacity out_ssq "
                             "ssq_capacity",
    "mellow_debug_dec_gemv": "h d W W2 x down h_ x_img x_img_bytes h_img h_img_bytes ssq rope_cos rope_sin blk_live out_pq pq_capacity out_down "
                             "down_capacity out_ssq1 ssq1_capacity out_xnew xnew_capacity out_rope out_pos out_gu gu_capacity out_h3 h3_capacity "
                             "out_xn xn_capacity out_snap out_q q_capacity",
    "mellow_debug_dec_tail": "h d W x x_img x_img_bytes blk_live cand_val cand_idx cand_sum seen_stop blk_left blk_snap row_of_slot row_ids "
                             "out_logits logits_capacity out_cand_val out_cand_idx out_cand_sum cand_capacity out_tokens tokens_capacity "
                             "out_record out_logprob record_capacity out_state state_capacity out_progress out_x x_capacity",
    "mellow_debug_prefill_attn": "h variant q k v B T Tmax qpos0 out_form out out_capacity",
    "mellow_debug_window_attn": "h qkv M C nH bias mask nW in16 out_form out out_capacity",
}
ARGS = {sym: names.split() for sym, names in ARGS.items()}


def _plain(a):
    """an argument as the expectations below write it: "p" for an address, None for none, a tuple of the fields for a descriptor"""
    if a is None:
        return None
    if isinstance(a, C.c_void_p):
        return "p" if a.value else None
    if isinstance(a, C.Array):
        return "p"
    if hasattr(a, "_obj"):
        o = a._obj
        return tuple(getattr(o, f) for f, _ in o._fields_) if isinstance(o, C.Structure) else "p"
    assert isinstance(a, (int, float)), a
    return a


class FakeLib:
    def __init__(self):
        self.calls = []
        for sym in ARGS:
            setattr(self, sym, lambda *a, _s=sym: self._call(_s, *a))

    def _call(self, sym, *args):
        assert len(args) == len(ARGS[sym]), (sym, len(args))
        self.calls.append((sym,) + tuple(_plain(a) for a in args[1:]))
        return 0


def _engine():
    e = object.__new__(E.Engine)
    e.tdev, e.lm, e.lib, e.h = torch.device("cpu"), E.LMConfig.load(), FakeLib(), None
    e._sync_inputs = lambda: None
    return e


def _returned(r):
    """a result as the expectations write it: (dtype, shape) for a tensor, the type's name for anything else"""
    if isinstance(r, torch.Tensor):
        return (str(r.dtype).replace("torch.", ""), tuple(r.shape))
    if isinstance(r, dict):
        return {k: _returned(v) for k, v in r.items()}
    if isinstance(r, tuple):
        return tuple(_returned(v) for v in r)
    return type(r).__name__


def z(*shape):
    return torch.zeros(shape)


def zi(*shape):
    return torch.zeros(shape, dtype=torch.int32)


def z16(*shape):
    return torch.zeros(shape, dtype=torch.int16)


def perm(n):
    return list(range(n))


# B = 33 decode rows: 64 padded rows, 2 row blocks
DA = dict(slabs=z(8, 33, 960), x_res=z(33, 576), k_pages=z(64, 3, 8, 64), v_pages=z(64, 3, 8, 64), pos=3, ctx_end=4, ts=2, ssq1=z(33, 8))
DAF = dict(DA, slabs=z(6, 33, 960), ssq1=None, fused=True, down=z(4, 33, 576))
STATE = dict(max_len=5, stop_id=2, T0=7, pos=9, n_seen=1, arrive=0, ticket=3)
LOOP = dict(cand_val=z(33, 2), cand_idx=zi(33, 2), state=STATE, seen_stop=zi(64))

# id -> (method, positional arguments, keyword arguments)
CASES = {
    "gemm_f32": ("debug_gemm_f32", (z(4, 32), z(8, 32)), dict(mode=16)),
    "gemm_f32_timed": ("debug_gemm_f32", (z(4, 32), z(8, 32)), dict(iters=2)),
    "gemm_fp8": ("debug_gemm_fp8", (z(4, 32), z(8, 32)), dict()),
    "gemm_fp8_timed": ("debug_gemm_fp8", (z(4, 32), z(8, 32)), dict(iters=3)),
    "epi_linear": ("debug_gemm_epi", (z(33, 32), z(6, 32)), dict()),
    "epi_linear_operands": ("debug_gemm_epi", (z(33, 32), z(6, 32)), dict(N=8, act="gelu", bias=z(6), resid=z(33, 8), ldc=16, rs_ssq=z(33, 2),
                                                                          rs_dim=64.0, rs_eps=0.5, no_x3w=True)),
    "epi_k17": ("debug_gemm_epi", (z(33, 48), z(64, 48)), dict(kernel=17, want_c3=True, want_ssq=True, crow_map=perm(11), rows_out=12,
                                                               resid=z(36, 64), in_place=True, splitk_max=4)),
    "epi_k17_c3_only": ("debug_gemm_epi", (z(33, 48), z(64, 48)), dict(kernel=17, want_c=False, want_c3=True, act="sigmoid")),
    "epi_swiglu": ("debug_gemm_epi", (z(33, 32), z(32, 32)), dict(kernel=16, epi="swiglu")),
    "epi_qkv_rope": ("debug_gemm_epi", (z(4, 32), z(960, 32)), dict(epi="qkv_rope", T=2, Tmax=4, rope=(z(4, 32), z(4, 32)))),
    "epi_qkv_own_tables": ("debug_gemm_epi", (z(4, 32), z(960, 32)), dict(epi="qkv_rope", T=2, Tmax=4)),
    "epi_qkv_at": ("debug_gemm_epi", (z(4, 32), z(960, 32)), dict(epi="qkv_rope", T=3, Tmax=4, pos0=1)),
    "norm_ln_0": ("debug_norm", (z(33, 96),), dict(w=z(96), b=z(96))),
    "norm_ln_1_map": ("debug_norm", (z(33, 96),), dict(form=1, w=z(96), b=z(96), row_map=perm(33), eps=1e-6)),
    "norm_ln_2": ("debug_norm", (z(33, 96),), dict(form=2, w=z(96), b=z(96))),
    "norm_ln_0_map": ("debug_norm", (z(33, 96),), dict(w=z(96), b=z(96), row_map=perm(11))),
    "norm_rms_0": ("debug_norm", (z(33, 96),), dict(op="rmsnorm", w=z(96), eps=0.25)),
    "norm_rms_1": ("debug_norm", (z(33, 96),), dict(op="rmsnorm", form=1, w=z(96))),
    "norm_rms_2": ("debug_norm", (z(33, 96),), dict(op="rmsnorm", form=2, w=z(96))),
    "norm_merge": ("debug_norm", (z(1, 4, 4),), dict(op="merge", w=z(16), b=z(16), n=1, R=2)),
    "norm_none_1": ("debug_norm", (z(33, 96),), dict(op="none", form=1)),
    "norm_none_2": ("debug_norm", (z(33, 96),), dict(op="none", form=2)),
    "attn": ("debug_dec_attn", (), dict(DA)),
    "attn_kv16_rope": ("debug_dec_attn", (), dict(DA, kv16=True, rope_cur=z(64), eps=0.5)),
    "attn_fused": ("debug_dec_attn", (), dict(DAF)),
    "attn_fused_kv16_wo": ("debug_dec_attn", (), dict(DAF, kv16=True, Wo=z(576, 576))),
    "attn_wo": ("debug_dec_attn", (), dict(DA, Wo=z(576, 576))),
    "attn_wo_x3": ("debug_dec_attn", (), dict(DA, Wo=z(576, 576), want_x3=True)),
    "attn_blocks": ("debug_dec_attn", (), dict(DA, blk_live=[1, 0], row_of_slot=perm(64))),
    "gemv_0_first_tables": ("debug_dec_gemv", (0, 33, z(960, 576)), dict(x=z(33, 576), first=True, inc_pos=True, pos=2, Tmax=8,
                                                                         rope_cos=z(8, 32), rope_sin=z(8, 32))),
    "gemv_0_first": ("debug_dec_gemv", (0, 33, z(960, 576)), dict(x=z(33, 576), first=True, pos=2, Tmax=8, eps=0.5)),
    "gemv_0_later": ("debug_dec_gemv", (0, 33, z(960, 576)), dict(x=z(33, 576), down=z(8, 33, 576), kcd=8)),
    "gemv_1": ("debug_dec_gemv", (1, 33, z(1536, 576)), dict(W2=z(1536, 576), x_img=z(64 * 576), ssq=z(64, 40))),
    "gemv_1_x3": ("debug_dec_gemv", (1, 33, z(1536, 576)), dict(W2=z(1536, 576), form=1, x_img=z16(64 * 576 * 3), ssq=z(64, 40))),
    "gemv_2": ("debug_dec_gemv", (2, 33, z(576, 1536)), dict(h=z(33, 1536))),
    "gemv_3": ("debug_dec_gemv", (3, 33, z(960, 576)), dict(W2=z(576, 1536), x=z(33, 576), h=z(33, 1536))),
    "gemv_3_x3": ("debug_dec_gemv", (3, 33, z(960, 576)), dict(W2=z(576, 1536), form=1, x_img=z16(64 * 576 * 3), h_img=z16(64 * 1536 * 3))),
    "gemv_4": ("debug_dec_gemv", (4, 33, z(576)), dict(x=z(33, 576), down=z(8, 33, 576), kcd=8)),
    "gemv_4_x3": ("debug_dec_gemv", (4, 33, z(576)), dict(x=z(33, 576), want_x3=True)),
    "gemv_4_blocks": ("debug_dec_gemv", (4, 33, z(576)), dict(x=z(33, 576), blk_live=[1, 1])),
    "tail_head": ("debug_dec_tail", (0, 33), dict(V=64, W=z(64, 576), x=z(33, 576), want_logits=True, want_sum=True)),
    "tail_head_x3": ("debug_dec_tail", (0, 33), dict(form=1, V=64, W=z(64, 576), x_img=z16(64 * 576 * 3), blk_live=[1, 0])),
    "tail_argmax": ("debug_dec_tail", (1, 33), dict(V=64, cand_val=z(33, 2), cand_idx=zi(33, 2))),
    "tail_argmax_state": ("debug_dec_tail", (1, 33), dict(LOOP, V=64, W=z(64, 576), write_x=True, blk_left=[32, 1], blk_live=[1, 1],
                                                          blk_snap=[1, 1], row_of_slot=perm(64))),
    "tail_argmax_logprob": ("debug_dec_tail", (1, 33), dict(LOOP, V=64, cand_sum=z(33, 2), with_logprob=True)),
    "tail_repack": ("debug_dec_tail", (2, 33), dict(x=z(33, 576), row_of_slot=perm(64), blk_live=[1, 1], blk_left=[32, 1], seen_stop=zi(64),
                                                    n_compactions=3)),
    "tail_load_ids": ("debug_dec_tail", (3, 33), dict(x=z(40, 576), row_ids=perm(33), ld=576, n_src=40)),
    "tail_load_last": ("debug_dec_tail", (3, 33), dict(x=z(40, 580), ld=580, n_src=40, T_last=1)),
    "prefill": ("debug_prefill_attn", (z(2, 64, 576), z(2, 3, 64, 64), z(2, 3, 64, 64), 64), dict()),
    "prefill_apb": ("debug_prefill_attn", (z(2, 64, 576), z(2, 3, 64, 64), z(2, 3, 64, 64), 64), dict(variant=1, out_form=1)),
    "prefill_past": ("debug_prefill_attn", (z(2, 32, 576), z(2, 3, 64, 64), z(2, 3, 64, 64), 64), dict(qpos0=32)),
    "prefill_past_apb": ("debug_prefill_attn", (z(2, 32, 576), z(2, 3, 64, 64), z(2, 3, 64, 64), 64), dict(variant=1, qpos0=32, out_form=1)),
    "window": ("debug_window_attn", (z(64, 288), z(4, 64, 64)), dict()),
    "window_mask_apb": ("debug_window_attn", (z(64, 288), z(4, 64, 64)), dict(mask=z(2, 64, 64), out_form=1)),
    "window_in16": ("debug_window_attn", (z(64, 288), z(4, 64, 64)), dict(in16=True)),
}

F32_EPS = C.c_float(1e-5).value      # the default eps as a descriptor's float field holds it
# results that recur: the state words of the tail tap, the outputs of the decode attention, of the q/k/v launches, of the lm_head
WORDS = {"seen_stop": ("int32", (96,)), "scalars": ("int32", (32,)), "n_seen": "int", "arrive": "int", "ticket": "int", "n_compactions": "int",
         "blk_left": ("int32", (64,)), "blk_live": ("int32", (64,)), "row_of_slot": ("int32", (96,))}
PAGES, PAGES16 = ("float32", (65, 3, 8, 64)), ("int16", (65, 3, 8, 64))
ATT = {"att": ("float32", (92160,)), "ml": ("float32", (9, 64, 2, 2)), "k": PAGES, "v": PAGES, "xnew": ("float32", (96, 576)), "gs": "int"}
OPROJ = {"xmid": ("float32", (36864,)), "x16": ("float32", (36864,)), "ssq": ("float32", (96, 40))}
QKV = {"pq": ("float32", (544, 960)), "ssq1": ("float32", (96, 8)), "xnew": ("float32", (96, 576)), "rope": ("float32", (128,)), "pos": "int"}
QKV2 = {"pq": ("float32", (544, 960)), "down": ("float32", (313344,)), "q": ("float32", (960, 1536))}
HEAD = {"logits": ("float32", (96, 64)), "cand_val": ("float32", (96, 2)), "cand_idx": ("int32", (96, 2)), "cand_sum": ("float32", (96, 2))}
X, TOK, REC = {"x": ("float32", (55296,))}, {"tokens": ("int32", (96,))}, {"record": ("int32", (64, 5)), "progress": "int"}
QKV_ROPE = {"q": ("float32", (36, 576)), "k": ("float32", (3, 3, 4, 64)), "v": ("float32", (3, 3, 4, 64))}
AMX = {"amx": ("uint8", (16384,)), "scales": ("uint8", (1024,))}
TIMED = (("float32", (4, 8)), ("float", "float"))
UNTIMED = (("float32", (4, 8)), "NoneType")

# id -> (the call as the library sees it, the result): "p" = an address; a tuple = the descriptor's fields in order
EXPECTED = {
    "gemm_f32": (("mellow_debug_gemm_f32", 16, "p", 4, 32, "p", 8, "p", 0, None), UNTIMED),
    "gemm_f32_timed": (("mellow_debug_gemm_f32", 0, "p", 4, 32, "p", 8, "p", 2, "p"), TIMED),
    "gemm_fp8": (("mellow_debug_gemm_fp8", "p", 4, 32, "p", 8, "p", 0, None), UNTIMED),
    "gemm_fp8_timed": (("mellow_debug_gemm_fp8", "p", 4, 32, "p", 8, "p", 3, "p"), TIMED),
    "epi_linear": (("mellow_debug_gemm_epi", (96, 0, 0, 33, 32, 6, 8, 0, 0, 0, 0, 0, 8, 1, 0, 0, 0, 0.0, 0.0, 0, 0, 1, 1, 0), "p", "p", None, None,
                    None, None, None, None, "p", 2080, None, 0, None, 0, None, 0, None, None, 0),
                   {"c": ("float32", (65, 8))}),
    "epi_linear_operands": (("mellow_debug_gemm_epi", (96, 0, 0, 33, 32, 6, 8, 1, 1, 1, 0, 0, 16, 1, 0, 0, 2, 64.0, 0.5, 0, 1, 1, 1, 0), "p", "p",
                             "p", "p", None, "p", None, None, "p", 4160, None, 0, None, 0, None, 0, None, None, 0),
                            {"c": ("float32", (65, 16))}),
    "epi_k17": (("mellow_debug_gemm_epi", (96, 17, 0, 33, 48, 64, 64, 0, 0, 2, 11, 12, 64, 1, 1, 1, 0, 0.0, 0.0, 4, 0, 1, 1, 0), "p", "p", None,
                 "p", "p", None, None, None, "p", 17408, "p", 49152, "p", 260, None, 0, None, None, 0),
                {"c": ("float32", (68, 64)), "c3": ("int32", (12288,)), "ssq": ("float32", (65, 1))}),
    "epi_k17_c3_only": (("mellow_debug_gemm_epi", (96, 17, 0, 33, 48, 64, 64, 2, 0, 0, 0, 0, 64, 0, 1, 0, 0, 0.0, 0.0, 0, 0, 1, 1, 0), "p", "p",
                         None, None, None, None, None, None, None, 0, "p", 49152, None, 0, None, 0, None, None, 0),
                        {"c3": ("int32", (12288,))}),
    "epi_swiglu": (("mellow_debug_gemm_epi", (96, 16, 1, 33, 32, 32, 16, 0, 0, 0, 0, 0, 16, 1, 0, 0, 0, 0.0, 0.0, 0, 0, 1, 1, 0), "p", "p", None,
                    None, None, None, None, None, "p", 4160, None, 0, None, 0, None, 0, None, None, 0),
                   {"c": ("float32", (65, 16))}),
    "epi_qkv_rope": (("mellow_debug_gemm_epi", (96, 0, 2, 4, 32, 960, 960, 0, 0, 0, 0, 0, 960, 1, 0, 0, 0, 0.0, 0.0, 0, 0, 2, 4, 0), "p", "p", None,
                      None, None, None, "p", "p", None, 0, None, 0, None, 0, "p", 82944, "p", "p", 9216), QKV_ROPE),
    "epi_qkv_own_tables": (("mellow_debug_gemm_epi", (96, 0, 2, 4, 32, 960, 960, 0, 0, 0, 0, 0, 960, 1, 0, 0, 0, 0.0, 0.0, 0, 0, 2, 4, 0), "p", "p",
                            None, None, None, None, None, None, None, 0, None, 0, None, 0, "p", 82944, "p", "p", 9216), QKV_ROPE),
    "epi_qkv_at": (("mellow_debug_gemm_epi", (96, 0, 2, 4, 32, 960, 960, 0, 0, 0, 0, 0, 960, 1, 0, 0, 0, 0.0, 0.0, 0, 0, 3, 4, 1), "p", "p", None,
                    None, None, None, None, None, None, 0, None, 0, None, 0, "p", 82944, "p", "p", 9216), QKV_ROPE),
    "norm_ln_0": (("mellow_debug_norm", 0, 0, "p", 33, 96, "p", "p", 1e-05, None, 0, 0, 0, "p", 24960, None, 0), {"y": ("float32", (65, 96))}),
    "norm_ln_1_map": (("mellow_debug_norm", 0, 1, "p", 33, 96, "p", "p", 1e-06, "p", 33, 0, 0, "p", 73728, None, 0), {"apb": ("int32", (18432,))}),
    "norm_ln_2": (("mellow_debug_norm", 0, 2, "p", 33, 96, "p", "p", 1e-05, None, 0, 0, 0, "p", 16384, "p", 1024), AMX),
    "norm_ln_0_map": (("mellow_debug_norm", 0, 0, "p", 33, 96, "p", "p", 1e-05, "p", 11, 0, 0, "p", 24960, None, 0), {"y": ("float32", (65, 96))}),
    "norm_rms_0": (("mellow_debug_norm", 2, 0, "p", 33, 96, "p", None, 0.25, None, 0, 0, 0, "p", 24960, None, 0), {"y": ("float32", (65, 96))}),
    "norm_rms_1": (("mellow_debug_norm", 2, 1, "p", 33, 96, "p", None, 1e-05, None, 0, 0, 0, "p", 73728, None, 0), {"apb": ("int32", (18432,))}),
    "norm_rms_2": (("mellow_debug_norm", 2, 2, "p", 33, 96, "p", None, 1e-05, None, 0, 0, 0, "p", 16384, "p", 1024), AMX),
    "norm_merge": (("mellow_debug_norm", 1, 0, "p", 1, 4, "p", "p", 1e-05, None, 0, 1, 2, "p", 2112, None, 0), {"y": ("float32", (33, 16))}),
    "norm_none_1": (("mellow_debug_norm", 3, 1, "p", 33, 96, None, None, 1e-05, None, 0, 0, 0, "p", 73728, None, 0), {"apb": ("int32", (18432,))}),
    "norm_none_2": (("mellow_debug_norm", 3, 2, "p", 33, 96, None, None, 1e-05, None, 0, 0, 0, "p", 16384, "p", 1024), AMX),
    "attn": (("mellow_debug_dec_attn", (44, 33, 64, 3, 8, 4, 2, 0, 0, 0, F32_EPS), "p", "p", "p", None, None, "p", "p", None, None, None, "p", "p",
              368640, "p", 9216, "p", "p", 399360, "p", 221184, None, 0, None, 0, None, 0), ATT),
    "attn_kv16_rope": (("mellow_debug_dec_attn", (44, 33, 64, 3, 8, 4, 2, 0, 1, 0, 0.5), "p", "p", "p", None, "p", "p", "p", None, None, None, "p",
                        "p", 368640, "p", 9216, "p", "p", 199680, "p", 221184, None, 0, None, 0, None, 0), dict(ATT, k=PAGES16, v=PAGES16)),
    "attn_fused": (("mellow_debug_dec_attn", (44, 33, 64, 3, 8, 4, 2, 1, 0, 0, F32_EPS), "p", None, "p", "p", None, "p", "p", None, None, None, "p",
                    "p", 368640, "p", 9216, "p", "p", 399360, "p", 221184, None, 0, None, 0, None, 0), ATT),
    "attn_fused_kv16_wo": (("mellow_debug_dec_attn", (44, 33, 64, 3, 8, 4, 2, 1, 1, 0, F32_EPS), "p", None, "p", "p", None, "p", "p", None, None,
                            "p", "p", "p", 368640, "p", 9216, "p", "p", 199680, "p", 221184, "p", 147456, "p", 147456, "p", 15360),
                           dict(ATT, k=PAGES16, v=PAGES16, **OPROJ)),
    "attn_wo": (("mellow_debug_dec_attn", (44, 33, 64, 3, 8, 4, 2, 0, 0, 0, F32_EPS), "p", "p", "p", None, None, "p", "p", None, None, "p", "p",
                 "p", 368640, "p", 9216, "p", "p", 399360, "p", 221184, "p", 147456, "p", 147456, "p", 15360), dict(ATT, **OPROJ)),
    "attn_wo_x3": (("mellow_debug_dec_attn", (44, 33, 64, 3, 8, 4, 2, 0, 0, 1, F32_EPS), "p", "p", "p", None, None, "p", "p", None, None, "p", "p",
                    "p", 368640, "p", 9216, "p", "p", 399360, "p", 221184, "p", 147456, "p", 442368, "p", 15360),
                   dict(ATT, **dict(OPROJ, x16=("int16", (2, 110592))))),
    "attn_blocks": (("mellow_debug_dec_attn", (44, 33, 64, 3, 8, 4, 2, 0, 0, 0, F32_EPS), "p", "p", "p", None, None, "p", "p", "p", "p", None, "p",
                     "p", 368640, "p", 9216, "p", "p", 399360, "p", 221184, None, 0, None, 0, None, 0), ATT),
    "gemv_0_first_tables": (("mellow_debug_dec_gemv", (44, 0, 0, 33, 0, 1, 1, 2, 8, 0, F32_EPS), "p", None, "p", None, None, None, 0, None, 0, None,
                             "p", "p", None, "p", 2088960, None, 0, "p", 3072, "p", 221184, "p", "p", None, 0, None, 0, None, 0, None, None, 0),
                            QKV),
    "gemv_0_first": (("mellow_debug_dec_gemv", (44, 0, 0, 33, 0, 1, 0, 2, 8, 0, 0.5), "p", None, "p", None, None, None, 0, None, 0, None, None,
                      None, None, "p", 2088960, None, 0, "p", 3072, "p", 221184, "p", "p", None, 0, None, 0, None, 0, None, None, 0), QKV),
    "gemv_0_later": (("mellow_debug_dec_gemv", (44, 0, 0, 33, 8, 0, 0, 0, 0, 0, F32_EPS), "p", None, "p", "p", None, None, 0, None, 0, None, None,
                      None, None, "p", 2088960, None, 0, "p", 3072, "p", 221184, "p", "p", None, 0, None, 0, None, 0, None, None, 0), QKV),
    "gemv_1": (("mellow_debug_dec_gemv", (44, 1, 0, 33, 0, 0, 0, 0, 0, 0, F32_EPS), "p", "p", None, None, None, "p", 147456, None, 0, "p", None,
                None, None, None, 0, None, 0, None, 0, None, 0, None, None, "p", 589824, None, 0, None, 0, None, None, 0),
               {"gu": ("float32", (147456,))}),
    "gemv_1_x3": (("mellow_debug_dec_gemv", (44, 1, 1, 33, 0, 0, 0, 0, 0, 0, F32_EPS), "p", "p", None, None, None, "p", 221184, None, 0, "p", None,
                   None, None, None, 0, None, 0, None, 0, None, 0, None, None, "p", 589824, "p", 884736, None, 0, None, None, 0),
                  {"gu": ("float32", (147456,)), "h3": ("int16", (442368,))}),
    "gemv_2": (("mellow_debug_dec_gemv", (44, 2, 0, 33, 0, 0, 0, 0, 0, 0, F32_EPS), "p", None, None, None, "p", None, 0, None, 0, None, None, None,
                None, None, 0, "p", 1253376, None, 0, None, 0, None, None, None, 0, None, 0, None, 0, None, None, 0),
               {"down": ("float32", (313344,))}),
    "gemv_3": (("mellow_debug_dec_gemv", (44, 3, 0, 33, 0, 0, 0, 0, 0, 0, F32_EPS), "p", "p", "p", None, "p", None, 0, None, 0, None, None, None,
                None, "p", 2088960, "p", 1253376, None, 0, None, 0, None, None, None, 0, None, 0, None, 0, None, "p", 5898240), QKV2),
    "gemv_3_x3": (("mellow_debug_dec_gemv", (44, 3, 1, 33, 0, 0, 0, 0, 0, 0, F32_EPS), "p", "p", None, None, None, "p", 221184, "p", 589824, None,
                   None, None, None, "p", 2088960, "p", 1253376, None, 0, None, 0, None, None, None, 0, None, 0, None, 0, None, "p", 5898240),
                  QKV2),
    "gemv_4": (("mellow_debug_dec_gemv", (44, 4, 0, 33, 8, 0, 0, 0, 0, 0, F32_EPS), "p", None, "p", "p", None, None, 0, None, 0, None, None, None,
                None, None, 0, None, 0, None, 0, None, 0, None, None, None, 0, None, 0, "p", 221184, None, None, 0),
               {"xn": ("float32", (55296,))}),
    "gemv_4_x3": (("mellow_debug_dec_gemv", (44, 4, 0, 33, 0, 0, 0, 0, 0, 1, F32_EPS), "p", None, "p", None, None, None, 0, None, 0, None, None,
                   None, None, None, 0, None, 0, None, 0, None, 0, None, None, None, 0, None, 0, "p", 331776, None, None, 0),
                  {"xn": ("int16", (165888,))}),
    "gemv_4_blocks": (("mellow_debug_dec_gemv", (44, 4, 0, 33, 0, 0, 0, 0, 0, 0, F32_EPS), "p", None, "p", None, None, None, 0, None, 0, None, None,
                       None, "p", None, 0, None, 0, None, 0, None, 0, None, None, None, 0, None, 0, "p", 221184, "p", None, 0),
                      {"xn": ("float32", (55296,)), "snap": ("int32", (64,))}),
    "tail_head": (("mellow_debug_dec_tail", (84, 0, 0, 33, 64, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), "p", "p", None, 0, None, None, None,
                   None, None, None, None, None, None, "p", 24576, "p", "p", "p", 768, None, 0, None, None, 0, None, 0, None, None, 0), HEAD),
    "tail_head_x3": (("mellow_debug_dec_tail", (84, 0, 1, 33, 64, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), "p", None, "p", 221184, "p", None,
                      None, None, None, None, None, None, None, "p", 24576, "p", "p", "p", 768, None, 0, None, None, 0, None, 0, None, None, 0),
                     HEAD),
    "tail_argmax": (("mellow_debug_dec_tail", (84, 1, 0, 33, 64, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), None, None, None, 0, None, "p", "p",
                     None, None, None, None, None, None, None, 0, None, None, None, 0, "p", 384, None, None, 0, None, 0, None, "p", 221184),
                    dict(X, **TOK)),
    "tail_argmax_state": (("mellow_debug_dec_tail", (84, 1, 0, 33, 64, 0, 0, 1, 1, 0, 5, 2, 7, 9, 1, 0, 3, 0, 0, 0, 0), "p", None, None, 0, "p", "p",
                           "p", None, "p", "p", "p", "p", None, None, 0, None, None, None, 0, "p", 384, "p", None, 1280, "p", 1408, "p", "p",
                           221184), dict(X, **TOK, **REC, **WORDS)),
    "tail_argmax_logprob": (("mellow_debug_dec_tail", (84, 1, 0, 33, 64, 0, 0, 0, 1, 1, 5, 2, 7, 9, 1, 0, 3, 0, 0, 0, 0), None, None, None, 0, None,
                             "p", "p", "p", "p", None, None, None, None, None, 0, None, None, None, 0, "p", 384, "p", "p", 1280, "p", 1408, "p",
                             "p", 221184), dict(X, **TOK, **REC, **WORDS, logprob=("float32", (64, 5)))),
    "tail_repack": (("mellow_debug_dec_tail", (84, 2, 0, 33, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0, 0), None, "p", None, 0, "p", None, None,
                     None, "p", "p", None, "p", None, None, 0, None, None, None, 0, None, 0, None, None, 0, "p", 1408, None, "p", 221184),
                    dict(X, **WORDS)),
    "tail_load_ids": (("mellow_debug_dec_tail", (84, 3, 0, 33, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 576, 40, 0), None, "p", None, 0, None, None,
                       None, None, None, None, None, None, "p", None, 0, None, None, None, 0, None, 0, None, None, 0, None, 0, None, "p", 221184),
                      X),
    "tail_load_last": (("mellow_debug_dec_tail", (84, 3, 0, 33, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 580, 40, 1), None, "p", None, 0, None, None,
                        None, None, None, None, None, None, None, None, 0, None, None, None, 0, None, 0, None, None, 0, None, 0, None, "p",
                        221184), X),
    "prefill": (("mellow_debug_prefill_attn", 0, "p", "p", "p", 2, 64, 64, 0, 0, "p", 368640), ("float32", (160, 576))),
    "prefill_apb": (("mellow_debug_prefill_attn", 1, "p", "p", "p", 2, 64, 64, 0, 1, "p", 442368), ("int32", (110592,))),
    "prefill_past": (("mellow_debug_prefill_attn", 0, "p", "p", "p", 2, 64, 64, 32, 0, "p", 221184), ("float32", (96, 576))),
    "prefill_past_apb": (("mellow_debug_prefill_attn", 1, "p", "p", "p", 2, 64, 64, 32, 1, "p", 442368), ("int32", (110592,))),
    "window": (("mellow_debug_window_attn", "p", 64, 96, 4, "p", None, 0, 0, 0, "p", 36864), ("float32", (96, 96))),
    "window_mask_apb": (("mellow_debug_window_attn", "p", 64, 96, 4, "p", "p", 2, 0, 1, "p", 73728), ("int32", (18432,))),
    "window_in16": (("mellow_debug_window_attn", "p", 64, 96, 4, "p", None, 0, 1, 0, "p", 36864), ("float32", (96, 96))),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_wrapper_hands_this_call_to_the_library_and_returns_these_tensors(case):
    method, args, kwargs = CASES[case]
    e = _engine()
    res = getattr(e, method)(*args, **kwargs)
    assert len(e.lib.calls) == 1
    call, returned = EXPECTED[case]
    assert e.lib.calls[0] == call
    assert _returned(res) == returned


def test_every_tap_symbol_is_reached():
    assert {c[0] for c, _ in EXPECTED.values()} == set(ARGS)
    assert set(EXPECTED) == set(CASES)


def test_a_wrong_shape_is_refused_before_the_library_is_called():
    e = _engine()
    with pytest.raises(ValueError, match=r"ssq1 \(33, 7\) is not \(33, 8\)"):
        e.debug_dec_attn(**dict(DA, ssq1=z(33, 7)))
    with pytest.raises(ValueError, match=r"W \(960, 575\) is not \(960, 576\)"):
        e.debug_dec_gemv(0, 33, z(960, 575), x=z(33, 576))
    with pytest.raises(ValueError, match=r"cand_idx \(33, 3\) is not \(33, 2\)"):
        e.debug_dec_tail(1, 33, V=64, cand_val=z(33, 2), cand_idx=zi(33, 3))
    with pytest.raises(ValueError, match="blk_live has 3 entries for 2"):
        e.debug_dec_attn(**dict(DA, blk_live=[1, 1, 1]))
    with pytest.raises(ValueError, match="w has 95 elements for 96 columns"):
        e.debug_norm(z(33, 96), w=z(95), b=z(96))
    with pytest.raises(ValueError, match="state has unknown keys"):
        e.debug_dec_tail(1, 33, V=64, cand_val=z(33, 2), cand_idx=zi(33, 2), state=dict(STATE, steps=1))
    assert e.lib.calls == []
