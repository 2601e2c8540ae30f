"""CPU: the C-ABI library loads, exports every symbol declared in include/mellow_hip.h, and its host-only
helpers (window permutation, weight fragment packing) agree with the reference's torch ops.
No compute call is made: there is no GPU here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from mellow_amd import engine as E
from oracle import mellow_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(E.LIB_PATH):
        from mellow_amd.csrc import build
        build.build()
    return E.load_library()


def test_library_exports_every_declared_symbol(lib):
    hdr = open(os.path.join(ROOT, "include", "mellow_hip.h")).read()
    declared = set(re.findall(r"\b(mellow_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"mellow_config", "mellow_engine"}
    assert declared == set(E.EXPORTED_SYMBOLS), declared ^ set(E.EXPORTED_SYMBOLS)
    raw = ctypes.CDLL(E.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
    assert lib.mellow_abi_version() == E.ABI_VERSION


def test_attention_taps_are_declared_bound_and_came_with_minor_5(lib):
    hdr = open(os.path.join(ROOT, "include", "mellow_hip.h")).read()
    assert lib.mellow_abi_minor() == 5 and re.search(r"#define MELLOW_ABI_MINOR 5\b", hdr)
    for name in ("mellow_debug_prefill_attn", "mellow_debug_window_attn"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in E.EXPORTED_SYMBOLS and name in E._ADDED_UNDER_MINOR_5
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 12 and fn.argtypes[-1] is ctypes.c_int64
        # host code only: a null engine is refused before any device is touched
        assert fn(*[None if t is ctypes.c_void_p else t(1) for t in fn.argtypes]) != 0
        assert "null argument" in lib.mellow_last_error().decode()
    # a library that predates them still loads; the Engine methods then say what is missing
    e = object.__new__(E.Engine)
    e.lib, e.h = type("OldLib", (), {})(), None
    for call in (lambda: e.debug_prefill_attn(None, None, None, 1), lambda: e.debug_window_attn(None, None)):
        with pytest.raises(E.EngineError, match="predates mellow_debug_"):
            call()


def test_gemm_epilogue_tap_is_declared_bound_and_refuses_without_a_device(lib):
    hdr = open(os.path.join(ROOT, "include", "mellow_hip.h")).read()
    name = "mellow_debug_gemm_epi"
    assert re.search(r"\bint\s+%s\s*\(" % name, hdr) and re.search(r"\}\s*mellow_gemm_epi_t;", hdr)
    assert name in E.EXPORTED_SYMBOLS and name in E._ADDED_UNDER_MINOR_5
    fn = getattr(lib, name)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 21
    # the descriptor of the binding is the header's: one 4-byte field per declared member, in the header's order
    body = re.search(r"typedef struct mellow_gemm_epi \{(.*?)\} mellow_gemm_epi_t;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [(t, n.strip()) for t, names in re.findall(r"\b(int32_t|float)\s+([^;]+);", body) for n in names.split(",")]
    assert [n for _, n in members] == [n for n, _ in E.GemmEpi._fields_]
    assert all((ct is ctypes.c_float) == (t == "float") for (t, _), (_, ct) in zip(members, E.GemmEpi._fields_))
    assert ctypes.sizeof(E.GemmEpi) == 4 * len(members)
    # host code only: a null engine is refused before any device is touched
    assert fn(*[None if (t is ctypes.c_void_p or hasattr(t, "contents")) else t(1) for t in fn.argtypes]) != 0
    assert "null argument" in lib.mellow_last_error().decode()
    e = object.__new__(E.Engine)
    e.lib, e.h = type("OldLib", (), {})(), None
    with pytest.raises(E.EngineError, match="predates mellow_debug_gemm_epi"):
        e.debug_gemm_epi(None, None)


def test_norm_tap_is_declared_bound_and_refuses_without_a_device(lib):
    hdr = open(os.path.join(ROOT, "include", "mellow_hip.h")).read()
    name = "mellow_debug_norm"
    assert re.search(r"\bint\s+%s\s*\(" % name, hdr)
    assert name in E.EXPORTED_SYMBOLS and name in E._ADDED_UNDER_MINOR_5
    assert lib.mellow_abi_minor() == 5          # added under the current minor: found by symbol lookup, not by the number
    fn = getattr(lib, name)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 17 and fn.argtypes[-1] is ctypes.c_int64 and fn.argtypes[8] is ctypes.c_float
    # the binding's argument list is the header's: one entry per declared parameter, pointers as pointers
    decl = re.search(r"int\s+%s\s*\((.*?)\);" % name, hdr, re.S).group(1)
    params = [a.strip() for a in decl.split(",")]
    assert len(params) == len(fn.argtypes)
    for a, t in zip(params, fn.argtypes):
        want = ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float") else ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_int
        assert t is want, (a, t)
    # host code only: a null engine is refused before any device is touched
    assert fn(*[None if t is ctypes.c_void_p else t(1) for t in fn.argtypes]) != 0
    assert "null argument" in lib.mellow_last_error().decode()
    e = object.__new__(E.Engine)
    e.lib, e.h = type("OldLib", (), {})(), None
    with pytest.raises(E.EngineError, match="predates mellow_debug_norm"):
        e.debug_norm(torch.zeros(4, 96))


def test_decode_attention_tap_is_declared_bound_and_refuses_without_a_device(lib):
    hdr = open(os.path.join(ROOT, "include", "mellow_hip.h")).read()
    name = "mellow_debug_dec_attn"
    assert re.search(r"\bint\s+%s\s*\(" % name, hdr) and re.search(r"\}\s*mellow_dec_attn_t;", hdr)
    assert name in E.EXPORTED_SYMBOLS and name in E._ADDED_UNDER_MINOR_5
    assert lib.mellow_abi_minor() == 5          # added under the current minor: found by symbol lookup, not by the number
    fn = getattr(lib, name)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 28 and fn.argtypes[-1] is ctypes.c_int64
    # the binding's argument list is the header's: one entry per declared parameter, pointers as pointers (the descriptor typed)
    decl = re.search(r"int\s+%s\s*\((.*?)\);" % name, hdr, re.S).group(1)
    params = [a.strip() for a in decl.split(",")]
    assert len(params) == len(fn.argtypes)
    for a, t in zip(params, fn.argtypes):
        if "mellow_dec_attn_t*" in a:
            assert t._type_ is E.DecAttn, (a, t)
            continue
        want = ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float") else ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_int
        assert t is want, (a, t)
    # the descriptor of the binding is the header's: one 4-byte field per declared member, in the header's order
    body = re.search(r"typedef struct mellow_dec_attn \{(.*?)\} mellow_dec_attn_t;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [(t, n.strip()) for t, names in re.findall(r"\b(int32_t|float)\s+([^;]+);", body) for n in names.split(",")]
    assert members[0] == ("int32_t", "size")
    assert [n for _, n in members] == [n for n, _ in E.DecAttn._fields_]
    assert all((ct is ctypes.c_float) == (t == "float") for (t, _), (_, ct) in zip(members, E.DecAttn._fields_))
    assert ctypes.sizeof(E.DecAttn) == 4 * len(members)
    # host code only: a null engine is refused before any device is touched
    assert fn(*[None if (t is ctypes.c_void_p or hasattr(t, "contents")) else t(1) for t in fn.argtypes]) != 0
    assert "null argument" in lib.mellow_last_error().decode()
    e = object.__new__(E.Engine)
    e.lib, e.h = type("OldLib", (), {})(), None
    with pytest.raises(E.EngineError, match="predates mellow_debug_dec_attn"):
        e.debug_dec_attn(None, None, None, None, 1, 2, 2)


def test_decode_gemv_tap_is_declared_bound_and_refuses_without_a_device(lib):
    hdr = open(os.path.join(ROOT, "include", "mellow_hip.h")).read()
    name = "mellow_debug_dec_gemv"
    assert re.search(r"\bint\s+%s\s*\(" % name, hdr) and re.search(r"\}\s*mellow_dec_gemv_t;", hdr)
    assert name in E.EXPORTED_SYMBOLS and name in E._ADDED_UNDER_MINOR_5
    assert lib.mellow_abi_minor() == 5          # added under the current minor: found by symbol lookup, not by the number
    fn = getattr(lib, name)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 34 and fn.argtypes[-1] is ctypes.c_int64
    # the binding's argument list is the header's: one entry per declared parameter, pointers as pointers (the descriptor typed)
    decl = re.search(r"int\s+%s\s*\((.*?)\);" % name, hdr, re.S).group(1)
    params = [a.strip() for a in decl.split(",")]
    assert len(params) == len(fn.argtypes)
    for a, t in zip(params, fn.argtypes):
        if "mellow_dec_gemv_t*" in a:
            assert t._type_ is E.DecGemv, (a, t)
            continue
        want = ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float") else ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_int
        assert t is want, (a, t)
    # the descriptor of the binding is the header's: one 4-byte field per declared member, in the header's order
    body = re.search(r"typedef struct mellow_dec_gemv \{(.*?)\} mellow_dec_gemv_t;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [(t, n.strip()) for t, names in re.findall(r"\b(int32_t|float)\s+([^;]+);", body) for n in names.split(",")]
    assert members[0] == ("int32_t", "size")
    assert [n for _, n in members] == [n for n, _ in E.DecGemv._fields_]
    assert all((ct is ctypes.c_float) == (t == "float") for (t, _), (_, ct) in zip(members, E.DecGemv._fields_))
    assert ctypes.sizeof(E.DecGemv) == 4 * len(members)
    # host code only: a null engine is refused before any device is touched
    assert fn(*[None if (t is ctypes.c_void_p or hasattr(t, "contents")) else t(1) for t in fn.argtypes]) != 0
    assert "null argument" in lib.mellow_last_error().decode()
    e = object.__new__(E.Engine)
    e.lib, e.h = type("OldLib", (), {})(), None
    with pytest.raises(E.EngineError, match="predates mellow_debug_dec_gemv"):
        e.debug_dec_gemv(0, 1, None)


def test_decode_tail_tap_is_declared_bound_and_refuses_without_a_device(lib):
    hdr = open(os.path.join(ROOT, "include", "mellow_hip.h")).read()
    name = "mellow_debug_dec_tail"
    assert re.search(r"\bint\s+%s\s*\(" % name, hdr) and re.search(r"\}\s*mellow_dec_tail_t;", hdr)
    assert name in E.EXPORTED_SYMBOLS and name in E._ADDED_UNDER_MINOR_5
    assert lib.mellow_abi_minor() == 5          # added under the current minor: found by symbol lookup, not by the number
    fn = getattr(lib, name)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 31 and fn.argtypes[-1] is ctypes.c_int64
    # the binding's argument list is the header's: one entry per declared parameter, pointers as pointers (the descriptor typed)
    decl = re.search(r"int\s+%s\s*\((.*?)\);" % name, hdr, re.S).group(1)
    params = [a.strip() for a in decl.split(",")]
    assert len(params) == len(fn.argtypes)
    for a, t in zip(params, fn.argtypes):
        if "mellow_dec_tail_t*" in a:
            assert t._type_ is E.DecTail, (a, t)
            continue
        want = ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float") else ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_int
        assert t is want, (a, t)
    # the descriptor of the binding is the header's: one 4-byte field per declared member, in the header's order
    body = re.search(r"typedef struct mellow_dec_tail \{(.*?)\} mellow_dec_tail_t;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [(t, n.strip()) for t, names in re.findall(r"\b(int32_t|float)\s+([^;]+);", body) for n in names.split(",")]
    assert members[0] == ("int32_t", "size")
    assert [n for _, n in members] == [n for n, _ in E.DecTail._fields_]
    assert all((ct is ctypes.c_float) == (t == "float") for (t, _), (_, ct) in zip(members, E.DecTail._fields_))
    assert ctypes.sizeof(E.DecTail) == 4 * len(members)
    # host code only: a null engine is refused before any device is touched
    assert fn(*[None if (t is ctypes.c_void_p or hasattr(t, "contents")) else t(1) for t in fn.argtypes]) != 0
    assert "null argument" in lib.mellow_last_error().decode()
    e = object.__new__(E.Engine)
    e.lib, e.h = type("OldLib", (), {})(), None
    with pytest.raises(E.EngineError, match="predates mellow_debug_dec_tail"):
        e.debug_dec_tail(0, 1)


def test_required_keys_are_the_reference_state_dict_keys(lib):
    from mellow_amd import spec
    layout = spec.state_dict_layout()
    n = lib.mellow_engine_num_required()
    keys = [lib.mellow_engine_required_key(i).decode() for i in range(n)]
    assert len(set(keys)) == n
    assert set(keys) <= set(layout)
    unused = set(layout) - set(keys)
    assert unused == set(spec.UNUSED_KEYS) | {spec.LM + "lm_head.weight"}, unused


def test_engine_create_fails_loudly_without_gpu(lib):
    if lib.mellow_device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(E.EngineError, match="no HIP device"):
        E.Engine()


@pytest.mark.parametrize("name", ["mellow_generate", "mellow_generate_sampled", "mellow_generate_scored", "mellow_generate_n"])
def test_every_generate_entry_point_refuses_a_null_engine(lib, name):
    """the four doors share one argument check (engine_generate.cpp): host code only, no device is touched"""
    fn = getattr(lib, name)
    args = [None if t is ctypes.c_void_p or hasattr(t, "contents") else t(1) for t in fn.argtypes]
    assert fn(*args) != 0
    assert "engine not finalized" in lib.mellow_last_error().decode()


@pytest.mark.parametrize("R,shift", [(64, 0), (64, 4), (32, 4), (16, 0), (16, 4), (8, 0)])
def test_window_map_is_roll_plus_partition(lib, R, shift):
    """row m of the window-ordered batch must be token map[m] (reference htsat.py:427-436)."""
    m = E.host_window_map(R, shift)
    tok = torch.arange(R * R, dtype=torch.float32).view(1, R, R, 1)
    x = torch.roll(tok, shifts=(-shift, -shift), dims=(1, 2)) if shift else tok
    ws = min(R, 8)
    ref = O.window_partition(x, ws).reshape(-1).to(torch.int64).numpy()
    assert np.array_equal(m, ref)
    # the same map scatters back: window_reverse + roll(+shift) is the inverse permutation
    y = torch.zeros(R * R)
    y[torch.from_numpy(m).long()] = torch.arange(R * R, dtype=torch.float32)
    back = O.window_reverse(torch.arange(R * R, dtype=torch.float32).view(-1, ws, ws, 1), ws, R, R)
    back = torch.roll(back, shifts=(shift, shift), dims=(1, 2)) if shift else back
    assert torch.equal(y, back.reshape(-1))


def test_pack_weight_fragment_order(lib):
    rng = np.random.default_rng(0)
    N, K = 70, 52
    w = rng.standard_normal((N, K)).astype(np.float32)
    p = E.host_pack_weight(w, npad=128)
    assert p.shape == (4, 8, 64, 4)
    for nt, k8, lane, j in [(0, 0, 0, 0), (1, 3, 37, 2), (2, 6, 5, 3), (2, 6, 63, 3), (0, 7, 40, 1), (3, 0, 0, 0)]:
        n, k = nt * 32 + (lane & 31), k8 * 8 + 4 * (lane >> 5) + j
        want = w[n, k] if (n < N and k < K) else 0.0
        assert p[nt, k8, lane, j] == want
    # mfma k-pairing: the 4 MFMAs of one float4 cover k0+j and k0+4+j -> all 8 k of the tile exactly once
    ks = sorted(k8 * 8 + 4 * h + j for k8 in range(1) for h in range(2) for j in range(4))
    assert ks == list(range(8))


def test_rope_tables_helper_against_the_hf_computation(lib):
    """`mellow_host_rope_tables` is what the engine uses when the binding does not load "mellow.rope_cos/sin"
    (include/mellow_hip.h): same fp32 inv_freq / angle as transformers' LlamaRotaryEmbedding, cos / sin correctly rounded.
    torch's vectorised fp32 cos / sin are allowed to differ from that by one unit in the last place, nothing more."""
    P, D, theta = 2048, 64, 100000.0
    c = np.empty((P, D // 2), dtype=np.float32)
    s = np.empty((P, D // 2), dtype=np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    assert lib.mellow_host_rope_tables(theta, D, P, c.ctypes.data_as(fp), s.ctypes.data_as(fp)) == 0
    hc, hs = E.hf_rope_tables(P, D, theta)
    # the angle path is bit-identical: position 1 holds cos / sin of inv_freq itself, and exact identities hold at position 0
    assert np.array_equal(c[0], np.ones(D // 2, dtype=np.float32)) and np.array_equal(s[0], np.zeros(D // 2, dtype=np.float32))
    for got, ref in ((c, hc), (s, hs)):
        ulp = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, ulp.max()
        assert (ulp != 0).mean() < 0.10
    # and against float64: the helper is the correctly rounded value
    inv = (1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.int64).float() / D))).numpy()
    ang = (np.arange(P, dtype=np.float32)[:, None] * inv[None, :]).astype(np.float32).astype(np.float64)
    assert np.array_equal(c, np.cos(ang).astype(np.float32)) and np.array_equal(s, np.sin(ang).astype(np.float32))
    assert lib.mellow_host_rope_tables(theta, 63, P, c.ctypes.data_as(fp), s.ctypes.data_as(fp)) != 0
