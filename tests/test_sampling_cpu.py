"""CPU: the seeded nucleus sampler's reference (tests/sampler_ref.py) against Random123's known answers and against a literal
transcription of the reference's top-p filter; the library exports the sampling entry points (ABI minor 4)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_ref as R  # noqa: E402


@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    got = R.philox4x32_10(*ctr, *key)
    assert tuple(int(w) for w in got) == want


def test_uniforms_in_open_unit_interval():
    u = R.uniforms(49152, seed=123456789012345, row=3, step=7)
    assert u.min() > 0.0 and u.max() < 1.0
    assert np.array_equal(np.float32(u).astype(np.float64), u)        # exact in fp32


def _reference_filter(logits, top_p):
    """reference wrapper.py:219-226, transcribed: sort, softmax, cumsum, shift right, mask (kept = not removed)"""
    sorted_logits, sorted_indices = torch.sort(logits, descending=True, stable=True)
    cumulative_probs = torch.cumsum(torch.softmax(sorted_logits, dim=-1), dim=-1)
    sorted_indices_to_remove = cumulative_probs > top_p
    sorted_indices_to_remove[..., 1:] = sorted_indices_to_remove[..., :-1].clone()
    sorted_indices_to_remove[..., 0] = 0
    remove = sorted_indices_to_remove.scatter(-1, sorted_indices, sorted_indices_to_remove)
    return ~remove


def test_nucleus_rule_matches_reference_filter():
    rng = np.random.default_rng(0)
    n_cmp = 0
    for r in range(40):
        V = 4096
        l = (rng.standard_normal(V) * rng.uniform(0.5, 6.0)).astype(np.float32)
        if r % 4 == 0:
            l = np.round(l)                   # heavy ties
        top_p = float(rng.choice([0.0, 0.1, 0.5, 0.8, 0.9, 0.95, 0.999]))
        kept, margin = R.nucleus_mask(R.scaled(l, 1.0), top_p)
        if margin < 1e-9:
            continue
        ref = _reference_filter(torch.from_numpy(l.astype(np.float64)), top_p).numpy()
        assert np.array_equal(kept, ref), (r, top_p, int(kept.sum()), int(ref.sum()))
        n_cmp += 1
    assert n_cmp >= 35


def test_reference_sampler_edges():
    l = np.array([0.0, 3.0, 3.0, 1.0, np.nan, np.nan], dtype=np.float32)
    assert R.sample_ref(l, 0.9, 1.0, 1, 0, 0)[0] == 4                  # first NaN
    l = np.array([0.0, 3.0, 3.0, 1.0], dtype=np.float32)
    for s in range(20):
        assert R.sample_ref(l, 0.0, 1.0, s, s, s)[0] == 1              # top_p = 0: the arg-max, lowest index on ties


def test_library_exports_sampling_entry_points():
    from mellow_amd import engine
    lib = engine.load_library()
    raw = ctypes.CDLL(lib._name)
    for sym in ("mellow_generate_sampled", "mellow_sample_logits"):
        assert sym in engine.EXPORTED_SYMBOLS
        getattr(raw, sym)
    assert lib.mellow_abi_minor() == 5            # the current minor (the sampling symbols are what minor 4 added)
