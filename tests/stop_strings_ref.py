"""The stop strings of include/mellow_hip.h (mellow_generate_stop_strings) in numpy and plain Python: a transcription of the
definition, not of the kernel.  The yardstick of tests/test_stop_strings_cpu.py and tests/test_gpu_stop_strings.py.

A byte table is (offsets [V + 1], bytes): token i is bytes[offsets[i] : offsets[i + 1]]; an id outside [0, V) has no bytes."""
import numpy as np

import logit_rules_ref as LR

TAIL = 63                      # bytes of text the incremental form keeps: the longest string less one


def tok_bytes(table, t) -> bytes:
    off, data = table
    t = int(t)
    if not 0 <= t < len(off) - 1:
        return b""
    return bytes(bytearray(data[int(off[t]):int(off[t + 1])]))


def text_of(table, history) -> bytes:
    """X(s): the bytes of the generated tokens, back to back"""
    return b"".join(tok_bytes(table, t) for t in history)


def hit_brute(table, history, strings) -> bool:
    """the definition: some stop string is a substring of the whole text"""
    x = text_of(table, history)
    return any(x.find(bytes(s)) >= 0 for s in strings)


def advance(state, token_bytes: bytes, strings):
    """one step of the incremental form: state = (hit, tail) -> the state after one more token"""
    hit, tail = state
    if hit:
        return state                       # sticky
    x = tail + token_bytes
    return any(x.find(bytes(s)) >= 0 for s in strings), x[-TAIL:] if len(x) > TAIL else x


def hit_incremental(table, history, strings) -> bool:
    state = (False, b"")
    for t in history:
        state = advance(state, tok_bytes(table, t), strings)
    return bool(state[0])


def first_hit_step(table, history, strings):
    """the number of tokens after which the text first holds a stop string, or None"""
    for s in range(1, len(history) + 1):
        if hit_brute(table, history[:s], strings):
            return s
    return None


def one_hot_row(V: int, stop_id: int) -> np.ndarray:
    row = np.full(V, -np.inf, dtype=np.float32)
    row[int(stop_id)] = 0.0
    return row


def apply_rows(logits, table, histories, strings, stop_id):
    """-> (processed rows float32 [B][V], hit bool [B]): a hit row is the one-hot row of the stop id, any other is untouched"""
    out = np.array(logits, dtype=np.float32, copy=True)
    hit = np.array([hit_brute(table, h, strings) for h in histories], dtype=bool)
    for b in np.nonzero(hit)[0]:
        out[b] = one_hot_row(out.shape[1], stop_id)
    return out, hit


def hit_partials(V: int, stop_id: int):
    """the tile partials of a hit row: (cand_val, cand_idx, cand_sum), each [V / 32]"""
    row = one_hot_row(V, stop_id)[None]
    val, idx = LR.tile_partials(row)
    s = np.where(np.isneginf(val), 0.0, 1.0).astype(np.float32)
    return val[0], idx[0], s[0]
