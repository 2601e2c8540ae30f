"""Stop strings, host side: the byte string of every token of a vocabulary, as the table of include/mellow_hip.h
(mellow_set_vocab_bytes), and the cut of a decoded text at the first stop string.

The device matches the stop strings of a `generate(stop_strings=...)` call on the BYTES of the generated tokens, inside the decode
step (mellow_amd/csrc/stop_strings.hip).  This module only builds the table and cuts texts; it needs no GPU and no library.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

MAX_TOKEN_BYTES = 256          # bytes of one token the table takes


def _gpt2_bytes_to_unicode() -> dict:
    """The GPT-2 byte-to-unicode alphabet: byte -> the printable character a byte-level BPE vocabulary writes it as.  The 188 bytes
    that are printable and no space in Latin-1 stand for themselves; the other 68 take the code points from 256 on, in byte order."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    table, n = {}, 0
    for b in range(256):
        if b in keep:
            table[b] = chr(b)
        else:
            table[b] = chr(256 + n)
            n += 1
    return table


BYTE_TO_UNICODE = _gpt2_bytes_to_unicode()                      # 256 entries: 0x20 -> "Ġ", 0x0A -> "Ċ", ...
UNICODE_TO_BYTE = {c: b for b, c in BYTE_TO_UNICODE.items()}
assert len(UNICODE_TO_BYTE) == 256 and BYTE_TO_UNICODE[0x20] == "Ġ" and BYTE_TO_UNICODE[0x0A] == "Ċ"


def token_bytes(token: str) -> bytes:
    """a token string of a byte-level BPE vocabulary -> its bytes: through the inverse alphabet where every character is in it,
    else (a special token written outside the alphabet) the string's UTF-8"""
    if all(c in UNICODE_TO_BYTE for c in token):
        return bytes(UNICODE_TO_BYTE[c] for c in token)
    return token.encode("utf-8")


def vocab_bytes(tokenizer, V: int) -> Tuple[np.ndarray, np.ndarray]:
    """-> (offsets int32 [V + 1], bytes uint8 [offsets[V]]): token i is bytes[offsets[i] : offsets[i + 1]].
    A tokenizer with `convert_ids_to_tokens` gives its token strings, taken back to bytes by token_bytes; any other is asked for
    `decode([i]).encode("utf-8")`.  Ids beyond the tokenizer's size (the padding rows of an embedding) are empty.  ValueError for a
    token of more than 256 bytes, the most the device table holds."""
    V = int(V)
    try:
        size = len(tokenizer)
    except TypeError:
        size = int(getattr(tokenizer, "vocab_size", V))
    size = min(int(size), V)
    parts: List[bytes] = []
    if hasattr(tokenizer, "convert_ids_to_tokens"):
        for i in range(size):
            t = tokenizer.convert_ids_to_tokens(i)
            parts.append(b"" if t is None else token_bytes(str(t)))
    else:
        for i in range(size):
            parts.append(tokenizer.decode([i]).encode("utf-8"))
    for i, b in enumerate(parts):
        if len(b) > MAX_TOKEN_BYTES:
            raise ValueError(f"vocabulary token {i} has {len(b)} bytes: stop strings take tokens of at most {MAX_TOKEN_BYTES} bytes")
    offsets = np.zeros(V + 1, dtype=np.int32)
    offsets[1:size + 1] = np.cumsum([len(b) for b in parts], dtype=np.int64)
    offsets[size + 1:] = offsets[size]
    return offsets, np.frombuffer(b"".join(parts), dtype=np.uint8).copy()


def cut_text(text: str, strings: Sequence[str], include: bool = False) -> Tuple[str, Optional[str]]:
    """Cut `text` at its first stop string: among all occurrences of all strings the one that ENDS first (where the device's match
    completes), on equal end the one that starts first.  The text is cut at the start of that occurrence, with `include` at its end.
    -> (text, the matched string or None)"""
    best = None
    for s in strings:
        i = text.find(s) if s else -1
        if i >= 0 and (best is None or (i + len(s), i) < (best[0], best[1])):
            best = (i + len(s), i, s)
    if best is None:
        return text, None
    return text[:best[0] if include else best[1]], best[2]


def stop_strings_digest(strings: Sequence[bytes]) -> str:
    """a digest of the stop strings of a call (what data-parallel ranks compare: the strings are per call and the same on every rank)"""
    import hashlib
    return hashlib.sha1(repr([bytes(b) for b in strings]).encode()).hexdigest()
