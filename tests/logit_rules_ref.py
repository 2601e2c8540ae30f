"""numpy transcription of the repetition controls of include/mellow_hip.h (mellow_generate_rules): the four rules on one row of fp32
logits in float32 operations (what the kernel is asked to match bit for bit), the tile partials the greedy arg-max reads, and an fp64
log-softmax of the processed row.  Used by tests/test_logit_rules_cpu.py and tests/test_gpu_logit_rules.py; it shares no code with
the engine."""
import numpy as np

TILE = 32


def apply_row(logits, history, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, bias=None, stop_id=-1):
    """the processed row: logits float32 [V], history = the tokens h[0 .. s) the row has generated -> float32 [V]"""
    l = np.array(logits, dtype=np.float32, copy=True)
    h = [int(t) for t in history]
    s = len(h)
    theta = np.float32(repetition_penalty)
    n, m = int(no_repeat_ngram_size), int(min_new_tokens)
    with np.errstate(all="ignore"):
        # 1. once per distinct token of the history
        for v in sorted(set(h)):
            l[v] = l[v] * theta if l[v] < 0 else l[v] / theta
        # 2. the bias, shared by all rows
        if bias is not None:
            l = (l + np.asarray(bias, dtype=np.float32)).astype(np.float32)
    # 3. a token that would complete an n-gram the history already holds
    if n > 0 and s >= n - 1:
        tail = h[s - n + 1:]
        for i in range(0, s - n + 1):
            if h[i:i + n - 1] == tail:
                l[h[i + n - 1]] = -np.inf
    # 4. the stop id before the row holds min_new_tokens tokens
    if s < m and stop_id >= 0:
        l[stop_id] = -np.inf
    return l


def apply_rows(logits, histories, **kw):
    return np.stack([apply_row(l, h, **kw) for l, h in zip(np.asarray(logits), histories)])


def first_argmax(row):
    """torch.argmax order: a NaN is the maximum, the lowest index wins among equals"""
    row = np.asarray(row)
    nan = np.isnan(row)
    return int(np.argmax(nan)) if nan.any() else int(np.argmax(row))


def tile_partials(rows):
    """per 32-column tile of every processed row: (maximum float32 [B][V / 32], its first index int32 [B][V / 32])"""
    rows = np.asarray(rows, dtype=np.float32)
    B, V = rows.shape
    t = rows.reshape(B, V // TILE, TILE)
    nan = np.isnan(t)
    idx = np.where(nan.any(axis=2), nan.argmax(axis=2), np.where(nan, -np.inf, t).argmax(axis=2)).astype(np.int64)      # (first_argmax per tile)
    val = np.take_along_axis(t, idx[:, :, None], axis=2)[:, :, 0]
    return val, (idx + np.arange(V // TILE)[None, :] * TILE).astype(np.int32)


def logsumexp64(rows):
    l = np.asarray(rows, dtype=np.float64)
    m = l.max(axis=-1, keepdims=True)
    with np.errstate(all="ignore"):
        return (m + np.log(np.exp(l - m).sum(axis=-1, keepdims=True)))[..., 0]


def log_softmax64(rows):
    """fp64 log-softmax of processed rows; a banned token (-inf) has log-prob -inf"""
    l = np.asarray(rows, dtype=np.float64)
    with np.errstate(all="ignore"):
        return l - logsumexp64(l)[..., None]


def merged_lse(cand_val, cand_sum):
    """the log-sum-exp a step merges from the tile partials, in fp64: M + log sum_t s_t exp(m_t - M), a tile whose maximum is -inf
    contributing nothing"""
    m = np.asarray(cand_val, dtype=np.float64)
    s = np.asarray(cand_sum, dtype=np.float64)
    M = m.max(axis=-1, keepdims=True)
    with np.errstate(all="ignore"):
        w = np.where(np.isneginf(m), 0.0, s * np.exp(m - M))
    return (M + np.log(w.sum(axis=-1, keepdims=True)))[..., 0]
