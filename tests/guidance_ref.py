"""numpy fp64 transcription of the contrastive guidance of include/mellow_hip.h (mellow_generate_guidance): per pair, with l_c / l_u the
logits of the conditional and the negative row and s the scale,
    lse_x = m_x + log(sum_v exp(l_x[v] - m_x)),  m_x = max_v l_x[v]
    a = l_c - lse_c;  b = l_u - lse_u;  g = b + s * (a - b)
Used by tests/test_guidance_cpu.py and tests/test_gpu_guidance.py; it shares no code with the engine."""
import numpy as np

TILE = 32


def logsumexp64(rows):
    l = np.asarray(rows, dtype=np.float64)
    m = l.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(l - m).sum(axis=-1, keepdims=True)))[..., 0]


def log_softmax64(rows):
    l = np.asarray(rows, dtype=np.float64)
    return l - logsumexp64(l)[..., None]


def guide(l_c, l_u, scale):
    """g in fp64 for one pair ([V], [V]) or a stack of pairs ([P][V], [P][V])"""
    a, b = log_softmax64(l_c), log_softmax64(l_u)
    return b + float(scale) * (a - b)


def guide_rows(rows, scale):
    """rows [2P][V], rows 2i / 2i + 1 the conditional / negative row of pair i -> g float64 [P][V]"""
    rows = np.asarray(rows)
    return guide(rows[0::2], rows[1::2], scale)


def bound(rows, scale):
    """per pair, the fp32 rounding bound of the formula: 4 * 2^-23 * (|s| + |s - 1|) * (max|l_c| + max|l_u| + |lse_c| + |lse_u| + 1)"""
    rows = np.asarray(rows, dtype=np.float64)
    c, u = rows[0::2], rows[1::2]
    s = float(scale)
    return 4 * 2.0 ** -23 * (abs(s) + abs(s - 1)) * (np.abs(c).max(-1) + np.abs(u).max(-1) + np.abs(logsumexp64(c)) + np.abs(logsumexp64(u)) + 1)


def first_argmax(row):
    """torch.argmax order on finite data: the lowest index among equals"""
    return int(np.argmax(np.asarray(row)))


def tile_partials(rows):
    """per 32-column tile of every (finite) row: (maximum [B][V / 32], its first index int32 [B][V / 32])"""
    rows = np.asarray(rows)
    B, V = rows.shape
    t = rows.reshape(B, V // TILE, TILE)
    idx = t.argmax(axis=2)
    val = np.take_along_axis(t, idx[:, :, None], axis=2)[:, :, 0]
    return val, (idx + np.arange(V // TILE)[None, :] * TILE).astype(np.int32)


def tile_sums64(rows):
    """per tile the fp64 sum of exp(l - tile maximum)"""
    rows = np.asarray(rows, dtype=np.float64)
    B, V = rows.shape
    t = rows.reshape(B, V // TILE, TILE)
    return np.exp(t - t.max(axis=2, keepdims=True)).sum(axis=2)
