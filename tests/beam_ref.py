"""numpy fp64 transcription of the beam search of include/mellow_hip.h (mellow_generate_beam): one selection step and the whole
search given a logits callback.  Used by tests/test_beam_cpu.py and tests/test_gpu_beam.py; it shares no code with the engine."""
import numpy as np


def log_softmax64(logits):
    l = np.asarray(logits, dtype=np.float64)
    m = l.max(axis=-1, keepdims=True)
    return l - (m + np.log(np.exp(l - m).sum(axis=-1, keepdims=True)))


def candidates(logits, cum, fin, k, stop_id):
    """every candidate of every example: list (one per example) of arrays [n][4] = (c, parent, token, lp), sorted in the order of
    the definition: c descending, parent ascending, token ascending"""
    logits = np.asarray(logits)
    cum = np.asarray(cum, dtype=np.float64)
    fin = np.asarray(fin)
    N, V = logits.shape
    out = []
    for b in range(N // k):
        rows = []
        for j in range(k):
            r = b * k + j
            if fin[r]:
                rows.append(np.array([[cum[r], j, stop_id, 0.0]]))
            else:
                lp = log_softmax64(logits[r])
                rows.append(np.stack([cum[r] + lp, np.full(V, float(j)), np.arange(V, dtype=np.float64), lp], axis=1))
        c = np.concatenate(rows, axis=0)
        order = np.lexsort((c[:, 2], c[:, 1], -c[:, 0]))
        out.append(c[order])
    return out


def select_step(logits, cum, fin, k, stop_id):
    """one selection: -> parent int [N], token int [N], cum float64 [N], lp float64 [N], and per example the gaps between
    consecutive DISTINCT candidate values among its best k + 1 (what decides whether fp32 arithmetic can change the choice)"""
    cands = candidates(logits, cum, fin, k, stop_id)
    N = np.asarray(logits).shape[0]
    parent, token = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    ncum, lp = np.zeros(N), np.zeros(N)
    gaps = []
    for b, c in enumerate(cands):
        top = c[:k]
        parent[b * k:(b + 1) * k] = top[:, 1].astype(np.int64)
        token[b * k:(b + 1) * k] = top[:, 2].astype(np.int64)
        ncum[b * k:(b + 1) * k] = top[:, 0]
        lp[b * k:(b + 1) * k] = top[:, 3]
        v = c[:k + 1, 0]
        d = -np.diff(v)
        d = d[np.isfinite(d) & (d > 0)]                # equal values are decided by (parent, token): no gap to cross
        gaps.append(float(d.min()) if d.size else np.inf)
    return parent, token, ncum, lp, gaps


def search(logits_fn, B, k, max_len, stop_id):
    """the whole search: logits_fn(step, sequences) -> logits [N][V] of the next token of every row, sequences = list of N token
    lists (the rows' histories).  -> dict of tables parent / token / lp [steps][N], cum [N], steps"""
    N = B * k
    cum = np.where(np.arange(N) % k == 0, 0.0, -np.inf)
    fin = np.zeros(N, dtype=np.int64)
    seqs = [[] for _ in range(N)]
    P, T, L = [], [], []
    for s in range(max_len):
        parent, token, cum, lp, _ = select_step(logits_fn(s, seqs), cum, fin, k, stop_id)
        seqs = [seqs[r // k * k + parent[r]] + [int(token[r])] for r in range(N)]
        fin = (token == stop_id).astype(np.int64)
        P.append(parent); T.append(token); L.append(lp)
        if fin.all():
            break
    return {"parent": np.stack(P), "token": np.stack(T), "lp": np.stack(L), "cum": cum, "steps": len(P)}
