"""numpy transcription of the constrained decoding of include/mellow_hip.h (mellow_generate_constraint): the trie builder's inverse,
the state of a row after a history, the allowed set of a state and the effect on rows of fp32 logits.  The partials and the fp64
log-softmax are those of tests/logit_rules_ref.py.  Used by tests/test_constraint_cpu.py and tests/test_gpu_constraint.py; it shares
no code with the engine (it reads the arrays mellow_amd/constraint.py builds, which the CPU tests check against `phrases_of`)."""
import numpy as np

DEAD, FREE, DONE = -1, -2, -3


def edges(trie, u):
    """{token: child} of node u"""
    a, b = int(trie["node_first"][u]), int(trie["node_first"][u + 1])
    return {int(t): int(c) for t, c in zip(trie["edge_token"][a:b], trie["edge_child"][a:b])}


def terminal(trie, u):
    return bool(int(trie["node_flags"][u]) & 1)


def phrases_of(trie, root):
    """the builder's inverse: the sorted list of the phrases (tuples) that end at a terminal node below `root`"""
    out, stack = [], [(int(root), ())]
    while stack:
        u, pre = stack.pop()
        if terminal(trie, u):
            out.append(pre)
        for t, c in edges(trie, u).items():
            stack.append((c, pre + (t,)))
    return sorted(out)


def step(trie, u, t, stop_id=-1, then_free=False):
    """one transition of the definition"""
    if u < 0:
        return u                               # DEAD, FREE and DONE absorb
    c = edges(trie, u).get(int(t))
    if c is not None:                          # an edge wins over the stop rule
        return FREE if then_free and terminal(trie, c) else c
    if int(t) == stop_id and stop_id >= 0 and terminal(trie, u):
        return DONE
    return DEAD


def state_after(trie, root, history, stop_id=-1, then_free=False):
    u = int(root)
    for t in history:
        u = step(trie, u, t, stop_id, then_free)
    return u


def allowed(trie, u, stop_id=-1):
    """the allowed set of a state: a sorted list of token ids, or None for everything.  An empty list constrains nothing."""
    if u == FREE:
        return None
    if u in (DEAD, DONE):
        return [stop_id] if stop_id >= 0 else []
    s = set(edges(trie, u))
    if terminal(trie, u) and stop_id >= 0:
        s.add(stop_id)
    return sorted(s)


def apply_rows(logits, trie, roots, histories, stop_id=-1, then_free=False):
    """-> (processed float32 [B][V], states int32 [B], constrained bool [B]: rows the launch edits -- the others it does not touch)"""
    out = np.array(logits, dtype=np.float32, copy=True)
    states = np.zeros(out.shape[0], dtype=np.int32)
    con = np.zeros(out.shape[0], dtype=bool)
    for b in range(out.shape[0]):
        u = state_after(trie, roots[b], histories[b], stop_id, then_free)
        states[b] = u
        a = allowed(trie, u, stop_id)
        if a is None or len(a) == 0:
            continue
        con[b] = True
        keep = np.zeros(out.shape[1], dtype=bool)
        keep[a] = True
        out[b, ~keep] = -np.inf
    return out, states, con
