"""Constrained decoding, host side: the phrase sets of a `generate(choices=...)` call as the trie arena of
include/mellow_hip.h (mellow_generate_constraint).

A constraint holds every answer to a set of phrases (token-id sequences).  The device walks a trie of the phrases by one transition
per generated token and bans, inside the decode step, every token that does not continue a phrase (mellow_amd/csrc/constrain.hip).
This module only builds the arrays; it needs no GPU and no library:

    node_first [n_nodes + 1]   offsets into the edge arrays (the edges of node u are node_first[u] .. node_first[u + 1])
    node_flags [n_nodes]       bit 0 = terminal: a phrase ends at this node
    edge_token, edge_child [n_edges]   the edges of a node sorted by token, strictly ascending; every child > its parent
    row_root [rows]            the root node of every row; rows with equal phrase sets share one root, and a root is never terminal
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

VOCAB = 49152                  # the vocabulary the constraint kernel is built for
MAX_COUNT = 1 << 20            # nodes, edges and rows one constraint takes
DEAD, FREE, DONE = -1, -2, -3  # the states of a row that are no node


def check_constraint(phrases_per_row, vocab: int = VOCAB) -> List[Tuple[Tuple[int, ...], ...]]:
    """The value rules of a constraint, in host code: per row a non-empty set of non-empty phrases of token ids in [0, vocab).
    -> per row the sorted tuple of its DISTINCT phrases (duplicates merged)."""
    if phrases_per_row is None or isinstance(phrases_per_row, (str, bytes)) or len(phrases_per_row) == 0:
        raise ValueError("a constraint needs a phrase set per row (got none)")
    out, memo = [], {}
    for r, phrases in enumerate(phrases_per_row):
        if id(phrases) in memo:          # the same list object given for many rows is checked once
            out.append(memo[id(phrases)])
            continue
        if isinstance(phrases, (str, bytes)) or phrases is None or len(phrases) == 0:
            raise ValueError(f"row {r} has an empty phrase set: a constrained answer needs at least one phrase")
        seen = set()
        for p in phrases:
            if isinstance(p, (str, bytes)):
                raise ValueError(f"row {r}: a phrase is a sequence of token ids, not a string ({p!r})")
            ids = tuple(int(t) for t in p)
            if len(ids) == 0:
                raise ValueError(f"row {r} has an empty phrase: every phrase holds at least one token")
            for t, raw in zip(ids, p):
                if isinstance(raw, bool) or t != raw or not 0 <= t < int(vocab):
                    raise ValueError(f"row {r}: token id {raw!r} is outside the vocabulary [0, {int(vocab)})")
            seen.add(ids)
        memo[id(phrases)] = tuple(sorted(seen))
        out.append(memo[id(phrases)])
    return out


def build_trie(phrases_per_row, vocab: int = VOCAB) -> Dict[str, np.ndarray]:
    """per row a list of token-id lists -> dict of int32 arrays node_first, node_flags, edge_token, edge_child, row_root (module
    docstring).  Nodes are numbered breadth first, one trie after the other, so every child has a larger index than its parent."""
    sets = check_constraint(phrases_per_row, vocab)
    root_of: Dict[Tuple[Tuple[int, ...], ...], int] = {}
    children: List[Dict[int, int]] = []            # node -> {token: child}
    terminal: List[int] = []
    for key in sets:
        if key in root_of:
            continue
        root_of[key] = root = len(children)
        children.append({})
        terminal.append(0)
        # breadth first over the prefixes: level d holds the nodes of the prefixes of length d, created in sorted order
        level = {(): root}
        depth = 0
        while level:
            nxt = {}
            for p in key:
                if len(p) <= depth:
                    continue
                pre = p[:depth + 1]
                if pre not in nxt:
                    nxt[pre] = len(children)
                    children.append({})
                    terminal.append(0)
                    children[level[pre[:-1]]][pre[-1]] = nxt[pre]
                if len(p) == depth + 1:
                    terminal[nxt[pre]] = 1
            level = nxt
            depth += 1
    n_nodes = len(children)
    n_edges = sum(len(c) for c in children)
    if n_nodes > MAX_COUNT or n_edges > MAX_COUNT or len(sets) > MAX_COUNT:
        raise ValueError(f"the constraint has {n_nodes} nodes, {n_edges} edges and {len(sets)} rows: at most {MAX_COUNT} of each")
    node_first = np.zeros(n_nodes + 1, dtype=np.int32)
    edge_token = np.zeros(n_edges, dtype=np.int32)
    edge_child = np.zeros(n_edges, dtype=np.int32)
    e = 0
    for u, c in enumerate(children):
        node_first[u] = e
        for t in sorted(c):
            edge_token[e], edge_child[e] = t, c[t]
            e += 1
    node_first[n_nodes] = e
    return {"node_first": node_first, "node_flags": np.asarray(terminal, dtype=np.int32), "edge_token": edge_token,
            "edge_child": edge_child, "row_root": np.asarray([root_of[k] for k in sets], dtype=np.int32)}


def constraint_digest(phrases_per_row: Sequence) -> str:
    """a digest of the phrase sets of a call (what data-parallel ranks compare: the sets are per call and the same on every rank)"""
    import hashlib
    return hashlib.sha1(repr(check_constraint(phrases_per_row, 1 << 31)).encode()).hexdigest()
