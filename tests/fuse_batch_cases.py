"""Inputs of the batched fusion tests (``mrag_fuse_topk_batch``) and a restatement of its rule on plain arrays.

A question is a dict ``{"n": (n_text, n_graph, n_dense), "keys": [...], "scores": [...], "payload": [...], "top_k": k}``:
the three channels' entries back to back, as the C call takes them.  ``reference`` restates the rule of
``fuse_kernel`` (csrc/fuse.hip) with Python floats (IEEE fp64, no contraction) and dicts; ``as_channels`` turns a question into the
hit dicts of ``fusion.fuse_channels`` so that tests/test_fuse_batch_host.py can tie ``reference`` to it.  Every case is
built for one condition, which that file establishes with the host code alone.
"""
import struct

import numpy as np

ALPHAS = (0.4, 0.2, 0.4)
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096)      # 4096: the limit, and a power of two


def question(text=(), graph=(), dense=(), top_k=10 ** 9):
    """channels as lists of (key, score); the payload is the entry's position in the question"""
    ent = list(text) + list(graph) + list(dense)
    return {"n": (len(text), len(graph), len(dense)), "keys": [int(k) for k, _ in ent], "scores": [float(s) for _, s in ent],
            "payload": list(range(len(ent))), "top_k": int(top_k)}


def _orderable(x: float) -> int:
    """the "orderable bits" of a double: a total order in which -0.0 < +0.0 (what the rule must NOT use)"""
    b = struct.unpack("<Q", struct.pack("<d", x))[0]
    return b ^ 0xFFFFFFFFFFFFFFFF if b >> 63 else b | (1 << 63)


def reference(q, alphas=ALPHAS, bitwise=False):
    """-> [(key, fused, text_norm, graph_norm, dense_norm, (payload_text, payload_graph, payload_dense))], best first, cut
    at ``q["top_k"]``.  ``bitwise=True`` compares scores through their orderable bits instead: the wrong rule."""
    gt = (lambda a, b: _orderable(a) > _orderable(b)) if bitwise else (lambda a, b: a > b)
    at = 0
    norm, pay = [], []
    for n_c in q["n"]:
        kept = {}                                           # key -> (score, payload, index): strictly larger wins the slot
        for i in range(at, at + n_c):
            k, s = q["keys"][i], q["scores"][i]
            if k not in kept or gt(s, kept[k][0]):
                kept[k] = (s, q["payload"][i], i)
        at += n_c
        order = sorted(kept.values(), key=lambda e: e[2])   # min / max walk the kept entries in index order
        lo = hi = None
        for s, _, _ in order:
            if lo is None:
                lo = hi = s
            else:
                lo = s if gt(lo, s) else lo
                hi = s if gt(s, hi) else hi
        norm.append({k: ((s - lo) / (hi - lo) if gt(hi, lo) else 0.0) for k, (s, _, _) in kept.items()})
        pay.append({k: p for k, (_, p, _) in kept.items()})
    out = []
    for k in sorted(set().union(*norm)):
        ts, gs, ds = (nm.get(k, 0.0) for nm in norm)
        out.append((k, alphas[0] * ts + alphas[1] * gs + alphas[2] * ds, ts, gs, ds, tuple(p.get(k, -1) for p in pay)))
    out.sort(key=lambda r: r[1], reverse=True)              # stable: ties stay in key order
    return out[:q["top_k"]]


def key_id(k: int) -> str:
    return "sent::K%09d::" % k                              # code-point order == key order


def as_channels(q):
    """-> (text_hits, graph_hits, dense_scores) of ``fusion.fuse_channels``; the dense channel is deduped like ``run``
    dedupes it (strictly larger wins).  Hit scores of -0.0 do not survive ``hit.get("score") or 0.0`` on the host, so
    questions with a negative zero are compared on arrays only."""
    nt, ng, nd = q["n"]
    ent = list(zip(q["keys"], q["scores"]))
    hits = lambda part: [{"id": key_id(k), "score": s, "meta": {}} for k, s in part]      # noqa: E731
    dense = {}
    for k, s in ent[nt + ng:]:
        if key_id(k) not in dense or s > dense[key_id(k)]:
            dense[key_id(k)] = s
    return hits(ent[:nt]), hits(ent[nt:nt + ng]), dense


def pack(questions):
    """-> (chan_ptr int32 [3B+1], keys int32, scores float64, payload int32, top_k int64 [B])"""
    ptr, keys, scores, payload = [0], [], [], []
    for q in questions:
        for n_c in q["n"]:
            ptr.append(ptr[-1] + n_c)
        keys += q["keys"]
        scores += q["scores"]
        payload += q["payload"]
    return (np.asarray(ptr, dtype=np.int32), np.asarray(keys, dtype=np.int32), np.asarray(scores, dtype=np.float64),
            np.asarray(payload, dtype=np.int32), np.asarray([q["top_k"] for q in questions], dtype=np.int64))


def random_question(n, seed, top_k=10 ** 9):
    """n entries split at random over the channels; few keys (duplicates inside and across channels) and scores that are
    multiples of 1/8 in [-1, 1] (equal scores among duplicates, ties of the fused score)"""
    rng = np.random.default_rng(seed)
    cut = np.sort(rng.integers(0, n + 1, size=2))
    keys = rng.integers(0, max(1, n // 2), size=n)
    scores = rng.integers(-8, 9, size=n) / 8.0
    ent = list(zip(keys.tolist(), scores.tolist()))
    return question(ent[:cut[0]], ent[cut[0]:cut[1]], ent[cut[1]:], top_k)


def size_questions():
    return [random_question(n, 100 + n) for n in SIZES]


def position_questions():
    """three questions whose rows must not depend on where they stand in a batch"""
    return [random_question(200, 7, top_k=20), random_question(65, 8, top_k=5), random_question(400, 9, top_k=50)]


def filler(g):
    return random_question(3 + g % 9, 1000 + g, top_k=4)


def channel_questions():
    t = [(3, 0.5), (1, 2.0), (7, -1.0), (1, 1.0)]
    return {
        "only text": question(text=t),
        "only graph": question(graph=t),
        "only dense": question(dense=t),
        "all-equal channel": question(text=[(1, 0.25), (2, 0.25), (3, 0.25)], dense=[(2, 1.0), (3, 3.0), (9, 2.0)]),
        "negative scores": question(text=[(1, -3.0), (2, -1.0), (3, -2.0)], graph=[(2, -0.5), (4, -8.0)], dense=[(1, -1.0), (5, -4.0)]),
        "one, two and three channels": question(text=[(1, 1.0), (2, 2.0), (3, 3.0)], graph=[(2, 5.0), (3, 1.0), (4, 2.0)],
                                                dense=[(3, 0.5), (5, 0.25), (6, 1.0)]),
    }


ZERO_ALPHAS = (0.0, 0.2, 0.8)                               # an alpha of 0: the text channel orders nothing


def dedupe_questions():
    return {
        # equal scores: the first one met keeps the slot (payload 1, not 2 .. 5)
        "five equal": question(text=[(9, 0.0), (4, 1.0), (4, 1.0), (4, 1.0), (4, 1.0), (4, 1.0), (2, 3.0)]),
        # a strictly larger, later entry takes it (payload 3), the equal one after it does not (payload 4)
        "later larger": question(dense=[(4, 1.0), (9, 0.0), (4, 1.5), (4, 2.0), (4, 2.0), (2, 3.0)]),
        # -0.0 and +0.0 are EQUAL: the first met stays (payload 0 in both orders); orderable bits would take +0.0
        "zeros as duplicates, -0 first": question(text=[(4, -0.0), (4, 0.0), (2, 3.0), (1, -1.0)]),
        "zeros as duplicates, +0 first": question(text=[(4, 0.0), (4, -0.0), (2, 3.0), (1, -1.0)]),
        # the channel's min is a zero of either sign: lo is the first met, and score - lo keeps that sign
        "zeros as min, +0 first": question(dense=[(1, 0.0), (2, -0.0), (3, 2.0)]),
        "zeros as min, -0 first": question(dense=[(1, -0.0), (2, 0.0), (3, 2.0)]),
        "zeros as max, +0 first": question(dense=[(1, 0.0), (2, -0.0), (3, -2.0)]),
        "zeros as max, -0 first": question(dense=[(1, -0.0), (2, 0.0), (3, -2.0)]),
    }


def tie_question(top_k=3):
    """keys 2, 4, 6, 8 fuse to the same score (0.4 * 0.5), below key 1 and above key 9: top_k = 3 cuts the group after
    key 4, by key order alone"""
    return question(text=[(9, 0.0), (8, 1.0), (6, 1.0), (1, 2.0), (4, 1.0), (2, 1.0)], top_k=top_k)


def cut_questions():
    """per-question top_k: 0, 1, exactly the distinct keys, more"""
    base = random_question(40, 77)
    distinct = len(set(base["keys"]))
    return [dict(base, top_k=k) for k in (0, 1, distinct, distinct + 5)], distinct
