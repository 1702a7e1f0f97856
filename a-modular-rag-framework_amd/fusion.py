"""Score fusion and hit normalisation of the retrieval boundary -- host side, runs on the k
results AFTER the GPU top-k.  Semantics follow the reference line by line (cited per
function); implementation is this package's own.

Declared tie-break where the reference leaves the order to ``set`` iteration
(retrieval_backend.py:357-359): equal fused scores are ordered by ascending id.
"""
from __future__ import annotations

from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

ID_KEYS = ["id", "doc_id", "docId", "sid", "sent_id"]          # retrieval_adapter.py:33
SCORE_KEYS = ["score", "relevance", "sim", "s"]                # retrieval_adapter.py:34


def raw_hit_id(row: Dict[str, Any]) -> str:
    """id of a corpus row as the reference's text channel spells it
    (retrieval_backend.py:116-119): ``sent::{doc_id|title|'doc'}::{sent_id or ''}``."""
    return "sent::%s::%s" % (row.get("doc_id") or row.get("title") or "doc", str(row.get("sent_id") or ""))


def row_meta(row: Dict[str, Any], source: str) -> Dict[str, Any]:
    """meta block of a hit (retrieval_backend.py:121-127); ``text``/``doc``/``sent_id`` are what
    reasoning and graph bootstrap read."""
    return {"kind": "sentence", "text": row.get("text"), "doc": row.get("title"), "sent_id": row.get("sent_id"),
            "source": source}


def normalize_id(hit: Dict[str, Any]) -> Tuple[str, Dict[str, Any]]:
    """retrieval_backend.py:283-294."""
    meta = hit.get("meta") or {}
    doc = meta.get("doc") or meta.get("title")
    sid = meta.get("sent_id") or meta.get("sid")
    if doc is not None:
        return ("sent::%s::%s" % (doc, sid if sid is not None else "")), meta
    return (hit.get("id") or "sent::unknown::"), meta


def minmax_norm(values: Dict[str, float]) -> Dict[str, float]:
    """retrieval_backend.py:296-301: empty -> {}, max <= min -> all 0.0."""
    if not values:
        return {}
    seq = list(values.values())
    lo, hi = min(seq), max(seq)
    if hi <= lo:
        return dict.fromkeys(values, 0.0)
    span = hi - lo
    return {key: (val - lo) / span for key, val in values.items()}


def dedupe_by_norm_id(hits: Optional[Iterable[Dict[str, Any]]]) -> Dict[str, Dict[str, Any]]:
    """retrieval_backend.py:336-348: strictly higher score wins the slot; a loser only
    contributes meta keys the winner does not have."""
    table: Dict[str, Dict[str, Any]] = {}
    for hit in hits or []:
        nid, meta = normalize_id(hit)
        score = float(hit.get("score") or 0.0)
        cur = table.get(nid)
        if cur is None or score > float(cur.get("score") or 0.0):
            table[nid] = {"id": nid, "score": score, "meta": dict(meta or {})}
            continue
        kept = cur.get("meta") or {}
        for key, val in (meta or {}).items():
            if key not in kept:
                kept[key] = val
        cur["meta"] = kept
    return table


def fuse_channels(text_hits, graph_hits, dense_scores: Dict[str, float], *, alpha_text: float,
                  alpha_graph: float, alpha_dense: float, top_k: int) -> List[Dict[str, Any]]:
    """retrieval_backend.py:350-372: per-channel min-max, alpha-weighted sum over the union of
    ids, meta = text meta overlaid by graph meta + the three ``score_*_norm`` keys, sort by
    score descending (ties: id ascending), keep ``top_k``."""
    tmap, gmap = dedupe_by_norm_id(text_hits), dedupe_by_norm_id(graph_hits)
    n_text = minmax_norm({key: float(val["score"]) for key, val in tmap.items()})
    n_graph = minmax_norm({key: float(val["score"]) for key, val in gmap.items()})
    n_dense = minmax_norm(dense_scores)
    out = []
    for nid in sorted(set(tmap).union(gmap, n_dense)):
        ts, gs, ds = n_text.get(nid, 0.0), n_graph.get(nid, 0.0), n_dense.get(nid, 0.0)
        meta: Dict[str, Any] = {}
        for src in (tmap, gmap):
            if nid in src and isinstance(src[nid].get("meta"), dict):
                meta.update(src[nid]["meta"])
        meta["score_text_norm"], meta["score_graph_norm"], meta["score_dense_norm"] = ts, gs, ds
        out.append({"id": nid, "score": float(alpha_text * ts + alpha_graph * gs + alpha_dense * ds), "meta": meta})
    out.sort(key=lambda h: h["score"], reverse=True)        # stable: ties stay in id order
    return out[:top_k]


def fuse_channels_device(text_hits, graph_hits, dense_scores: Dict[str, float], *, alpha_text: float, alpha_graph: float,
                         alpha_dense: float, top_k: int, device: int = 0) -> List[Dict[str, Any]]:
    """:func:`fuse_channels` with the arithmetic on the GPU, as one question of :func:`fuse_entries_device_batch`: ids
    are normalised and ranked on the host (a key = the id's position among the call's sorted ids), the dedupe / min-max /
    weighted sum / sort / truncate of retrieval_backend.py:336-372 run in one launch, and the host re-attaches ids and
    meta to the ``top_k`` survivors.  Same values bit for bit (fp64, same operation order), same declared tie order."""
    import numpy as np
    chans = []
    for hits in (text_hits, graph_hits):
        ent = []
        for hit in hits or []:
            nid, _ = normalize_id(hit)
            ent.append((nid, float(hit.get("score") or 0.0)))
        chans.append(ent)
    chans.append([(nid, float(v)) for nid, v in dense_scores.items()])
    ids = sorted({nid for ent in chans for nid, _ in ent})
    if not ids or top_k <= 0:
        return []
    key_of = {nid: i for i, nid in enumerate(ids)}
    keys = np.asarray([key_of[nid] for ent in chans for nid, _ in ent], dtype=np.int32)
    scores = np.asarray([v for ent in chans for _, v in ent], dtype=np.float64)
    chan_ptr = np.cumsum([0] + [len(ent) for ent in chans], dtype=np.int32)
    ok, osc, nt, ng, nd, _, n_out = fuse_entries_device_batch(
        chan_ptr, keys, scores, None, alpha_text=alpha_text, alpha_graph=alpha_graph, alpha_dense=alpha_dense,
        top_k=int(min(top_k, len(ids))), device=device)
    tmap, gmap = dedupe_by_norm_id(text_hits), dedupe_by_norm_id(graph_hits)        # meta merge of the survivors (host dicts)
    out = []
    for i in range(int(n_out[0])):
        nid = ids[int(ok[0, i])]
        meta: Dict[str, Any] = {}
        for src in (tmap, gmap):
            if nid in src and isinstance(src[nid].get("meta"), dict):
                meta.update(src[nid]["meta"])
        meta["score_text_norm"], meta["score_graph_norm"], meta["score_dense_norm"] = float(nt[0, i]), float(ng[0, i]), float(nd[0, i])
        out.append({"id": nid, "score": float(osc[0, i]), "meta": meta})
    return out


def normalize_raw_hit(raw: Any, id_keys: Sequence[str] = ID_KEYS, score_keys: Sequence[str] = SCORE_KEYS,
                      meta_key: Optional[str] = "meta") -> Optional[Dict[str, Any]]:
    """retrieval_adapter.py:71-109: first non-None id/score alias, unparsable score -> 0.0,
    meta from ``meta_key`` when it is a dict else all non-alias fields, missing id rebuilt
    as ``sent::{doc|title|'doc'}::{sent_id|sid|''}``."""
    if raw is None:
        return None
    if isinstance(raw, dict):
        d = dict(raw)
    else:
        d = {k: getattr(raw, k) for k in dir(raw) if not k.startswith("_") and hasattr(raw, k)}

    def first(keys):
        for k in keys:
            if d.get(k) is not None:
                return d[k]
        return None

    hid, score = first(id_keys), first(score_keys)
    try:
        score = 0.0 if score is None else float(score)
    except Exception:
        score = 0.0
    if meta_key and isinstance(d.get(meta_key), dict):
        meta = dict(d[meta_key])
    else:
        meta = {k: v for k, v in d.items() if k not in id_keys and k not in score_keys}
    if not hid:
        hid = "sent::%s::%s" % (meta.get("doc") or meta.get("title") or "doc", meta.get("sent_id") or meta.get("sid") or "")
    return {"id": str(hid), "score": score, "meta": meta}


# ---- device fusion (mrag_fuse_topk_batch): many questions, one launch ----------------------------------------------
FUSE_MAX_ENTRIES = 4096          # entries of one question over its three channels: the limit of the device call


def corpus_norm_keys(rows: Sequence[Dict[str, Any]]):
    """``(keys int32 [n_rows], sorted_ids)``: ``keys[r]`` is the rank of row r's NORMALISED id (:func:`normalize_id` of
    the hit either channel builds from the row) among the distinct normalised ids of the corpus, ``sorted_ids[key]`` the
    id itself.  Ascending key is ascending id, and rows that share a normalised id share a key -- so the device's dedupe
    by key is :func:`dedupe_by_norm_id`, and nothing per entry has to be normalised or sorted at query time."""
    import numpy as np
    nids = [normalize_id({"id": raw_hit_id(row), "meta": row_meta(row, "")})[0] for row in rows]
    sorted_ids = sorted(set(nids))
    rank = {nid: i for i, nid in enumerate(sorted_ids)}
    return np.asarray([rank[nid] for nid in nids], dtype=np.int32).reshape(-1), sorted_ids


def batch_entries(text_docs, text_scores, text_n, dense_ids, dense_scores, norm_keys, pool=None, graph_rows=None,
                  graph_scores=None, graph_n=None):
    """The entries of ``mrag_fuse_topk_batch`` from the result arrays of the two batched searches, without a Python
    object per entry: ``text_docs`` / ``text_scores`` [B][kt] with ``text_n`` [B] valid slots per question (BM25),
    ``dense_ids`` / ``dense_scores`` [B][kd] with id -1 = no row (dense), ``norm_keys`` from :func:`corpus_norm_keys`,
    ``pool`` [B] (optional) = how many leading slots of each list the question uses.  Returns ``(chan_ptr int32
    [3B+1], keys int32, scores float64, payload int32)``: per question its text entries, its graph entries, its dense
    entries, each in list order; key = the row's normalised-id rank, payload = the row, fp32 scores widened exactly.
    The graph channel (optional, all three or none) is ``graph_rows`` [B][kg] corpus rows, ``graph_scores`` [B][kg]
    fp64 and ``graph_n`` [B] valid leading slots per question (``DenseIndex.expand_neighbors``); without it every
    question has no graph entries and the result is what it was before the arguments existed."""
    import numpy as np
    text_docs, dense_ids = np.asarray(text_docs, dtype=np.int64), np.asarray(dense_ids, dtype=np.int64)
    B = text_docs.shape[0]
    if B == 0:
        return np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64), np.zeros(0, dtype=np.int32)
    if (graph_rows is None) != (graph_scores is None) or (graph_rows is None) != (graph_n is None):
        raise ValueError("pass graph_rows, graph_scores and graph_n together or not at all")
    text_docs, dense_ids = text_docs.reshape(B, -1), dense_ids.reshape(B, -1)
    text_scores = np.asarray(text_scores, dtype=np.float64).reshape(B, -1)
    dense_scores = np.asarray(dense_scores).astype(np.float64).reshape(B, -1)
    lim = np.full(B, 2 ** 31 - 1, dtype=np.int64) if pool is None else np.asarray(pool, dtype=np.int64).reshape(B)
    t_mask = np.arange(text_docs.shape[1])[None, :] < np.minimum(np.asarray(text_n, dtype=np.int64).reshape(B), lim)[:, None]
    d_mask = (np.arange(dense_ids.shape[1])[None, :] < lim[:, None]) & (dense_ids >= 0)
    tn, dn = t_mask.sum(axis=1), d_mask.sum(axis=1)
    gn = np.zeros(B, dtype=tn.dtype)
    if graph_rows is not None:
        graph_rows = np.asarray(graph_rows, dtype=np.int64).reshape(B, -1)
        graph_scores = np.asarray(graph_scores, dtype=np.float64).reshape(B, -1)
        g_mask = ((np.arange(graph_rows.shape[1])[None, :] < np.minimum(np.asarray(graph_n, dtype=np.int64).reshape(B), lim)[:, None])
                  & (graph_rows >= 0))
        gn = g_mask.sum(axis=1)
    start = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(tn + gn + dn, out=start[1:])
    if start[-1] > 2 ** 31 - 1:
        raise ValueError(f"{int(start[-1])} fusion entries in one batch exceed the int32 offsets of the call")
    chan_ptr = np.empty(3 * B + 1, dtype=np.int32)
    chan_ptr[0:3 * B:3] = start[:-1]
    chan_ptr[1:3 * B:3] = start[:-1] + tn
    chan_ptr[2:3 * B:3] = start[:-1] + tn + gn
    chan_ptr[3 * B] = start[-1]
    E = int(start[-1])
    keys, scores, payload = np.empty(E, dtype=np.int32), np.empty(E, dtype=np.float64), np.empty(E, dtype=np.int32)
    norm_keys = np.asarray(norm_keys, dtype=np.int32)
    channels = [(t_mask, start[:-1], text_docs, text_scores), (d_mask, start[:-1] + tn + gn, dense_ids, dense_scores)]
    if graph_rows is not None:
        channels.insert(1, (g_mask, start[:-1] + tn, graph_rows, graph_scores))
    for mask, first, rows, vals in channels:
        dest = (first[:, None] + np.cumsum(mask, axis=1) - 1)[mask]
        r = rows[mask]
        keys[dest], scores[dest], payload[dest] = norm_keys[r], vals[mask], r
    return chan_ptr, keys, scores, payload


def fuse_entries_device_batch(chan_ptr, keys, scores, payload=None, *, alpha_text: float, alpha_graph: float, alpha_dense: float,
                              top_k, device: int = 0):
    """``mrag_fuse_topk_batch``, arrays in and arrays out.  ``chan_ptr`` int32 [3B+1]: question g's text, graph and dense
    entries are the three consecutive ranges of ``keys`` / ``scores`` / ``payload`` starting at ``chan_ptr[3g]``;
    ``top_k`` is an int or one value per question (cut to the question's entry count, which bounds its distinct keys).
    Returns ``(out_keys, out_scores, text_norm, graph_norm, dense_norm, out_payload | None, out_n)``, the first five
    [B][stride] with stride = the largest ``top_k``, ``out_payload`` [B][stride][3]; slots past ``out_n[g]`` hold
    key -1, payload -1 and 0.0."""
    import numpy as np
    from . import _native as N
    cp = np.ascontiguousarray(chan_ptr, dtype=np.int32).reshape(-1)
    if cp.shape[0] % 3 != 1:
        raise ValueError(f"chan_ptr must hold 3 * n_questions + 1 offsets, got {cp.shape[0]}")
    B = cp.shape[0] // 3
    keys = np.ascontiguousarray(keys, dtype=np.int32).reshape(-1)
    scores = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)
    if keys.shape[0] != scores.shape[0] or (B and int(cp[-1]) > keys.shape[0]):
        raise ValueError(f"chan_ptr ends at {int(cp[-1])}, keys / scores hold {keys.shape[0]} / {scores.shape[0]} entries")
    if payload is not None:
        payload = np.ascontiguousarray(payload, dtype=np.int32).reshape(-1)
        if payload.shape[0] != keys.shape[0]:
            raise ValueError(f"payload holds {payload.shape[0]} entries, keys {keys.shape[0]}")
    tk = np.broadcast_to(np.asarray(top_k, dtype=np.int64), (B,)) if np.ndim(top_k) == 0 else np.asarray(top_k, dtype=np.int64).reshape(-1)
    if tk.shape[0] != B:
        raise ValueError(f"top_k holds {tk.shape[0]} values for {B} questions")
    if B and int(tk.min()) < 0:
        raise ValueError("top_k must not be negative")
    tk = np.ascontiguousarray(np.minimum(tk, np.maximum(cp[3::3].astype(np.int64) - cp[0:-1:3], 0)), dtype=np.int32)
    stride = int(tk.max()) if B else 0
    ok = np.full((B, stride), -1, dtype=np.int32)
    osc, nt, ng, nd = (np.zeros((B, stride), dtype=np.float64) for _ in range(4))
    op = np.full((B, stride, 3), -1, dtype=np.int32) if payload is not None else None
    n = np.zeros(B, dtype=np.int32)
    if B:
        N.check(N.load().mrag_fuse_topk_batch(int(device), B, cp.ctypes.data, keys.ctypes.data, scores.ctypes.data,
                                              payload.ctypes.data if payload is not None else None, float(alpha_text),
                                              float(alpha_graph), float(alpha_dense), tk.ctypes.data, stride, ok.ctypes.data,
                                              osc.ctypes.data, nt.ctypes.data, ng.ctypes.data, nd.ctypes.data,
                                              op.ctypes.data if op is not None else None, n.ctypes.data, None))
    return ok, osc, nt, ng, nd, op, n


def fuse_channels_device_batch(questions, *, alpha_text: float, alpha_graph: float, alpha_dense: float, top_k,
                               device: int = 0) -> List[List[Dict[str, Any]]]:
    """:func:`fuse_channels` for many questions with ONE device call (``mrag_fuse_topk_batch``): ``questions[g] =
    (text_hits, graph_hits, dense_scores)``, ``top_k`` an int or one value per question; the result holds one hit list
    per question, equal to ``fuse_channels(*questions[g], top_k=...)``.  Ids are normalised and ranked per question on
    the host as :func:`fuse_channels_device` does; a question of more than ``FUSE_MAX_ENTRIES`` entries is fused by
    :func:`fuse_channels` on the host."""
    import numpy as np
    questions = list(questions)
    B = len(questions)
    if not B:
        return []
    tks = [int(top_k)] * B if np.ndim(top_k) == 0 else [int(v) for v in top_k]
    if len(tks) != B:
        raise ValueError(f"top_k holds {len(tks)} values for {B} questions")
    alphas = dict(alpha_text=alpha_text, alpha_graph=alpha_graph, alpha_dense=alpha_dense)
    out: List[Optional[List[Dict[str, Any]]]] = [None] * B
    dev, ids_of, ptr, keys, scores, dev_tk = [], [], [0], [], [], []
    for g, (text_hits, graph_hits, dense_scores) in enumerate(questions):
        chans = [[(normalize_id(hit)[0], float(hit.get("score") or 0.0)) for hit in hits or []] for hits in (text_hits, graph_hits)]
        chans.append([(nid, float(v)) for nid, v in dense_scores.items()])
        n = sum(len(ent) for ent in chans)
        if tks[g] <= 0 or n == 0:
            out[g] = []
            continue
        if n > FUSE_MAX_ENTRIES:
            out[g] = fuse_channels(text_hits, graph_hits, dense_scores, top_k=tks[g], **alphas)
            continue
        ids = sorted({nid for ent in chans for nid, _ in ent})
        key_of = {nid: i for i, nid in enumerate(ids)}
        for ent in chans:
            keys.extend(key_of[nid] for nid, _ in ent)
            scores.extend(v for _, v in ent)
            ptr.append(len(keys))
        dev.append(g)
        ids_of.append(ids)
        dev_tk.append(min(tks[g], len(ids)))
    if dev:
        ok, osc, nt, ng, nd, _, n_out = fuse_entries_device_batch(
            np.asarray(ptr, dtype=np.int32), np.asarray(keys, dtype=np.int32), np.asarray(scores, dtype=np.float64), None,
            top_k=np.asarray(dev_tk, dtype=np.int64), device=device, **alphas)
        for j, g in enumerate(dev):
            text_hits, graph_hits, _ = questions[g]
            tmap, gmap = dedupe_by_norm_id(text_hits), dedupe_by_norm_id(graph_hits)     # meta merge of the survivors (host dicts)
            hits = []
            for i in range(int(n_out[j])):
                nid = ids_of[j][int(ok[j, i])]
                meta: Dict[str, Any] = {}
                for src in (tmap, gmap):
                    if nid in src and isinstance(src[nid].get("meta"), dict):
                        meta.update(src[nid]["meta"])
                meta["score_text_norm"], meta["score_graph_norm"], meta["score_dense_norm"] = float(nt[j, i]), float(ng[j, i]), float(nd[j, i])
                hits.append({"id": nid, "score": float(osc[j, i]), "meta": meta})
            out[g] = hits
    return out
