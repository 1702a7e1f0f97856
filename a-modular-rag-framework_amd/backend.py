"""Boundary B2 -- retrieval backends selected by ``modules.retrieval.impl``
(config/settings.yaml:83; built by RetrievalAgentFlow.from_settings,
app/modules/retrieval/flow.py:91-108: kwargs filtered to ``__init__``, ``router``/``sink``
injected when declared).

``HipDenseReranker``      drop-in for ``DenseReranker`` (retrieval_backend.py:186-247): same
                          embed-call sequence and error policy, the N cosines run as one fp64
                          GPU kernel instead of a Python loop.
``DenseRetrievalBackend`` corpus-wide dense retrieval: the whole docs.jsonl is embedded once
                          (cached on disk and process-wide), kept in HBM as fp16, and every
                          query is one fused MFMA cosine top-k -- ``run(req) -> {"hits",
                          "diagnostics"}`` and ``retrieve(req) -> RetrievalOut`` like
                          ``HybridRetrievalBackend`` (:303-390), hit ids / meta / fusion keys
                          unchanged.  Optional text / graph channels are injected callables
                          with the reference's hit shape and fused with the reference's
                          min-max + alpha rule.  ``dense_mode="rerank"``: the dense channel
                          scores the text channel's candidates (the reference's step 4, :332-334)
                          instead of searching the corpus.  ``graph_channel="neighbors"``:
                          the graph channel on the device, the sentences around the leading
                          dense hits inside their documents (``DenseIndex.expand_neighbors``).
"""
from __future__ import annotations

import logging
from typing import Any, Callable, Dict, List, Optional

import numpy as np

from . import corpus as _corpus
from . import fusion as _fusion
from .dto import Hit, RetrievalIn, RetrievalOut
from .telemetry import span

logger = logging.getLogger(__name__)
DEFAULT_EMBED_MODEL = "text-embedding-3-large"      # retrieval_backend.py:213


def resolve_embed_model(router) -> str:
    """retrieval_backend.py:199-213."""
    try:
        policy = getattr(router, "policy", {}) or {}
        emb = policy.get("embedding") or []
        if emb and isinstance(emb[0], dict) and emb[0].get("model"):
            return emb[0]["model"]
        name = policy.get("embedding_provider")
        prov = (getattr(router, "providers", {}) or {}).get(name) if name else None
        if prov is not None and hasattr(prov, "kwargs"):
            model = (getattr(prov, "kwargs") or {}).get("embed_model")
            if model:
                return model
    except Exception:
        pass
    return DEFAULT_EMBED_MODEL


def _vectors(ret):
    return ret.get("vectors") if isinstance(ret, dict) else ret


class HipDenseReranker:
    """``DenseReranker`` with the cosine loop on the GPU.  Same constructor fields."""

    def __init__(self, router, max_pool: int = 200, embed_batch: int = 50, device: int = 0, corpus=None):
        """``corpus`` (optional): a :class:`DenseRetrievalBackend` over the docs.jsonl the candidates come
        from.  Candidates whose id is a row of its index are then scored by row id against the stored
        embedding -- no embed call for them (the reference pays 1 + ceil(N/bs) embedding
        round-trips per question, retrieval_backend.py:227-243); candidates it does not know, or whose
        text differs from the stored row's, are embedded as before."""
        self.router, self.max_pool, self.embed_batch, self.device = router, max_pool, embed_batch, device
        self.corpus = corpus

    def _resolve_embed_model(self) -> str:
        return resolve_embed_model(self.router)

    def _cosines(self, qv, vecs) -> List[float]:
        """retrieval_backend.py:192-197 for every candidate: 0.0 when a side is empty, the
        lengths differ (:193) or a norm is zero (:197); everything else in one kernel."""
        from .index import cosine_f64
        d = len(qv)
        out = [0.0] * len(vecs)
        rows = [i for i, v in enumerate(vecs) if d and v is not None and len(v) == d]
        if rows:
            got = cosine_f64(np.asarray(qv, dtype=np.float64),
                             np.asarray([vecs[i] for i in rows], dtype=np.float64), device=self.device)
            for i, g in zip(rows, got):
                out[i] = float(g)
        return out

    def score(self, *, query: str, candidates: List[Dict[str, Any]], trace_id: str) -> Dict[str, float]:
        if not candidates:
            return {}
        ids, texts = self._select(candidates)
        if not texts:
            return {}
        model_hint = self._resolve_embed_model()
        try:
            qv = _vectors(self.router.embed(model_hint=model_hint, texts=[query], require={"trace_id": trace_id}))[0]
        except Exception as e:                      # :229-231
            logger.error("[HipDenseReranker] query embed error: %s", e)
            return {}
        known: Dict[int, float] = {}                # candidate position -> score from the stored row
        if self.corpus is not None:
            known = self._lookup(ids, texts, qv, model_hint, trace_id)
        return self._score_rest(ids, texts, qv, known, model_hint, trace_id)

    def _score_rest(self, ids: List[str], texts: List[str], qv, known: Dict[int, float], model_hint: str,
                    trace_id: str) -> Dict[str, float]:
        """The candidates ``known`` does not cover, embedded in chunks and scored (:234-245), merged with ``known``."""
        todo = [i for i in range(len(texts)) if i not in known]
        vecs: List[Any] = []
        step = max(8, int(self.embed_batch))        # :234
        for lo in range(0, len(todo), step):
            chunk = [texts[i] for i in todo[lo:lo + step]]
            try:
                got = _vectors(self.router.embed(model_hint=model_hint, texts=chunk, require={"trace_id": trace_id}))
                vecs.extend(got or [])
            except Exception as e:                  # :241-243
                logger.error("[HipDenseReranker] batch embed error: %s", e)
                vecs.extend([[0.0] * len(qv) for _ in chunk])
        n = min(len(todo), len(vecs))               # zip() truncation of :245
        scored = dict(zip(todo[:n], self._cosines(qv, vecs[:n])))
        scored.update(known)
        return {ids[i]: scored[i] for i in range(len(ids)) if i in scored}

    def _select(self, candidates):
        """The candidates ``score`` looks at (:218-224): the leading ``max_pool``, those without text skipped."""
        ids, texts = [], []
        for h in (candidates or [])[: self.max_pool]:
            t = (h.get("meta") or {}).get("text") or ""
            if t:
                ids.append(h["id"])
                texts.append(t)
        return ids, texts

    def score_batch(self, *, queries: List[str], candidates: List[List[Dict[str, Any]]],
                    trace_ids: List[str]) -> List[Dict[str, float]]:
        """:meth:`score` for every question of a list: one ``{id: score}`` dict per question, each equal to
        ``score(query=, candidates=, trace_id=)`` of that question alone.  The queries are embedded in chunks of
        ``embed_batch`` instead of one call each, and with ``corpus=`` the known candidates of ALL questions are scored
        in one ``DenseIndex.score_rows_batch``; each question's unknown remainder is embedded and scored as in
        :meth:`score`.  If a query chunk raises or comes back with the wrong count, a wrong dim or an all-zero vector (the
        router's answer to a provider failure), the whole call is the loop of :meth:`score` -- the per-question error
        policy (:229-231) is then the reference's."""
        queries, candidates, trace_ids = list(queries), list(candidates), list(trace_ids)
        B = len(queries)
        if len(candidates) != B or len(trace_ids) != B:
            raise ValueError(f"{B} queries, {len(candidates)} candidate lists, {len(trace_ids)} trace ids")
        sel = [self._select(c) for c in candidates]
        live = [g for g in range(B) if sel[g][1]]    # the questions for which score() reaches the query embed
        out: List[Dict[str, float]] = [{} for _ in range(B)]
        if not live:
            return out
        model_hint = self._resolve_embed_model()
        qvs: Dict[int, Any] = {}
        step = max(1, int(self.embed_batch))
        try:
            for lo in range(0, len(live), step):
                chunk = live[lo:lo + step]
                got = list(_vectors(self.router.embed(model_hint=model_hint, texts=[queries[g] for g in chunk],
                                                      require={"trace_id": trace_ids[chunk[0]]})) or [])
                if len(got) != len(chunk):
                    raise ValueError(f"{len(got)} vectors for {len(chunk)} queries")
                qvs.update(zip(chunk, got))
            dim = len(qvs[live[0]])
            if not dim or any(len(qvs[g]) != dim for g in live):
                raise ValueError("query vectors of differing or zero dim")
            if not all(any(qvs[g]) for g in live):     # the router's answer to a provider failure (llm_router.py:124-129)
                raise ValueError("an all-zero query vector")
        except Exception as e:
            logger.error("[HipDenseReranker] batched query embed failed, scoring question by question: %s", e)
            return [self.score(query=q, candidates=c, trace_id=t) for q, c, t in zip(queries, candidates, trace_ids)]
        known: Dict[int, Dict[int, float]] = {}
        if self.corpus is not None:
            known = self._lookup_batch(live, sel, qvs, dim, model_hint, trace_ids[live[0]])
        for g in live:
            out[g] = self._score_rest(sel[g][0], sel[g][1], qvs[g], known.get(g, {}), model_hint, trace_ids[g])
        return out

    def _lookup_batch(self, live, sel, qvs, dim: int, model_hint: str, trace_id: str) -> Dict[int, Dict[int, float]]:
        """:meth:`_lookup` for the questions ``live``: question -> {candidate position: score}, the known candidates of
        all of them scored in one call.  Any failure degrades to "nothing known" for every question."""
        try:
            state = self.corpus._get_state(model_hint, trace_id)
            ix, row_of, rows = state["index"], state["row_of"], state["rows"]
            if ix is None or dim != state["dim"]:
                return {}
            who, pos, rid = [], [], []
            for g in live:
                p, r = [], []
                for i, (hid, text) in enumerate(zip(*sel[g])):
                    row = row_of.get(hid)
                    if row is not None and (rows[row].get("text") or "") == text:
                        p.append(i)
                        r.append(row)
                if p:
                    who.append(g)
                    pos.append(p)
                    rid.append(np.asarray(r, dtype=np.int64))
            if not who:
                return {}
            sc = ix.score_rows_batch(np.asarray([qvs[g] for g in who], dtype=np.float32), rid)
            return {g: {i: float(v) for i, v in zip(p, s)} for g, p, s in zip(who, pos, sc)}
        except Exception as e:
            logger.error("[HipDenseReranker] row lookup failed, embedding every candidate: %s", e)
            return {}

    def _lookup(self, ids: List[str], texts: List[str], qv, model_hint: str, trace_id: str) -> Dict[int, float]:
        """Scores of the candidates that are rows of ``self.corpus``'s index (same embedding model, same
        text), by row id on the GPU.  Any failure degrades to "nothing known" -- the embed path then
        scores everything, as the reference does."""
        try:
            state = self.corpus._get_state(model_hint, trace_id)
            ix, row_of, rows = state["index"], state["row_of"], state["rows"]
            if ix is None or len(qv) != state["dim"]:
                return {}
            pos, rid = [], []
            for i, (hid, text) in enumerate(zip(ids, texts)):
                r = row_of.get(hid)
                if r is not None and (rows[r].get("text") or "") == text:
                    pos.append(i)
                    rid.append(r)
            if not pos:
                return {}
            sc = ix.score_rows(np.asarray(qv, dtype=np.float32), np.asarray(rid, dtype=np.int64))
            return {i: float(v) for i, v in zip(pos, sc)}
        except Exception as e:
            logger.error("[HipDenseReranker] row lookup failed, embedding every candidate: %s", e)
            return {}


class DenseRetrievalBackend:
    """Corpus-wide dense retrieval behind ``run`` / ``retrieve`` (see module docstring)."""

    def __init__(self, router, sink=None, index_path: str = "data/hotpotqa/docs.jsonl",
                 alpha_text: float = 0.4, alpha_graph: float = 0.2, alpha_dense: float = 0.4,
                 default_top_k: int = 20, dense_pool_k: int = 200, embed_batch: int = 256,
                 cache_dir: Optional[str] = None, device: int = 0, index_dtype: str = "f16",
                 text_search: Optional[Callable[..., List[Dict[str, Any]]]] = None,
                 graph_expand: Optional[Callable[..., List[Dict[str, Any]]]] = None,
                 text_channel: Optional[str] = None, bm25_k1: float = 1.5, bm25_b: float = 0.75,
                 fuse_on_device: bool = False, bulk_ingest: bool = True, bulk_batch: int = 4096,
                 dense_row_filter: Optional[Any] = None, dense_mode: str = "search", dense_filter_batch: bool = False,
                 query_expander: Optional[Any] = None, dense_expanded: bool = False,
                 dense_collapse: Optional[Any] = None,
                 graph_channel: Optional[str] = None, graph_window: int = 2, graph_seed_k: Optional[int] = None,
                 graph_doc: Any = "title"):
        self.router, self.sink = router, sink
        self.index_path = index_path
        self.alpha_text, self.alpha_graph, self.alpha_dense = float(alpha_text), float(alpha_graph), float(alpha_dense)
        self.default_top_k, self.dense_pool_k, self.embed_batch = int(default_top_k), int(dense_pool_k), int(embed_batch)
        self.cache_dir, self.device, self.index_dtype = cache_dir, int(device), index_dtype
        self.text_search, self.graph_expand = text_search, graph_expand
        # text_channel="bm25": the reference's BM25 channel (text_index.py, retrieval_backend.py:102-128) over the same
        # docs.jsonl, on the device (mrag_amd.text_index), built once per file and shared process-wide
        self.text_channel, self.bm25_k1, self.bm25_b = text_channel, float(bm25_k1), float(bm25_b)
        self.fuse_on_device = bool(fuse_on_device)     # a7's arithmetic in one launch (mrag_fuse_topk_batch) instead of host Python
        # corpus ingest: when the provider the router resolves can embed in bulk on the device (``embed_device``), the
        # index is built from docs.jsonl through it in ``bulk_batch``-passage batches (text_index.py:32-53: the reference
        # builds its index from the file in one go); the router path below stays as the fallback / error-policy reference
        self.bulk_ingest, self.bulk_batch = bool(bulk_ingest), int(bulk_batch)
        self.last_build: Dict[str, Any] = {}
        # dense_row_filter(req, rows) -> None | bool mask over the corpus rows | row positions: the dense channel then
        # searches only those rows (DenseIndex.search(allow=...)); a "pkg.mod:func" string (settings.yaml impl_kwargs)
        # is resolved like the reference's impl strings
        if isinstance(dense_row_filter, str):
            from .adapter import import_from_string
            dense_row_filter = import_from_string(dense_row_filter)
        if dense_row_filter is not None and not callable(dense_row_filter):
            raise TypeError(f"dense_row_filter must be callable or a 'pkg.mod:func' string, got {type(dense_row_filter)}")
        self.dense_row_filter = dense_row_filter
        # run_batch: the requests whose filter returns a set share ONE DenseIndex.search_sets call instead of one filtered
        # search each (off by default: their diagnostics then name the path "sets", not the single search's)
        self.dense_filter_batch = bool(dense_filter_batch)
        self._own_text_search = None                     # the searcher _bm25_searcher() made over index_path, if any
        if text_channel not in (None, "bm25"):
            raise ValueError(f"unknown text_channel {text_channel!r} (supported: 'bm25')")
        # dense_mode="search": the dense channel is a corpus-wide top-k (above).  "rerank": it scores the text channel's
        # candidates instead -- the reference's step 4 (retrieval_backend.py:332-334) with max_pool = pool
        if dense_mode not in ("search", "rerank"):
            raise ValueError(f"unknown dense_mode {dense_mode!r} (supported: 'search', 'rerank')")
        if dense_mode == "rerank" and dense_row_filter is not None:
            raise ValueError("dense_row_filter restricts the corpus-wide search: it has no meaning with dense_mode='rerank'")
        self.dense_mode = dense_mode
        # query_expander(query=, trace_id=) -> List[str] (the signature of the reference's LLMQueryExpander.expand): the
        # reference's Expand step, queries = [req.query] + expanded (retrieval_backend.py:307-310); a "pkg.mod:func"
        # string is resolved like dense_row_filter.  The text channel always receives the list; the dense channel embeds
        # and searches all of it, max-merged per row (DenseIndex.search_groups), only with dense_expanded=True
        if isinstance(query_expander, str):
            from .adapter import import_from_string
            query_expander = import_from_string(query_expander)
        if query_expander is not None and not callable(query_expander):
            raise TypeError(f"query_expander must be callable or a 'pkg.mod:func' string, got {type(query_expander)}")
        self.query_expander = query_expander
        self.dense_expanded = bool(dense_expanded)
        if self.dense_expanded and dense_mode == "rerank":
            raise ValueError("dense_mode='rerank' scores the candidates with req.query alone (retrieval_backend.py:333): "
                             "it does not combine with dense_expanded=True")
        # dense_collapse: the dense channel returns the best DOCUMENTS, each by its best row (DenseIndex.search_collapsed),
        # instead of the best rows.  A row field name ("title"), a callable row -> hashable, or a "pkg.mod:func" string
        # resolved like dense_row_filter gives every row its document
        if isinstance(dense_collapse, str) and ":" in dense_collapse:
            from .adapter import import_from_string
            dense_collapse = import_from_string(dense_collapse)
        if dense_collapse is not None and not isinstance(dense_collapse, str) and not callable(dense_collapse):
            raise TypeError(f"dense_collapse must be a row field name, a callable or a 'pkg.mod:func' string, got {type(dense_collapse)}")
        if dense_collapse is not None and (dense_mode == "rerank" or dense_row_filter is not None or self.dense_expanded):
            raise ValueError("dense_collapse does not combine with dense_mode='rerank', dense_row_filter or dense_expanded=True")
        self.dense_collapse = dense_collapse
        # graph_channel="neighbors": the reference's graph channel (retrieval_backend.py:134-182, graph_utils.py:58-129)
        # over the corpus rows, on the device (DenseIndex.expand_neighbors): the sentences within graph_window rows of the
        # request's leading graph_seed_k dense hits (None: its top_k), inside their own document.  graph_doc names every
        # row's document like dense_collapse does (a row field, a callable or a "pkg.mod:func" string); the index holds ONE
        # key array, so with dense_collapse both must name the same keys
        if graph_channel not in (None, "neighbors"):
            raise ValueError(f"unknown graph_channel {graph_channel!r} (supported: 'neighbors')")
        if graph_channel is not None and graph_expand is not None:
            raise ValueError("graph_channel and an injected graph_expand both fill the graph channel: give one")
        if graph_channel is not None and dense_mode == "rerank":
            raise ValueError("graph_channel seeds from the corpus-wide dense search: it does not combine with dense_mode='rerank'")
        if isinstance(graph_doc, str) and ":" in graph_doc:
            from .adapter import import_from_string
            graph_doc = import_from_string(graph_doc)
        if not isinstance(graph_doc, str) and not callable(graph_doc):
            raise TypeError(f"graph_doc must be a row field name, a callable or a 'pkg.mod:func' string, got {type(graph_doc)}")
        if graph_channel is not None and dense_collapse is not None and graph_doc != dense_collapse:
            raise ValueError("graph_doc and dense_collapse must name the same row keys: the index holds one key array")
        if isinstance(graph_window, bool) or not isinstance(graph_window, int) or graph_window < 0:
            raise ValueError(f"graph_window must be a non-negative integer, got {graph_window!r}")
        if graph_seed_k is not None and (isinstance(graph_seed_k, bool) or not isinstance(graph_seed_k, int) or graph_seed_k < 1):
            raise ValueError(f"graph_seed_k must be a positive integer or None, got {graph_seed_k!r}")
        self.graph_channel, self.graph_window, self.graph_seed_k, self.graph_doc = graph_channel, graph_window, graph_seed_k, graph_doc
        self._state = None

    def _row_keys(self, state, by):
        """The row keys ``by`` (a row field or a callable) gives the state's rows -> ``(keys, distinct keys, max rows per
        key)``: built once per state and per ``by``, and set on the (shared) index unless it already holds that array."""
        from .index import row_keys_of
        made = state.setdefault("collapse_keys", {})
        if by not in made:
            made[by] = row_keys_of([by(r) if callable(by) else r.get(by) for r in state["rows"]])
        entry = made[by]
        if state.get("collapse_on_index") is not entry[0]:
            state["index"].set_row_keys(entry[0])
            state["collapse_on_index"] = entry[0]
        return entry

    def _collapse_keys(self, state):
        """:meth:`_row_keys` of ``dense_collapse``"""
        return self._row_keys(state, self.dense_collapse)

    # -- graph_channel="neighbors" ------------------------------------------------------------------------------------------
    def _graph_window_of(self, req) -> int:
        """the request's own integer ``graph_window``, else the backend's (retrieval_backend.py:318-324, :156)"""
        gw = getattr(req, "graph_window", None)
        return max(0, int(gw if isinstance(gw, int) else self.graph_window))

    def _graph_seeds_of(self, top_k: int, window: int) -> int:
        """how many leading dense hits seed the expansion: ``graph_seed_k`` or the request's ``top_k``, inside the call's limits"""
        k = top_k if self.graph_seed_k is None else self.graph_seed_k
        return max(0, min(int(k), 256, 4096 // (2 * window + 1)))

    def _graph_expand_rows(self, state, seeds: np.ndarray, window: int, m: int):
        """ONE ``expand_neighbors`` call over the seed rows [n, s] -> (ids [n, m], dist [n, m]) under ``graph_doc``'s keys"""
        self._row_keys(state, self.graph_doc)
        _, ids, dist, _ = state["index"].expand_neighbors(np.ascontiguousarray(seeds, dtype=np.int64), window, m=m, return_from=True)
        return ids, dist

    @staticmethod
    def _graph_hits(rows, ids, dist, window: int) -> List[Dict[str, Any]]:
        """one result row of the expansion as the graph channel's hits (retrieval_backend.py:168-175): the score is the
        reference's own fp64 decay value of the distance, the meta the row's plus ``distance``"""
        from .index import reference_decay
        decay = reference_decay(window)
        return [{"id": _fusion.raw_hit_id(rows[i]), "score": float(decay[d]),
                 "meta": dict(_fusion.row_meta(rows[i], "graph"), distance=int(d))}
                for i, d in zip(np.asarray(ids).tolist(), np.asarray(dist).tolist()) if i >= 0]

    # -- corpus index: built once per (file signature, model), shared process-wide --------------
    def _embed_texts(self, texts: List[str], model_hint: str, trace_id: str, dim: Optional[int] = None) -> np.ndarray:
        """Embed through the router, one call per ``embed_batch`` texts, and VALIDATE every batch.  The
        router answers ``[[0.0]*3]*n`` instead of raising when the provider fails (llm_router.py:119-129):
        such a batch (wrong row count, a dim that differs from the first batch / ``dim``, or all zeros)
        must never be built into -- or cached as -- the corpus index, so it raises here."""
        out = []
        for lo in range(0, len(texts), self.embed_batch):
            chunk = texts[lo:lo + self.embed_batch]
            got = np.asarray(_vectors(self.router.embed(model_hint=model_hint, texts=chunk,
                                                        require={"trace_id": trace_id})), dtype=np.float32)
            if got.ndim != 2 or got.shape[0] != len(chunk):
                raise ValueError(f"embed batch at row {lo}: expected {len(chunk)} vectors, got shape {got.shape}")
            if dim is None:
                dim = int(got.shape[1])
            if got.shape[1] != dim or dim == 0:
                raise ValueError(f"embed batch at row {lo}: dim {got.shape[1]}, expected {dim}")
            if not np.isfinite(got).all():
                raise ValueError(f"embed batch at row {lo}: non-finite values")
            if not got.any():
                raise ValueError(f"embed batch at row {lo}: all-zero vectors (the router's failure fallback)")
            out.append(got)
        return np.concatenate(out, axis=0) if out else np.zeros((0, dim or 0), dtype=np.float32)

    def _bulk_provider(self):
        """The provider ``router.embed`` would call (llm_router.py:103-115 / retrieval_backend.py:203-206:
        ``router.providers[policy["embedding_provider"]]``) when it offers the bulk device form, else None."""
        if not self.bulk_ingest:
            return None
        try:
            policy = getattr(self.router, "policy", {}) or {}
            name = policy.get("embedding_provider")
            prov = (getattr(self.router, "providers", {}) or {}).get(name) if name else None
            return prov if prov is not None and hasattr(prov, "embed_device") else None
        except Exception:
            return None

    def _bulk_build(self, prov, ix, texts: List[str], dim: int) -> None:
        """texts -> encoder (large length-sorted batches) -> DenseIndex.add, device to device.  Validated like the
        router path (row count, dim, finite, not all-zero) chunk by chunk BEFORE the rows enter the index."""
        import torch
        step = 65536
        for lo in range(0, len(texts), step):
            chunk = texts[lo:lo + step]
            emb = prov.embed_device(chunk, batch_size=self.bulk_batch)
            if tuple(emb.shape) != (len(chunk), dim):
                raise ValueError(f"bulk embed at row {lo}: expected {(len(chunk), dim)}, got {tuple(emb.shape)}")
            ok = torch.stack([torch.isfinite(emb).all(), emb.any()]).cpu().tolist()      # one sync per 65 536 rows
            if not ok[0]:
                raise ValueError(f"bulk embed at row {lo}: non-finite values")
            if not ok[1]:
                raise ValueError(f"bulk embed at row {lo}: all-zero vectors")
            ix.add(emb)                                                                    # K1: fp64 norm, ONE rounding

    def _build_state(self, model_hint: str, trace_id: str):
        import time
        from .index import DenseIndex
        t_start = time.perf_counter()
        rows = _corpus.read_docs_jsonl(self.index_path)
        state = {"rows": rows, "index": None, "dim": 0, "row_of": {}}
        if not rows:
            return state
        texts = [r.get("text") or "" for r in rows]
        probe = self._embed_texts(texts[:1], model_hint, trace_id)
        dim = int(probe.shape[1])
        cache = _corpus.EmbeddingCache(self.cache_dir) if self.cache_dir else None
        bits, key = None, None
        if cache is not None:
            key = cache.key(self.index_path, model_hint, dim, self.index_dtype)
            bits = cache.load(key)
            if bits is not None and (bits.shape != (len(rows), dim) or bits.dtype != np.uint16):
                bits = None
        ix = DenseIndex(dim, metric="cosine", dtype=self.index_dtype, device=self.device)
        step = 131072
        if bits is not None:
            # warm start: the cache holds the 16-bit patterns K1 produced in the cold build; they are
            # re-added verbatim, so cold and warm indexes are bit-identical (doc-id order near ties
            # cannot depend on the cache state)
            for lo in range(0, len(rows), step):
                ix.add_stored_bits(np.ascontiguousarray(bits[lo:lo + step]))
        else:
            prov, how = self._bulk_provider(), "router"
            if prov is not None:
                try:
                    self._bulk_build(prov, ix, texts, dim)
                    how = "bulk"
                except Exception as e:          # the router path is the reference behaviour: fall back to it, loudly
                    logger.error("[DenseRetrievalBackend] bulk ingest failed (%s); rebuilding through router.embed", e)
                    ix.close()
                    ix = DenseIndex(dim, metric="cosine", dtype=self.index_dtype, device=self.device)
            if how == "router":
                emb = self._embed_texts(texts, model_hint, trace_id, dim=dim)
                for lo in range(0, len(rows), step):
                    ix.add(np.ascontiguousarray(emb[lo:lo + step]))       # K1: fp64 norm, ONE rounding
            state["ingest"] = how
            if cache is not None:
                cache.store(key, ix.stored_bits(), {"model": model_hint, "rows": len(rows), "dim": dim,
                                                    "dtype": self.index_dtype, "format": "storage bits (uint16)",
                                                    "docs": _corpus.file_signature(self.index_path)})
        state["index"], state["dim"] = ix, dim
        # raw hit id (retrieval_backend.py:116-119) -> corpus row, for the re-ranker's lookup by id; ids that
        # occur twice (duplicate doc_id lines) are ambiguous and left out: such candidates are embedded as before
        seen: Dict[str, int] = {}
        for r in rows:
            hid = _fusion.raw_hit_id(r)
            seen[hid] = seen.get(hid, 0) + 1
        row_of: Dict[str, int] = {}
        for i, r in enumerate(rows):
            hid = _fusion.raw_hit_id(r)
            if seen[hid] == 1:
                row_of[hid] = i
        state["row_of"] = row_of
        self.last_build = {"rows": len(rows), "dim": dim, "ingest": state.get("ingest", "cache"),
                           "seconds": time.perf_counter() - t_start}
        return state

    def _bm25_searcher(self):
        from .text_index import HipBM25Index, HipBM25TextSearcher
        try:
            sig = _corpus.file_signature(self.index_path)
        except OSError:
            sig = f"{self.index_path}|missing"
        key = f"bm25-index|{sig}|{self.device}|{self.bm25_k1}|{self.bm25_b}"
        ix = _corpus.shared(key, lambda: HipBM25Index(self.index_path, k1=self.bm25_k1, b=self.bm25_b, device=self.device))
        self._own_text_search = HipBM25TextSearcher(ix)    # run_batch reads its document positions as corpus rows
        return self._own_text_search

    _FAIL_BACKOFF_S = 30.0
    _failed: Dict[str, Any] = {}        # key -> (monotonic deadline, error text): no re-embed storm after a failed build

    def _get_state(self, model_hint: str, trace_id: str):
        if self._state is None:
            import time
            try:
                sig = _corpus.file_signature(self.index_path)
            except OSError:
                sig = f"{self.index_path}|missing"
            key = f"dense-index|{sig}|{model_hint}|{self.device}|{self.index_dtype}"
            bad = DenseRetrievalBackend._failed.get(key)
            if bad and time.monotonic() < bad[0]:
                raise RuntimeError(f"corpus index build failed {self._FAIL_BACKOFF_S:.0f}s ago or less: {bad[1]}")
            try:
                self._state = _corpus.shared(key, lambda: self._build_state(model_hint, trace_id))
            except Exception as e:
                DenseRetrievalBackend._failed[key] = (time.monotonic() + self._FAIL_BACKOFF_S, repr(e))
                raise
            DenseRetrievalBackend._failed.pop(key, None)
        return self._state

    # -- the backend protocol ---------------------------------------------------------------------
    def _expand(self, req, trace_id: str):
        """The reference's Expand step (retrieval_backend.py:307-310) -> (``[req.query] + expanded``, error text or None).
        Without a ``query_expander`` there is no step and no span; an expander that raises is logged and the request
        runs with ``[req.query]``."""
        if self.query_expander is None:
            return [req.query], None
        with span("Backend/Expand", self.sink, trace_id):
            try:
                expanded = self.query_expander(query=req.query, trace_id=trace_id)
                return [req.query] + [str(q) for q in (expanded or [])], None
            except Exception as e:
                logger.error("[DenseRetrievalBackend] query expansion failed: %s", e)
                return [req.query], repr(e)

    def run(self, req) -> Dict[str, Any]:
        trace_id = getattr(req, "trace_id", None) or "trace-demo"                       # :304
        top_k = int(getattr(req, "top_k", None) or self.default_top_k)                  # :305
        model_hint = resolve_embed_model(self.router)
        pool = max(top_k, self.dense_pool_k)
        queries, expand_error = self._expand(req, trace_id)

        t_hits: List[Dict[str, Any]] = []
        g_hits: List[Dict[str, Any]] = []
        text_error = None
        if self.text_search is None and self.text_channel == "bm25":
            try:
                self.text_search = self._bm25_searcher()
            except Exception as e:     # degrade like the dense channel: report, keep serving the other channels
                text_error = repr(e)
                logger.error("[DenseRetrievalBackend] BM25 channel unavailable: %s", e)
        rerank = self.dense_mode == "rerank"
        own = rerank and self._is_own_searcher()
        t_docs: List[int] = []                           # rerank over the own searcher: the hits' document positions
        if self.text_search is not None:
            with span("Backend/TextSearch", self.sink, trace_id):
                if own:
                    ranked = (self.text_search.index.search(queries, top_k=pool, alpha_merge="max")
                              if self.text_search.index.N > 0 else [])
                    t_docs = [int(d) for d, _ in ranked]
                    t_hits = self.text_search._hits(ranked)
                else:
                    t_hits = list(self.text_search(queries=queries, top_k=pool) or [])
        if self.graph_expand is not None:
            with span("Backend/GraphExpand", self.sink, trace_id):
                g_hits = list(self.graph_expand(query=req.query, graph_id=getattr(req, "graph_id", "") or "",
                                                top_k=pool) or [])

        dense_hits: List[Dict[str, Any]] = []
        dense_error = None
        dense_filter = None
        dense_collapse = None
        dense_rows = None                                # the dense list's row ids, the seeds of graph_channel="neighbors"
        state = None
        k_eff = 0
        with span("Backend/DenseRerank", self.sink, trace_id):      # same span name as :332
            try:
                state = None if rerank else self._get_state(model_hint, trace_id)
                if rerank and t_hits:
                    dense_hits = self._rerank_one(req, t_hits[:pool], t_docs[:pool] if own else None, pool, model_hint, trace_id)
                    k_eff = len(dense_hits)
                if state is not None and state["index"] is not None and self.dense_expanded:
                    # every query of the request, max-merged per row on the device: one group
                    Qv = self._embed_texts(queries, model_hint, trace_id, dim=state["dim"])
                    k_eff = min(pool, len(state["rows"]), state["index"].max_k(1))
                    allow = self.dense_row_filter(req, state["rows"]) if self.dense_row_filter is not None else None
                    sc, ids = state["index"].search_groups(Qv, k_eff, sizes=[len(queries)], allow=allow)
                    if allow is not None:
                        dense_filter = state["index"].last_filter()
                    dense_hits = self._dense_hits(state["rows"], sc[0], ids[0])
                    dense_rows = ids[0]
                elif state is not None and state["index"] is not None:
                    qv = np.asarray(_vectors(self.router.embed(model_hint=model_hint, texts=[req.query],
                                                               require={"trace_id": trace_id}))[0], dtype=np.float32)
                    if qv.shape[0] != state["dim"]:
                        raise ValueError(f"query embedding has dim {qv.shape[0]}, corpus has {state['dim']}")
                    # the reference scores its whole pool (retrieval_backend.py:218,245); the index serves
                    # k up to max_k() (256) -- anything beyond is reported, never silently dropped
                    k = min(pool, len(state["rows"]))
                    k_eff = min(k, state["index"].max_k(1))
                    allow = self.dense_row_filter(req, state["rows"]) if self.dense_row_filter is not None else None
                    if self.dense_collapse is not None:      # the best documents, each by its best row
                        _, n_keys, m = self._collapse_keys(state)
                        k_eff = min(pool, n_keys, state["index"].max_k(1))
                        sc, ids = state["index"].search_collapsed(qv[None, :], k_eff, return_keys=False)
                        lc = state["index"].last_collapsed()
                        dense_collapse = {"keys": n_keys, "max_rows_per_key": m, "scan_k": lc["scan_k"], "redone": lc["redone_queries"]}
                    elif allow is None:
                        sc, ids = state["index"].search(qv[None, :], k_eff)
                    else:
                        sc, ids = state["index"].search(qv[None, :], k_eff, allow=allow)
                        dense_filter = state["index"].last_filter()
                    dense_hits = self._dense_hits(state["rows"], sc[0], ids[0])
                    dense_rows = ids[0]
            except Exception as e:     # reference policy: degrade, never raise out of run() (:229-231)
                dense_error = repr(e)
                logger.error("[DenseRetrievalBackend] dense channel failed: %s", e)

        # the device graph channel: the neighbours of the leading dense hits inside their documents (after the dense search,
        # which gives the seeds; the reference's step 3, retrieval_backend.py:317-329)
        graph_error = None
        graph_info = None
        if self.graph_channel is not None:
            window = self._graph_window_of(req)
            with span("Backend/GraphExpand", self.sink, trace_id):
                try:
                    if dense_error is not None:
                        raise RuntimeError(f"no seeds, the dense channel failed: {dense_error}")
                    n_seeds = min(self._graph_seeds_of(top_k, window), len(dense_rows)) if dense_rows is not None else 0
                    if n_seeds > 0:
                        g_ids, g_dist = self._graph_expand_rows(state, np.asarray(dense_rows[:n_seeds])[None, :], window, min(pool, 4096))
                        g_hits = self._graph_hits(state["rows"], g_ids[0], g_dist[0], window)
                    graph_info = {"seeds": n_seeds, "window": window, "max_entries": n_seeds * (2 * window + 1)}
                except Exception as e:
                    graph_error = repr(e)
                    g_hits = []
                    logger.error("[DenseRetrievalBackend] graph channel failed: %s", e)

        # dense hits double as candidates (their meta gives the normalised id); scores fused per :350-372
        dense_norm_hits = _fusion.dedupe_by_norm_id(dense_hits)
        dense_scores = {nid: h["score"] for nid, h in dense_norm_hits.items()}
        fuse = _fusion.fuse_channels
        if self.fuse_on_device and len(t_hits) + len(g_hits) + len(dense_scores) <= 4096:
            fuse = lambda *a, **kw: _fusion.fuse_channels_device(*a, device=self.device, **kw)    # noqa: E731
        fused = fuse(t_hits, g_hits, dense_scores, alpha_text=self.alpha_text,
                     alpha_graph=self.alpha_graph, alpha_dense=self.alpha_dense, top_k=10 ** 9)
        for h in fused:                                   # dense-only ids carry their own meta
            if not h["meta"].get("text") and h["id"] in dense_norm_hits:
                meta = dict(dense_norm_hits[h["id"]]["meta"])
                meta.update({k: v for k, v in h["meta"].items() if k.startswith("score_")})
                h["meta"] = meta
        fused = fused[:top_k]
        diagnostics = {
            "queries": queries,
            "bm25_candidates": len(t_hits),
            "graph_candidates": len(g_hits),
            "dense_scored": len(dense_scores),
            "weights": {"alpha_text": self.alpha_text, "alpha_graph": self.alpha_graph, "alpha_dense": self.alpha_dense},
            "pool": {"dense_pool_k": self.dense_pool_k, "final_top_k": top_k, "dense_pool_k_effective": k_eff},
            "resolved_embed_model": model_hint,
            "dense_backend": "mrag_amd.DenseIndex",
            "dense_error": dense_error,
            "text_error": text_error,
        }
        if rerank:
            diagnostics["dense_mode"] = "rerank"
        if dense_filter is not None:
            diagnostics["dense_filter"] = dense_filter
        if dense_collapse is not None:
            diagnostics["dense_collapse"] = dense_collapse
        if expand_error is not None:
            diagnostics["expand_error"] = expand_error
        if self.graph_channel is not None:
            diagnostics["graph_window_used"] = window
            if graph_info is not None:
                diagnostics["graph_channel"] = graph_info
            if graph_error is not None:
                diagnostics["graph_error"] = graph_error
        return {"hits": fused, "diagnostics": diagnostics}

    @staticmethod
    def _dense_hits(rows, scores, ids) -> List[Dict[str, Any]]:
        """one result row of a dense search as the dense channel's hits; the (-inf, -1) slots are left out"""
        return [{"id": _fusion.raw_hit_id(rows[int(i)]), "score": float(s), "meta": _fusion.row_meta(rows[int(i)], "dense")}
                for s, i in zip(scores, ids) if i >= 0]

    # -- dense_mode="rerank": the dense channel scores the text channel's candidates ------------------------------------
    def _is_own_searcher(self) -> bool:
        """The text channel is the BM25 searcher this backend made over ``index_path``: its document positions are then
        the dense state's rows (both read the file's non-empty lines in order)."""
        return self.text_channel == "bm25" and self.text_search is not None and self.text_search is self._own_text_search

    def _rows_are_docs(self, state) -> bool:
        return state["index"] is not None and len(self.text_search.index.docs) == len(state["rows"])

    @staticmethod
    def _scored_hits(cands: List[Dict[str, Any]], scores: Dict[str, float]) -> List[Dict[str, Any]]:
        """The re-ranker's ``{raw id: score}`` as dense hits that carry the candidates' meta, so that they are keyed by
        normalised id like the text hits (the backend's fusion convention; the reference's raw-id keying, SURVEY a7,
        stays consciously fixed)."""
        return [{"id": h["id"], "score": float(scores[h["id"]]), "meta": dict(h.get("meta") or {})}
                for h in cands if h.get("id") in scores]

    def _rerank_one(self, req, cands, docs, pool: int, model_hint: str, trace_id: str) -> List[Dict[str, Any]]:
        """The dense hits of one request in rerank mode.  ``docs`` (own searcher): the candidates' document positions --
        they are scored as corpus rows by ``score_rows``, rows whose ``doc_id`` occurs twice in the file included, and
        nothing is re-embedded.  Otherwise (injected searcher) the candidates go through :class:`HipDenseReranker` with
        this backend as its corpus.  :meth:`run_batch` makes the same choice, so both score the same thing."""
        if docs is not None:
            state = self._get_state(model_hint, trace_id)
            if self._rows_are_docs(state):
                qv = self._embed_texts([req.query], model_hint, trace_id, dim=state["dim"])[0]      # validated as run_batch's
                sc = state["index"].score_rows(qv, np.asarray(docs, dtype=np.int64))
                rows = state["rows"]
                return [{"id": _fusion.raw_hit_id(rows[d]), "score": float(s), "meta": _fusion.row_meta(rows[d], "dense")}
                        for d, s in zip(docs, sc)]
        rr = HipDenseReranker(self.router, max_pool=pool, embed_batch=self.embed_batch, device=self.device, corpus=self)
        return self._scored_hits(cands, rr.score(query=req.query, candidates=cands, trace_id=trace_id))

    def retrieve(self, req) -> RetrievalOut:
        result = self.run(req)
        hits = [Hit(id=h["id"], score=h["score"], meta=h.get("meta") or {}) for h in result["hits"]]
        return RetrievalOut(hits=hits, diagnostics=result.get("diagnostics", {}))

    # -- the same protocol for a list of requests: one dense search, one BM25 batch search, one fusion launch ------------
    def _norm_keys(self, state):
        """``fusion.corpus_norm_keys`` of the state's rows, built once per state and kept in it."""
        if "norm_keys" not in state:
            state["norm_keys"] = _fusion.corpus_norm_keys(state["rows"])
        return state["norm_keys"]

    def run_batch(self, reqs) -> List[Dict[str, Any]]:
        """:meth:`run` for every request of ``reqs``, in order, with the device work of the whole list in three calls:
        one ``DenseIndex.search`` over all query embeddings, one ``HipBM25Index.search_batch`` (``text_channel="bm25"``)
        and one ``mrag_fuse_topk_batch``.  ``top_k``, ``trace_id`` and the pool are each request's own: the searches run
        at the list's largest pool and every question uses the leading part of its lists that its own pool covers (both
        searches are exact with a declared order, so a prefix is the smaller search's answer).  Requests for which
        ``dense_row_filter`` returns a set are searched one by one with their ``allow`` -- or, with
        ``dense_filter_batch=True``, all together in one ``DenseIndex.search_sets`` call in which sets of equal content
        are shared and whose diagnostics read ``dense_filter = {"path": "sets", "allowed": m}``; an injected ``text_search`` and
        ``graph_expand`` are called once per request.  Like :meth:`run` it degrades and never raises out of the dense
        channel.  Diagnostics are :meth:`run`'s plus ``batch_size``.  With ``dense_mode="rerank"`` the dense search is
        replaced by one ``DenseIndex.score_rows_batch`` over every question's leading text candidates (own BM25 searcher)
        or one ``HipDenseReranker.score_batch`` (injected searcher): :meth:`_rerank_batch`.  With a ``query_expander``
        every request is expanded first (``Backend/Expand``) and the text channel receives each request's list; with
        ``dense_expanded=True`` the dense channel embeds all of those queries and makes ONE ``DenseIndex.search_groups``
        call over the unfiltered requests and one per filtered request (``dense_filter_batch`` then has no effect).
        With ``dense_collapse`` the dense search is ONE ``DenseIndex.search_collapsed`` over all requests at the list's
        largest pool -- one hit per document, a prefix per request -- and ``diagnostics["dense_collapse"]`` describes
        that call.  With ``graph_channel="neighbors"`` the graph channel is ONE ``DenseIndex.expand_neighbors`` call per
        distinct ``graph_window`` of the list (normally one) over every request's leading dense hits, and the array
        path carries its rows into the fusion launch."""
        from .index import pack_sets
        from .text_index import HipBM25TextSearcher
        reqs = list(reqs)
        B = len(reqs)
        if not B:
            return []
        model_hint = resolve_embed_model(self.router)
        trace = [getattr(r, "trace_id", None) or "trace-demo" for r in reqs]
        top_k = [int(getattr(r, "top_k", None) or self.default_top_k) for r in reqs]
        pool = [max(k, self.dense_pool_k) for k in top_k]
        pool_max = max(pool)
        expanded = [self._expand(r, trace[g]) for g, r in enumerate(reqs)]
        queries = [e[0] for e in expanded]

        # ---- text and graph channels
        text_error = None
        if self.text_search is None and self.text_channel == "bm25":
            try:
                self.text_search = self._bm25_searcher()
            except Exception as e:
                text_error = repr(e)
                logger.error("[DenseRetrievalBackend] BM25 channel unavailable: %s", e)
        bm25 = self.text_channel == "bm25" and isinstance(self.text_search, HipBM25TextSearcher)
        # only the searcher made here over index_path numbers its documents as the dense state numbers its rows (both read
        # the file's non-empty lines in order); an injected one, even of the same length, is fused by id strings
        own = bm25 and self.text_search is self._own_text_search
        t_arrays = None                                  # bm25: (docs [B][k], scores [B][k], n [B]) of the batch search
        t_hits: List[List[Dict[str, Any]]] = [[] for _ in reqs]
        g_hits: List[List[Dict[str, Any]]] = [[] for _ in reqs]
        if bm25:
            with span("Backend/TextSearch", self.sink, trace[0]):
                if self.text_search.index.N > 0:
                    t_arrays = self.text_search.index.search_batch_arrays(queries, top_k=pool_max,
                                                                          alpha_merge="max")
        elif self.text_search is not None:
            for g, r in enumerate(reqs):
                with span("Backend/TextSearch", self.sink, trace[g]):
                    t_hits[g] = list(self.text_search(queries=queries[g], top_k=pool[g]) or [])
        if self.graph_expand is not None:
            for g, r in enumerate(reqs):
                with span("Backend/GraphExpand", self.sink, trace[g]):
                    g_hits[g] = list(self.graph_expand(query=r.query, graph_id=getattr(r, "graph_id", "") or "",
                                                       top_k=pool[g]) or [])

        # ---- dense channel: d_ids / d_sc [B][kd], (-1, -inf) where a request has no row
        dense_error: List[Optional[str]] = [None] * B
        dense_filter: List[Any] = [None] * B
        dense_collapse = None
        k_eff = [0] * B
        state = None
        d_ids = np.full((B, 0), -1, dtype=np.int64)
        d_sc = np.full((B, 0), -np.inf, dtype=np.float32)
        rerank = self.dense_mode == "rerank"
        rr_hits: Optional[List[List[Dict[str, Any]]]] = None      # rerank through HipDenseReranker: the dense hits per request
        with span("Backend/DenseRerank", self.sink, trace[0]):
            try:
                if rerank:
                    state, d_ids, d_sc, k_eff, dense_error, rr_hits = self._rerank_batch(reqs, pool, trace, model_hint,
                                                                                         t_arrays, t_hits)
                else:
                    state = self._get_state(model_hint, trace[0])
                if not rerank and state["index"] is not None:
                    ix, rows = state["index"], state["rows"]
                    if self.dense_expanded:              # every query of every request: request g owns Q[qp[g]:qp[g + 1]]
                        qp = np.zeros(B + 1, dtype=np.int64)
                        np.cumsum([len(q) for q in queries], out=qp[1:])
                        Q = self._embed_texts([q for qs in queries for q in qs], model_hint, trace[0], dim=state["dim"])
                    else:
                        Q = self._embed_texts([r.query for r in reqs], model_hint, trace[0], dim=state["dim"])
                    k_one, k_many = ix.max_k(1), ix.max_k(B)
                    d_ids = np.full((B, max(min(pool_max, len(rows)), 0)), -1, dtype=np.int64)
                    d_sc = np.full(d_ids.shape, -np.inf, dtype=np.float32)
                    plain = []
                    in_sets: List[int] = []                  # dense_filter_batch: the requests that share the search_sets call
                    set_index: Dict[bytes, int] = {}         # ... the distinct sets by content -> position in set_list
                    set_list: List[np.ndarray] = []
                    set_of: List[int] = []
                    for g, r in enumerate(reqs):
                        try:
                            allow = self.dense_row_filter(r, rows) if self.dense_row_filter is not None else None
                            if allow is None:
                                plain.append(g)
                                continue
                            k_eff[g] = min(pool[g], len(rows), k_one)
                            if self.dense_expanded:          # one grouped search per filtered request, as run()
                                sc, ids = ix.search_groups(Q[qp[g]:qp[g + 1]], k_eff[g], sizes=[len(queries[g])], allow=allow)
                                dense_filter[g] = ix.last_filter()
                                d_sc[g, :k_eff[g]], d_ids[g, :k_eff[g]] = sc[0], ids[0]
                                continue
                            if self.dense_filter_batch:
                                set_rows = pack_sets([allow], len(rows))[1]
                                key = set_rows.tobytes()
                                if key not in set_index:
                                    set_index[key] = len(set_list)
                                    set_list.append(set_rows)
                                in_sets.append(g)
                                set_of.append(set_index[key])
                                continue
                            sc, ids = ix.search(Q[g:g + 1], k_eff[g], allow=allow)
                            dense_filter[g] = ix.last_filter()
                            d_sc[g, :k_eff[g]], d_ids[g, :k_eff[g]] = sc[0], ids[0]
                        except Exception as e:
                            dense_error[g] = repr(e)
                            d_ids[g] = -1
                            logger.error("[DenseRetrievalBackend] dense channel failed for request %d: %s", g, e)
                    if in_sets:
                        try:
                            sc, ids = ix.search_sets(Q[in_sets], max(k_eff[g] for g in in_sets), set_list,
                                                     set_of=np.asarray(set_of, dtype=np.int32))
                            for j, g in enumerate(in_sets):
                                d_sc[g, :k_eff[g]], d_ids[g, :k_eff[g]] = sc[j, :k_eff[g]], ids[j, :k_eff[g]]
                                dense_filter[g] = {"path": "sets", "allowed": int(set_list[set_of[j]].shape[0])}
                        except Exception as e:
                            for g in in_sets:
                                dense_error[g] = repr(e)
                                d_ids[g] = -1
                            logger.error("[DenseRetrievalBackend] dense channel failed for the filtered requests: %s", e)
                    if plain and self.dense_expanded:
                        # ONE grouped search at the largest pool; a request whose queries x that pool exceed the merge's
                        # 4096 entries is searched alone at its own pool, where run() would succeed or fail as well
                        k_batch = min(max(pool[g] for g in plain), len(rows), k_many)
                        alone = [g for g in plain if len(queries[g]) * k_batch > 4096]
                        plain = [g for g in plain if len(queries[g]) * k_batch <= 4096]
                        for g in alone:
                            try:
                                k_eff[g] = min(pool[g], len(rows), k_one)
                                sc, ids = ix.search_groups(Q[qp[g]:qp[g + 1]], k_eff[g], sizes=[len(queries[g])])
                                d_sc[g, :k_eff[g]], d_ids[g, :k_eff[g]] = sc[0], ids[0]
                            except Exception as e:
                                dense_error[g] = repr(e)
                                d_ids[g] = -1
                                logger.error("[DenseRetrievalBackend] dense channel failed for request %d: %s", g, e)
                        if plain:
                            try:
                                rows_of = np.concatenate([np.arange(qp[g], qp[g + 1]) for g in plain])
                                sc, ids = ix.search_groups(Q[rows_of], k_batch, sizes=[len(queries[g]) for g in plain])
                                for j, g in enumerate(plain):
                                    k_eff[g] = min(pool[g], k_batch)
                                    d_sc[g, :k_eff[g]], d_ids[g, :k_eff[g]] = sc[j, :k_eff[g]], ids[j, :k_eff[g]]
                            except Exception as e:
                                for g in plain:
                                    dense_error[g] = repr(e)
                                    d_ids[g] = -1
                                logger.error("[DenseRetrievalBackend] dense channel failed: %s", e)
                    elif plain:
                        try:
                            k_batch = min(max(pool[g] for g in plain), len(rows), k_many)
                            if self.dense_collapse is not None:      # ONE collapsed search at the largest pool, a prefix each
                                _, n_keys, m = self._collapse_keys(state)
                                k_batch = min(max(pool[g] for g in plain), n_keys, k_many)
                                sc, ids = ix.search_collapsed(Q, k_batch, return_keys=False)
                                lc = ix.last_collapsed()
                                dense_collapse = {"keys": n_keys, "max_rows_per_key": m, "scan_k": lc["scan_k"],
                                                  "redone": lc["redone_queries"]}
                            else:
                                sc, ids = ix.search(Q[plain] if len(plain) < B else Q, k_batch)
                            for j, g in enumerate(plain):
                                k_eff[g] = min(pool[g], k_batch)
                                d_sc[g, :k_eff[g]], d_ids[g, :k_eff[g]] = sc[j, :k_eff[g]], ids[j, :k_eff[g]]
                        except Exception as e:
                            for g in plain:
                                dense_error[g] = repr(e)
                                d_ids[g] = -1
                            logger.error("[DenseRetrievalBackend] dense channel failed: %s", e)
            except Exception as e:     # reference policy: degrade, never raise out of run() (:229-231)
                dense_error = [repr(e)] * B
                d_ids = np.full((B, 0), -1, dtype=np.int64)
                d_sc = np.full((B, 0), -np.inf, dtype=np.float32)
                logger.error("[DenseRetrievalBackend] dense channel failed: %s", e)

        # ---- device graph channel: ONE expand_neighbors call per distinct window of the batch (normally one); a request's
        # seed row is padded with -1 beyond its own seeds, which changes nothing of its result
        graph_on = self.graph_channel is not None
        g_win = [self._graph_window_of(r) for r in reqs] if graph_on else [0] * B
        g_error: List[Optional[str]] = [None] * B
        g_info: List[Any] = [None] * B
        g_n = np.zeros(B, dtype=np.int64)                # graph hits per request: the leading slots of g_rows / g_dist
        g_rows = np.full((B, min(pool_max, 4096) if graph_on else 0), -1, dtype=np.int64)
        g_dist = np.full(g_rows.shape, -1, dtype=np.int32)
        if graph_on:
            with span("Backend/GraphExpand", self.sink, trace[0]):
                have = state is not None and state["index"] is not None and d_ids.shape[1] > 0
                n_seeds = [0] * B
                for g in range(B):
                    if dense_error[g] is not None:
                        g_error[g] = repr(RuntimeError(f"no seeds, the dense channel failed: {dense_error[g]}"))
                    elif have:
                        n_seeds[g] = min(self._graph_seeds_of(top_k[g], g_win[g]), k_eff[g])
                for w in sorted({g_win[g] for g in range(B) if n_seeds[g] > 0}):
                    grp = [g for g in range(B) if n_seeds[g] > 0 and g_win[g] == w]
                    try:
                        seeds = np.full((len(grp), max(n_seeds[g] for g in grp)), -1, dtype=np.int64)
                        for j, g in enumerate(grp):
                            seeds[j, :n_seeds[g]] = d_ids[g, :n_seeds[g]]
                        ids, dist = self._graph_expand_rows(state, seeds, w, min(max(pool[g] for g in grp), 4096))
                        for j, g in enumerate(grp):
                            c = min(pool[g], 4096)       # the request's own m: a prefix of the call's (strict declared order)
                            g_rows[g, :c], g_dist[g, :c] = ids[j, :c], dist[j, :c]
                            g_n[g] = int((ids[j, :c] >= 0).sum())
                    except Exception as e:
                        for g in grp:
                            g_error[g] = repr(e)
                            g_rows[g], g_dist[g], g_n[g] = -1, -1, 0
                        logger.error("[DenseRetrievalBackend] graph channel failed: %s", e)
                for g in range(B):
                    if g_error[g] is None:
                        g_info[g] = {"seeds": n_seeds[g], "window": g_win[g], "max_entries": n_seeds[g] * (2 * g_win[g] + 1)}

        alphas = dict(alpha_text=self.alpha_text, alpha_graph=self.alpha_graph, alpha_dense=self.alpha_dense)
        fast = (own and self.graph_expand is None and state is not None and state["index"] is not None
                and (t_arrays is None or len(self.text_search.index.docs) == len(state["rows"])))
        if fast:
            norm_keys, sorted_ids = self._norm_keys(state)
            if t_arrays is None:
                t_arrays = (np.full((B, 0), -1, dtype=np.int64), np.zeros((B, 0), dtype=np.float64), np.zeros(B, dtype=np.int32))
            graph_arrays = {}
            if graph_on:                                 # the reference's own fp64 decay values, looked up by distance
                from .index import reference_decay
                g_sc = np.zeros(g_rows.shape, dtype=np.float64)
                for g in range(B):
                    g_sc[g, :g_n[g]] = reference_decay(g_win[g])[g_dist[g, :g_n[g]]]
                graph_arrays = dict(graph_rows=g_rows, graph_scores=g_sc, graph_n=g_n)
            chan_ptr, keys, scores, payload = _fusion.batch_entries(t_arrays[0], t_arrays[1], t_arrays[2], d_ids, d_sc, norm_keys,
                                                                    pool=pool, **graph_arrays)
            sizes = chan_ptr[3::3] - chan_ptr[0:-1:3]
            fast = int(sizes.max()) <= _fusion.FUSE_MAX_ENTRIES
        results = []
        if fast:
            rows = state["rows"]
            ok, osc, nt, ng, nd, op, n_out = _fusion.fuse_entries_device_batch(chan_ptr, keys, scores, payload, top_k=top_k,
                                                                              device=self.device, **alphas)
            for g in range(B):
                hits = []
                dist_of = dict(zip(g_rows[g, :g_n[g]].tolist(), g_dist[g, :g_n[g]].tolist())) if g_n[g] else {}
                for i in range(int(n_out[g])):
                    rt, rg, rd = int(op[g, i, 0]), int(op[g, i, 1]), int(op[g, i, 2])
                    meta = _fusion.row_meta(rows[rt], "bm25") if rt >= 0 else {}
                    if rg >= 0:                                    # the graph meta overlays the text meta, as fuse_channels does
                        meta.update(_fusion.row_meta(rows[rg], "graph"), distance=dist_of[rg])
                    if not meta.get("text") and rd >= 0:           # dense-only ids carry their own meta
                        meta = _fusion.row_meta(rows[rd], "dense")
                    meta["score_text_norm"], meta["score_graph_norm"], meta["score_dense_norm"] = float(nt[g, i]), float(ng[g, i]), float(nd[g, i])
                    hits.append({"id": sorted_ids[int(ok[g, i])], "score": float(osc[g, i]), "meta": meta})
                dk = keys[chan_ptr[3 * g + 2]:chan_ptr[3 * g + 3]]
                results.append((hits, int(chan_ptr[3 * g + 1] - chan_ptr[3 * g]), int(np.unique(dk).shape[0])))
        else:
            if t_arrays is not None:
                dl, sl, nl = t_arrays[0].tolist(), t_arrays[1].tolist(), t_arrays[2].tolist()
                for g in range(B):
                    c = min(nl[g], pool[g])
                    t_hits[g] = self.text_search._hits(list(zip(dl[g][:c], sl[g][:c])))
            dense_norm, questions = [], []
            for g in range(B):
                if g_n[g]:
                    g_hits[g] = self._graph_hits(state["rows"], g_rows[g, :g_n[g]], g_dist[g, :g_n[g]], g_win[g])
                dense_hits = []
                if rr_hits is not None:
                    dense_hits = rr_hits[g]
                elif state is not None:
                    for s, i in zip(d_sc[g].tolist(), d_ids[g].tolist()):
                        if i < 0:
                            continue
                        row = state["rows"][i]
                        dense_hits.append({"id": _fusion.raw_hit_id(row), "score": float(s), "meta": _fusion.row_meta(row, "dense")})
                dn = _fusion.dedupe_by_norm_id(dense_hits)
                dense_norm.append(dn)
                questions.append((t_hits[g], g_hits[g], {nid: h["score"] for nid, h in dn.items()}))
            if self.fuse_on_device:
                fused_all = _fusion.fuse_channels_device_batch(questions, top_k=10 ** 9, device=self.device, **alphas)
            else:
                fused_all = [_fusion.fuse_channels(*q, top_k=10 ** 9, **alphas) for q in questions]
            for g, fused in enumerate(fused_all):
                for h in fused:                               # dense-only ids carry their own meta
                    if not h["meta"].get("text") and h["id"] in dense_norm[g]:
                        meta = dict(dense_norm[g][h["id"]]["meta"])
                        meta.update({k: v for k, v in h["meta"].items() if k.startswith("score_")})
                        h["meta"] = meta
                results.append((fused[:top_k[g]], len(t_hits[g]), len(dense_norm[g])))

        out = []
        for g, (hits, n_text, n_dense) in enumerate(results):
            diagnostics = {
                "queries": queries[g],
                "bm25_candidates": n_text,
                "graph_candidates": int(g_n[g]) if graph_on else len(g_hits[g]),
                "dense_scored": n_dense,
                "weights": dict(alphas),
                "pool": {"dense_pool_k": self.dense_pool_k, "final_top_k": top_k[g], "dense_pool_k_effective": k_eff[g]},
                "resolved_embed_model": model_hint,
                "dense_backend": "mrag_amd.DenseIndex",
                "dense_error": dense_error[g],
                "text_error": text_error,
                "batch_size": B,
            }
            if rerank:
                diagnostics["dense_mode"] = "rerank"
            if dense_filter[g] is not None:
                diagnostics["dense_filter"] = dense_filter[g]
            if dense_collapse is not None and dense_error[g] is None:
                diagnostics["dense_collapse"] = dense_collapse
            if expanded[g][1] is not None:
                diagnostics["expand_error"] = expanded[g][1]
            if graph_on:
                diagnostics["graph_window_used"] = g_win[g]
                if g_info[g] is not None:
                    diagnostics["graph_channel"] = g_info[g]
                if g_error[g] is not None:
                    diagnostics["graph_error"] = g_error[g]
            out.append({"hits": hits, "diagnostics": diagnostics})
        return out

    def _rerank_batch(self, reqs, pool, trace, model_hint: str, t_arrays, t_hits):
        """The dense channel of :meth:`run_batch` in rerank mode: ``(state, d_ids, d_sc, k_eff, dense_error, rr_hits)``.
        Own searcher: every question's leading ``min(n, pool[g])`` documents of the batch search are scored as corpus rows
        in ONE ``score_rows_batch`` after one ``_embed_texts`` of the queries (d_ids = those documents, d_sc = their
        scores, for the ``batch_entries`` path).  Otherwise one ``HipDenseReranker.score_batch`` over the requests' text
        hits (``rr_hits``: its scores as dense hits).  The choice is :meth:`_rerank_one`'s.  Requests without candidates
        have an empty dense channel and no error; a failure is reported for the others and never raised."""
        B = len(reqs)
        state, rr_hits = None, None
        d_ids, d_sc = np.full((B, 0), -1, dtype=np.int64), np.full((B, 0), -np.inf, dtype=np.float32)
        k_eff: List[int] = [0] * B
        dense_error: List[Optional[str]] = [None] * B
        own = self._is_own_searcher()
        if t_arrays is not None:                     # a batched BM25 search: the backend's own searcher or an injected one
            n_c = [min(int(n), pool[g]) for g, n in enumerate(t_arrays[2].tolist())]
        elif own:
            n_c = [0] * B
        else:
            n_c = [len(t_hits[g][:pool[g]]) for g in range(B)]
        live = [g for g in range(B) if n_c[g] > 0]
        if not live:
            return state, d_ids, d_sc, k_eff, dense_error, rr_hits
        try:
            by_row = False
            if own:
                state = self._get_state(model_hint, trace[0])
                by_row = self._rows_are_docs(state)
            if by_row:
                try:
                    Q = self._embed_texts([reqs[g].query for g in live], model_hint, trace[0], dim=state["dim"])
                except Exception:                        # one bad vector fails its chunk: find out whose, as run() would
                    good, vecs = [], []
                    for g in live:
                        try:
                            vecs.append(self._embed_texts([reqs[g].query], model_hint, trace[g], dim=state["dim"])[0])
                            good.append(g)
                        except Exception as e:
                            dense_error[g] = repr(e)
                            logger.error("[DenseRetrievalBackend] dense channel failed for request %d: %s", g, e)
                    live, Q = good, np.asarray(vecs, dtype=np.float32).reshape(len(good), state["dim"])
                ptr = np.zeros(len(live) + 1, dtype=np.int64)
                np.cumsum([n_c[g] for g in live], out=ptr[1:])
                flat = np.concatenate([t_arrays[0][g, :n_c[g]] for g in live]) if live else np.zeros(0, dtype=np.int64)
                _, sc = state["index"].score_rows_batch(Q, (ptr, flat))
                ids_out = np.full(t_arrays[0].shape, -1, dtype=np.int64)
                sc_out = np.full(t_arrays[0].shape, -np.inf, dtype=np.float32)
                for j, g in enumerate(live):
                    ids_out[g, :n_c[g]], sc_out[g, :n_c[g]] = flat[ptr[j]:ptr[j + 1]], sc[ptr[j]:ptr[j + 1]]
                    k_eff[g] = n_c[g]
                d_ids, d_sc = ids_out, sc_out
            else:
                if t_arrays is not None:                 # an injected BM25 searcher, or documents that are not the state's
                    dl, sl = t_arrays[0].tolist(), t_arrays[1].tolist()      # rows: the hits, scored by id and text
                    for g in range(B):
                        t_hits[g] = self.text_search._hits(list(zip(dl[g][:n_c[g]], sl[g][:n_c[g]])))
                cands = [t_hits[g][:pool[g]] for g in range(B)]
                rr = HipDenseReranker(self.router, max_pool=max(pool), embed_batch=self.embed_batch, device=self.device,
                                      corpus=self)
                scores = rr.score_batch(queries=[r.query for r in reqs], candidates=cands, trace_ids=trace)
                rr_hits = [self._scored_hits(c, s) for c, s in zip(cands, scores)]
                k_eff = [len(h) for h in rr_hits]
        except Exception as e:
            state, rr_hits = None, None
            d_ids, d_sc = np.full((B, 0), -1, dtype=np.int64), np.full((B, 0), -np.inf, dtype=np.float32)
            k_eff = [0] * B
            for g in live:
                dense_error[g] = repr(e)
            logger.error("[DenseRetrievalBackend] dense channel failed: %s", e)
        return state, d_ids, d_sc, k_eff, dense_error, rr_hits

    def retrieve_batch(self, reqs) -> List[RetrievalOut]:
        return [RetrievalOut(hits=[Hit(id=h["id"], score=h["score"], meta=h.get("meta") or {}) for h in result["hits"]],
                             diagnostics=result.get("diagnostics", {})) for result in self.run_batch(reqs)]
