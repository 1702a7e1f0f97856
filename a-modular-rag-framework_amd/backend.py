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
from collections import Counter
from dataclasses import dataclass
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


def _resolve_option(name: str, value, field: bool = False, required: bool = False):
    """An option given as a callable, as a ``"pkg.mod:func"`` string (resolved like the reference's impl strings,
    settings.yaml impl_kwargs) or, with ``field``, as a row field name (a string without a colon) -> the callable or the
    field name; ``None`` passes unless ``required``."""
    if isinstance(value, str) and (":" in value or not field):
        from .adapter import import_from_string
        value = import_from_string(value)
    if (value is None and not required) or callable(value) or (field and isinstance(value, str)):
        return value
    kinds = "a row field name, a callable" if field else "callable"
    raise TypeError(f"{name} must be {kinds} or a 'pkg.mod:func' string, got {type(value)}")


@dataclass
class _Dense:
    """The dense channel of a batch, as every dense stage of ``run_batch`` leaves it: ``ids`` / ``sc`` [B, kd], (-1, -inf) where
    a request has no row, and per request ``k_eff`` (its leading slots), ``error`` and ``filter`` (its search's ``last_filter``).
    ``collapse``: the record of the batch's one collapsed search; ``hits``: the dense hits the re-ranker made from text hits."""
    state: Optional[Dict[str, Any]]
    ids: np.ndarray
    sc: np.ndarray
    k_eff: List[int]
    error: List[Optional[str]]
    filter: List[Any]
    collapse: Optional[Dict[str, Any]] = None
    hits: Optional[List[List[Dict[str, Any]]]] = None

    @classmethod
    def empty(cls, B: int, state=None, error: Optional[str] = None) -> "_Dense":
        return cls(state, np.full((B, 0), -1, dtype=np.int64), np.full((B, 0), -np.inf, dtype=np.float32), [0] * B, [error] * B, [None] * B)


@dataclass
class _Graph:
    """The device graph channel of a batch: per request its window, ``error`` or ``info`` (the ``graph_channel`` record) and
    the leading ``n[g]`` slots of ``rows`` / ``dist`` [B, m].  ``on`` False: no such channel, every array empty."""
    on: bool
    win: List[int]
    error: List[Optional[str]]
    info: List[Any]
    n: np.ndarray
    rows: np.ndarray
    dist: np.ndarray


class DenseRetrievalBackend:
    """Corpus-wide dense retrieval behind ``run`` / ``retrieve`` (see module docstring)."""

    def __init__(self, router, sink=None, index_path: str = "data/hotpotqa/docs.jsonl", alpha_text: float = 0.4,
                 alpha_graph: float = 0.2, alpha_dense: float = 0.4, default_top_k: int = 20, dense_pool_k: int = 200,
                 embed_batch: int = 256, cache_dir: Optional[str] = None, device: int = 0, index_dtype: str = "f16",
                 text_search: Optional[Callable[..., List[Dict[str, Any]]]] = None,
                 graph_expand: Optional[Callable[..., List[Dict[str, Any]]]] = None, text_channel: Optional[str] = None,
                 bm25_k1: float = 1.5, bm25_b: float = 0.75, fuse_on_device: bool = False, bulk_ingest: bool = True,
                 bulk_batch: int = 4096, dense_row_filter: Optional[Any] = None, dense_mode: str = "search",
                 dense_filter_batch: bool = False, query_expander: Optional[Any] = None, dense_expanded: bool = False,
                 dense_collapse: Optional[Any] = None, graph_channel: Optional[str] = None, graph_window: int = 2,
                 graph_seed_k: Optional[int] = None, graph_doc: Any = "title"):
        """``text_channel="bm25"``: the reference's BM25 channel (text_index.py, retrieval_backend.py:102-128) over the same
        docs.jsonl, on the device (mrag_amd.text_index), built once per file and shared process-wide.  ``fuse_on_device``:
        a7's arithmetic in one launch (mrag_fuse_topk_batch) instead of host Python.  ``bulk_ingest``: a provider that can
        embed in bulk on the device (``embed_device``) builds the index from docs.jsonl in ``bulk_batch``-passage batches
        (text_index.py:32-53); the router path stays as the fallback / error-policy reference.
        ``dense_row_filter(req, rows) -> None | bool mask over the corpus rows | row positions``: the dense channel searches
        only those rows (``DenseIndex.search(allow=...)``); ``dense_filter_batch``: see :meth:`_search_sets`.
        ``dense_mode="rerank"``: the dense channel scores the text channel's candidates instead of searching the corpus --
        the reference's step 4 (retrieval_backend.py:332-334) with max_pool = pool.
        ``query_expander(query=, trace_id=) -> List[str]`` (the reference's LLMQueryExpander.expand): the Expand step,
        queries = [req.query] + expanded (retrieval_backend.py:307-310).  The text channel always receives the list; the
        dense channel searches all of it, max-merged per row (``DenseIndex.search_groups``), only with ``dense_expanded``.
        ``dense_collapse`` (a row field name or a callable row -> hashable): the dense channel returns the best DOCUMENTS,
        each by its best row (``DenseIndex.search_collapsed``), instead of the best rows.
        ``graph_channel="neighbors"``: the reference's graph channel (retrieval_backend.py:134-182, graph_utils.py:58-129)
        on the device (``DenseIndex.expand_neighbors``): the sentences within ``graph_window`` rows of the request's leading
        ``graph_seed_k`` dense hits (None: its top_k), inside their own document.  ``graph_doc`` names every row's document
        like ``dense_collapse``; the index holds ONE key array, so with ``dense_collapse`` both must name the same keys.
        The filter, the expander, ``dense_collapse`` and ``graph_doc`` may each be a "pkg.mod:func" string."""
        self.router, self.sink = router, sink
        self.index_path = index_path
        self.alpha_text, self.alpha_graph, self.alpha_dense = float(alpha_text), float(alpha_graph), float(alpha_dense)
        self.default_top_k, self.dense_pool_k, self.embed_batch = int(default_top_k), int(dense_pool_k), int(embed_batch)
        self.cache_dir, self.device, self.index_dtype = cache_dir, int(device), index_dtype
        self.text_search, self.graph_expand = text_search, graph_expand
        self.text_channel, self.bm25_k1, self.bm25_b = text_channel, float(bm25_k1), float(bm25_b)
        self.fuse_on_device = bool(fuse_on_device)
        self.bulk_ingest, self.bulk_batch = bool(bulk_ingest), int(bulk_batch)
        self.last_build: Dict[str, Any] = {}
        self.dense_filter_batch, self.dense_expanded = bool(dense_filter_batch), bool(dense_expanded)
        self.dense_mode, self.graph_channel, self.graph_window, self.graph_seed_k = dense_mode, graph_channel, graph_window, graph_seed_k
        self._own_text_search = None                     # the searcher _bm25_searcher() made over index_path, if any
        self._state = None
        # the four resolved options and every refusal, in one order: the first rule violated is the one reported
        rerank = dense_mode == "rerank"
        self.dense_row_filter = dense_row_filter = _resolve_option("dense_row_filter", dense_row_filter)
        if text_channel not in (None, "bm25"):
            raise ValueError(f"unknown text_channel {text_channel!r} (supported: 'bm25')")
        if dense_mode not in ("search", "rerank"):
            raise ValueError(f"unknown dense_mode {dense_mode!r} (supported: 'search', 'rerank')")
        if rerank and dense_row_filter is not None:
            raise ValueError("dense_row_filter restricts the corpus-wide search: it has no meaning with dense_mode='rerank'")
        self.query_expander = _resolve_option("query_expander", query_expander)
        if self.dense_expanded and rerank:
            raise ValueError("dense_mode='rerank' scores the candidates with req.query alone (retrieval_backend.py:333): "
                             "it does not combine with dense_expanded=True")
        self.dense_collapse = dense_collapse = _resolve_option("dense_collapse", dense_collapse, field=True)
        if dense_collapse is not None and (rerank or dense_row_filter is not None or self.dense_expanded):
            raise ValueError("dense_collapse does not combine with dense_mode='rerank', dense_row_filter or dense_expanded=True")
        if graph_channel not in (None, "neighbors"):
            raise ValueError(f"unknown graph_channel {graph_channel!r} (supported: 'neighbors')")
        if graph_channel is not None and graph_expand is not None:
            raise ValueError("graph_channel and an injected graph_expand both fill the graph channel: give one")
        if graph_channel is not None and rerank:
            raise ValueError("graph_channel seeds from the corpus-wide dense search: it does not combine with dense_mode='rerank'")
        self.graph_doc = graph_doc = _resolve_option("graph_doc", graph_doc, field=True, required=True)
        if graph_channel is not None and dense_collapse is not None and graph_doc != dense_collapse:
            raise ValueError("graph_doc and dense_collapse must name the same row keys: the index holds one key array")
        if isinstance(graph_window, bool) or not isinstance(graph_window, int) or graph_window < 0:
            raise ValueError(f"graph_window must be a non-negative integer, got {graph_window!r}")
        if graph_seed_k is not None and (isinstance(graph_seed_k, bool) or not isinstance(graph_seed_k, int) or graph_seed_k < 1):
            raise ValueError(f"graph_seed_k must be a positive integer or None, got {graph_seed_k!r}")

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

    # -- graph_channel="neighbors" ------------------------------------------------------------------------------------------
    def _graph_window_of(self, req) -> int:
        """the request's own integer ``graph_window``, else the backend's (retrieval_backend.py:318-324, :156)"""
        gw = getattr(req, "graph_window", None)
        return max(0, int(gw if isinstance(gw, int) else self.graph_window))

    def _graph_seeds_of(self, top_k: int, window: int, n_dense: int = 256) -> int:
        """how many leading dense hits seed the expansion: ``graph_seed_k`` or the request's ``top_k``, inside the call's limits
        and never more than the ``n_dense`` its dense list holds"""
        k = top_k if self.graph_seed_k is None else self.graph_seed_k
        return max(0, min(int(k), 256, 4096 // (2 * window + 1), n_dense))

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
        hids = [_fusion.raw_hit_id(r) for r in rows]
        seen = Counter(hids)
        state["row_of"] = {hid: i for i, hid in enumerate(hids) if seen[hid] == 1}
        self.last_build = {"rows": len(rows), "dim": dim, "ingest": state.get("ingest", "cache"),
                           "seconds": time.perf_counter() - t_start}
        return state

    def _file_signature(self) -> str:
        try:
            return _corpus.file_signature(self.index_path)
        except OSError:
            return f"{self.index_path}|missing"

    def _bm25_searcher(self):
        from .text_index import HipBM25Index, HipBM25TextSearcher
        key = f"bm25-index|{self._file_signature()}|{self.device}|{self.bm25_k1}|{self.bm25_b}"
        ix = _corpus.shared(key, lambda: HipBM25Index(self.index_path, k1=self.bm25_k1, b=self.bm25_b, device=self.device))
        self._own_text_search = HipBM25TextSearcher(ix)    # run_batch reads its document positions as corpus rows
        return self._own_text_search

    _FAIL_BACKOFF_S = 30.0
    _failed: Dict[str, Any] = {}        # key -> (monotonic deadline, error text): no re-embed storm after a failed build

    def _get_state(self, model_hint: str, trace_id: str):
        if self._state is None:
            import time
            key = f"dense-index|{self._file_signature()}|{model_hint}|{self.device}|{self.index_dtype}"
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

    # -- the backend protocol: leaves that run and run_batch share --------------------------------------------------------
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

    def _graph_expand_hits(self, req, pool: int, trace_id: str) -> List[Dict[str, Any]]:
        """one request's hits of an injected ``graph_expand``"""
        if self.graph_expand is None:
            return []
        with span("Backend/GraphExpand", self.sink, trace_id):
            return list(self.graph_expand(query=req.query, graph_id=getattr(req, "graph_id", "") or "", top_k=pool) or [])

    def _ensure_text_search(self) -> Optional[str]:
        """``text_channel="bm25"`` without a searcher yet: make it (:meth:`_bm25_searcher`) -> ``text_error``.  A failure
        degrades like the dense channel: it is reported and the other channels keep serving."""
        if self.text_search is None and self.text_channel == "bm25":
            try:
                self.text_search = self._bm25_searcher()
            except Exception as e:
                logger.error("[DenseRetrievalBackend] BM25 channel unavailable: %s", e)
                return repr(e)
        return None

    @staticmethod
    def _dense_hits(rows, scores, ids) -> List[Dict[str, Any]]:
        """one result row of a dense search as the dense channel's hits; the (-inf, -1) slots are left out"""
        return [{"id": _fusion.raw_hit_id(rows[int(i)]), "score": float(s), "meta": _fusion.row_meta(rows[int(i)], "dense")}
                for s, i in zip(scores, ids) if i >= 0]

    def _search_one(self, ix, Q, k: int, allow=None):
        """The search of ONE request over its query rows ``Q`` -- all of its queries max-merged per row with
        ``dense_expanded`` -- inside ``allow`` if given -> ``(scores [1, k], ids [1, k], last_filter record or None)``."""
        kw = {} if allow is None else {"allow": allow}
        sc, ids = ix.search_groups(Q, k, sizes=[len(Q)], **kw) if self.dense_expanded else ix.search(Q, k, **kw)
        return sc, ids, (ix.last_filter() if allow is not None else None)

    def _search_collapsed(self, state, Q, k: int):
        """ONE ``search_collapsed`` -- the best documents, each by its best row -> ``(scores, ids, the dense_collapse record
        of the diagnostics)``"""
        _, n_keys, m = self._row_keys(state, self.dense_collapse)
        sc, ids = state["index"].search_collapsed(Q, k, return_keys=False)
        lc = state["index"].last_collapsed()
        return sc, ids, {"keys": n_keys, "max_rows_per_key": m, "scan_k": lc["scan_k"], "redone": lc["redone_queries"]}

    @staticmethod
    def _graph_record(n_seeds: int, window: int) -> Dict[str, int]:
        return {"seeds": n_seeds, "window": window, "max_entries": n_seeds * (2 * window + 1)}

    @staticmethod
    def _fuse_overlay(fused, dense_norm, top_k: int):
        """dense-only ids carry their own meta -> the leading ``top_k`` of ``fused``"""
        for h in fused:
            if not h["meta"].get("text") and h["id"] in dense_norm:
                meta = dict(dense_norm[h["id"]]["meta"])
                meta.update({k: v for k, v in h["meta"].items() if k.startswith("score_")})
                h["meta"] = meta
        return fused[:top_k]

    def _diagnostics(self, queries, counts, top_k: int, k_eff: int, model_hint: str, dense_error, text_error, **optional):
        """One request's diagnostics.  ``counts``: the (text, graph, dense) candidates.  ``optional``: the keys that exist only
        when they say something (None: left out) -- ``batch_size``, ``dense_filter``, ``dense_collapse``, ``expand_error``,
        ``graph_window_used``, ``graph_channel``, ``graph_error``; ``dense_mode`` is added here."""
        d = {
            "queries": queries,
            "bm25_candidates": counts[0],
            "graph_candidates": counts[1],
            "dense_scored": counts[2],
            "weights": self._alphas(),
            "pool": {"dense_pool_k": self.dense_pool_k, "final_top_k": top_k, "dense_pool_k_effective": k_eff},
            "resolved_embed_model": model_hint,
            "dense_backend": "mrag_amd.DenseIndex",
            "dense_error": dense_error,
            "text_error": text_error,
        }
        if self.dense_mode == "rerank":
            d["dense_mode"] = "rerank"
        d.update({key: v for key, v in optional.items() if v is not None})
        return d

    # -- run: one request.  Its text, dense and graph steps stay its own (DESIGN.md "Backend orchestration") -------------
    def run(self, req) -> Dict[str, Any]:
        trace_id = getattr(req, "trace_id", None) or "trace-demo"                       # :304
        top_k = int(getattr(req, "top_k", None) or self.default_top_k)                  # :305
        model_hint = resolve_embed_model(self.router)
        pool = max(top_k, self.dense_pool_k)
        queries, expand_error = self._expand(req, trace_id)
        text_error = self._ensure_text_search()
        t_hits, t_docs = self._run_text(queries, pool, trace_id)
        g_hits = self._graph_expand_hits(req, pool, trace_id)
        with span("Backend/DenseRerank", self.sink, trace_id):      # same span name as :332
            state, dense_hits, dense_rows, k_eff, dense_error, dense_filter, dense_collapse = self._run_dense(
                req, queries, pool, t_hits, t_docs, model_hint, trace_id)
        graph = {}
        if self.graph_channel is not None:
            g_hits, graph = self._run_graph(req, state, dense_rows, dense_error, top_k, pool, trace_id)

        # dense hits double as candidates (their meta gives the normalised id); scores fused per :350-372
        dense_norm_hits = _fusion.dedupe_by_norm_id(dense_hits)
        dense_scores = {nid: h["score"] for nid, h in dense_norm_hits.items()}
        fuse = _fusion.fuse_channels
        if self.fuse_on_device and len(t_hits) + len(g_hits) + len(dense_scores) <= 4096:
            fuse = lambda *a, **kw: _fusion.fuse_channels_device(*a, device=self.device, **kw)    # noqa: E731
        fused = fuse(t_hits, g_hits, dense_scores, alpha_text=self.alpha_text,
                     alpha_graph=self.alpha_graph, alpha_dense=self.alpha_dense, top_k=10 ** 9)
        hits = self._fuse_overlay(fused, dense_norm_hits, top_k)
        return {"hits": hits, "diagnostics": self._diagnostics(
            queries, (len(t_hits), len(g_hits), len(dense_scores)), top_k, k_eff, model_hint, dense_error, text_error,
            dense_filter=dense_filter, dense_collapse=dense_collapse, expand_error=expand_error, **graph)}

    def _run_text(self, queries, pool: int, trace_id: str):
        """:meth:`run`'s text channel -> (hits, their document positions).  The positions are kept only in rerank mode over
        the backend's own searcher, where they are the dense state's rows."""
        if self.text_search is None:
            return [], []
        with span("Backend/TextSearch", self.sink, trace_id):
            if self.dense_mode == "rerank" and self._is_own_searcher():
                ranked = (self.text_search.index.search(queries, top_k=pool, alpha_merge="max")
                          if self.text_search.index.N > 0 else [])
                return self.text_search._hits(ranked), [int(d) for d, _ in ranked]
            return list(self.text_search(queries=queries, top_k=pool) or []), []

    def _run_dense(self, req, queries, pool: int, t_hits, t_docs, model_hint: str, trace_id: str):
        """:meth:`run`'s dense channel -> ``(state, hits, row ids or None, k_eff, error, dense_filter, dense_collapse)``.  The
        reference's policy: degrade, never raise out of run() (:229-231); what was known before a failure is reported."""
        rerank = self.dense_mode == "rerank"
        state, hits, ids, k_eff, error, dense_filter, dense_collapse = None, [], None, 0, None, None, None
        try:
            state = None if rerank else self._get_state(model_hint, trace_id)
            if rerank and t_hits:
                own = self._is_own_searcher()
                hits = self._rerank_one(req, t_hits[:pool], t_docs[:pool] if own else None, pool, model_hint, trace_id)
                k_eff = len(hits)
            if state is not None and state["index"] is not None:
                ix, rows = state["index"], state["rows"]
                if self.dense_expanded:                  # every query of the request, max-merged per row on the device
                    Q = self._embed_texts(queries, model_hint, trace_id, dim=state["dim"])
                else:
                    qv = np.asarray(_vectors(self.router.embed(model_hint=model_hint, texts=[req.query],
                                                               require={"trace_id": trace_id}))[0], dtype=np.float32)
                    if qv.shape[0] != state["dim"]:
                        raise ValueError(f"query embedding has dim {qv.shape[0]}, corpus has {state['dim']}")
                    Q = qv[None, :]
                # the reference scores its whole pool (:218,245); the index serves k up to max_k() (256): the rest is reported
                k_one = ix.max_k(1)
                k_eff = min(pool, len(rows), k_one)
                allow = self.dense_row_filter(req, rows) if self.dense_row_filter is not None else None
                if self.dense_collapse is not None:
                    k_eff = min(pool, self._row_keys(state, self.dense_collapse)[1], k_one)      # never more than there are documents
                    sc, ids, dense_collapse = self._search_collapsed(state, Q, k_eff)
                else:
                    sc, ids, dense_filter = self._search_one(ix, Q, k_eff, allow)
                ids = ids[0]
                hits = self._dense_hits(rows, sc[0], ids)
        except Exception as e:
            error = repr(e)
            logger.error("[DenseRetrievalBackend] dense channel failed: %s", e)
        return state, hits, ids, k_eff, error, dense_filter, dense_collapse

    def _run_graph(self, req, state, dense_rows, dense_error, top_k: int, pool: int, trace_id: str):
        """:meth:`run`'s device graph channel: the neighbours of the leading dense hits inside their documents (after the
        dense search, which gives the seeds; the reference's step 3, retrieval_backend.py:317-329) -> ``(graph hits, its
        keys of the diagnostics)``"""
        window = self._graph_window_of(req)
        g_hits, info, error = [], None, None
        with span("Backend/GraphExpand", self.sink, trace_id):
            try:
                if dense_error is not None:
                    raise RuntimeError(f"no seeds, the dense channel failed: {dense_error}")
                n_seeds = self._graph_seeds_of(top_k, window, len(dense_rows)) if dense_rows is not None else 0
                if n_seeds > 0:
                    g_ids, g_dist = self._graph_expand_rows(state, np.asarray(dense_rows[:n_seeds])[None, :], window, min(pool, 4096))
                    g_hits = self._graph_hits(state["rows"], g_ids[0], g_dist[0], window)
                info = self._graph_record(n_seeds, window)
            except Exception as e:
                error, g_hits = repr(e), []
                logger.error("[DenseRetrievalBackend] graph channel failed: %s", e)
        return g_hits, {"graph_window_used": window, "graph_channel": info, "graph_error": error}

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
                return self._dense_hits(state["rows"], sc, docs)
        rr = HipDenseReranker(self.router, max_pool=pool, embed_batch=self.embed_batch, device=self.device, corpus=self)
        return self._scored_hits(cands, rr.score(query=req.query, candidates=cands, trace_id=trace_id))

    # -- run_batch: the same protocol for a list of requests, as a sequence of stages -----------------------------------
    def run_batch(self, reqs) -> List[Dict[str, Any]]:
        """:meth:`run` for every request of ``reqs``, in order; the diagnostics are :meth:`run`'s plus ``batch_size``.  The
        device work of the whole list is a few calls, made by these stages (each one's docstring has its detail): every
        request is expanded (:meth:`_expand`); the text channel, one batched BM25 search, and an injected ``graph_expand``
        (:meth:`_text_batch`); the dense channel (:meth:`_dense_batch`), one search over all query embeddings or with
        ``dense_mode="rerank"`` one scoring of every request's text candidates; the device graph channel
        (:meth:`_graph_batch`); fusion in one launch over arrays (:meth:`_fuse_arrays`) where :meth:`_array_entries` can
        build them, else over hit dicts (:meth:`_fuse_hits`); one :meth:`_diagnostics` each.  ``top_k``, ``trace_id`` and
        the pool are each request's own: the searches run at the list's largest pool and a request uses the leading part
        of its lists that its own pool covers (exact searches with a declared order: a prefix is the smaller search's
        answer).  Like :meth:`run` it degrades and never raises out of the dense channel."""
        reqs = list(reqs)
        B = len(reqs)
        if not B:
            return []
        model_hint = resolve_embed_model(self.router)
        trace = [getattr(r, "trace_id", None) or "trace-demo" for r in reqs]
        top_k = [int(getattr(r, "top_k", None) or self.default_top_k) for r in reqs]
        pool = [max(k, self.dense_pool_k) for k in top_k]
        expanded = [self._expand(r, trace[g]) for g, r in enumerate(reqs)]
        queries = [e[0] for e in expanded]
        text_error = self._ensure_text_search()
        t_arrays, t_hits, g_hits = self._text_batch(reqs, queries, pool, trace)
        dense = self._dense_batch(reqs, queries, pool, trace, model_hint, t_arrays, t_hits)
        graph = self._graph_batch(reqs, dense, top_k, pool, trace)
        entries = self._array_entries(dense, graph, t_arrays, pool)
        if entries is not None:
            results = self._fuse_arrays(entries, dense.state, graph, top_k)
        else:
            results = self._fuse_hits(dense, graph, t_arrays, t_hits, g_hits, pool, top_k)
        out = []
        for g, (hits, n_text, n_dense) in enumerate(results):
            n_graph = int(graph.n[g]) if graph.on else len(g_hits[g])
            of_graph = dict(graph_window_used=graph.win[g], graph_channel=graph.info[g], graph_error=graph.error[g]) if graph.on else {}
            out.append({"hits": hits, "diagnostics": self._diagnostics(
                queries[g], (n_text, n_graph, n_dense), top_k[g], dense.k_eff[g], model_hint, dense.error[g], text_error,
                batch_size=B, dense_filter=dense.filter[g], dense_collapse=dense.collapse if dense.error[g] is None else None,
                expand_error=expanded[g][1], **of_graph)})
        return out

    def _text_batch(self, reqs, queries, pool, trace):
        """The text channel and an injected graph channel of a batch -> ``(t_arrays, t_hits, g_hits)``.  A BM25 searcher answers
        every request in ONE ``search_batch_arrays`` at the list's largest pool: ``t_arrays = (docs [B][k], scores [B][k],
        n [B])``, None when its index is empty.  Any other ``text_search``, and ``graph_expand``, are called per request."""
        from .text_index import HipBM25TextSearcher
        t_arrays = None
        t_hits: List[List[Dict[str, Any]]] = [[] for _ in reqs]
        if self.text_channel == "bm25" and isinstance(self.text_search, HipBM25TextSearcher):
            with span("Backend/TextSearch", self.sink, trace[0]):
                if self.text_search.index.N > 0:
                    t_arrays = self.text_search.index.search_batch_arrays(queries, top_k=max(pool), alpha_merge="max")
        elif self.text_search is not None:
            for g in range(len(reqs)):
                with span("Backend/TextSearch", self.sink, trace[g]):
                    t_hits[g] = list(self.text_search(queries=queries[g], top_k=pool[g]) or [])
        return t_arrays, t_hits, [self._graph_expand_hits(r, pool[g], trace[g]) for g, r in enumerate(reqs)]

    def _text_hits(self, t_arrays, pool) -> List[List[Dict[str, Any]]]:
        """the batched BM25 search's arrays as hits: per request the leading part that its own pool covers"""
        docs, scores, n = (a.tolist() for a in t_arrays)
        return [self.text_search._hits(list(zip(docs[g][:min(n[g], p)], scores[g][:min(n[g], p)]))) for g, p in enumerate(pool)]

    def _dense_batch(self, reqs, queries, pool, trace, model_hint: str, t_arrays, t_hits) -> _Dense:
        """The dense channel of a batch under its one ``Backend/DenseRerank`` span.  An exception that escapes its stage fails
        every request, is logged and never raised (the reference's policy, :229-231)."""
        dense = _Dense.empty(len(reqs))
        with span("Backend/DenseRerank", self.sink, trace[0]):
            try:
                if self.dense_mode == "rerank":
                    dense = self._rerank_batch(reqs, pool, trace, model_hint, t_arrays, t_hits)
                else:
                    dense.state = self._get_state(model_hint, trace[0])
                    if dense.state["index"] is not None:
                        self._search_batch(dense, reqs, queries, pool, trace, model_hint)
            except Exception as e:
                dense = _Dense.empty(len(reqs), dense.state, repr(e))
                logger.error("[DenseRetrievalBackend] dense channel failed: %s", e)
        return dense

    @staticmethod
    def _search_requests(dense: _Dense, who, caps, call, label: str = ""):
        """ONE index call for the requests ``who``.  ``call() -> (scores, ids, info)``: row j of the result is request
        ``who[j]``'s, which takes its leading ``k_eff = min(caps[j], the result's width)`` slots -> ``info``.  If the
        call raises, exactly those requests report the error and lose their rows, it is logged once, and None returns."""
        try:
            sc, ids, info = call()
            for j, g in enumerate(who):
                dense.k_eff[g] = k = min(caps[j], sc.shape[1])
                dense.sc[g, :k], dense.ids[g, :k] = sc[j, :k], ids[j, :k]
            return info
        except Exception as e:
            DenseRetrievalBackend._fail(dense, who, e, label)
            return None

    def _search_batch(self, dense: _Dense, reqs, queries, pool, trace, model_hint: str) -> None:
        """The corpus-wide dense search of a batch, into ``dense``.  One :meth:`_embed_texts` embeds all queries -- with
        ``dense_expanded`` every query of every request -- and the requests are searched in three classes, in this order,
        each call through :meth:`_search_requests`.  *Filtered* (``dense_row_filter`` gave a set): one :meth:`_search_one`
        each with its ``allow`` at its own pool; with ``dense_filter_batch`` and without ``dense_expanded``, all in
        :meth:`_search_sets`.  *Alone* (``dense_expanded``: its queries x the batch's k exceed the merge's 4096 entries): one
        grouped search at its own pool, where :meth:`run` would succeed or fail as well.  *Together*, the others, in ONE call
        at their largest pool, a prefix each: ``search_groups``, :meth:`_search_collapsed` (``dense.collapse`` describes
        it) or ``search``.  A request whose own search fails still reports its ``k_eff``; those of a failed shared call report 0."""
        state, ix, rows = dense.state, dense.state["index"], dense.state["rows"]
        B, n = len(reqs), len(rows)
        sizes = [len(q) for q in queries] if self.dense_expanded else [1] * B
        texts = [q for qs in queries for q in qs] if self.dense_expanded else [r.query for r in reqs]
        Q = self._embed_texts(texts, model_hint, trace[0], dim=state["dim"])
        qp = np.zeros(B + 1, dtype=np.int64)             # request g owns Q[qp[g]:qp[g + 1]]
        np.cumsum(sizes, out=qp[1:])
        k_one, k_many = ix.max_k(1), ix.max_k(B)
        dense.ids = np.full((B, max(min(max(pool), n), 0)), -1, dtype=np.int64)
        dense.sc = np.full(dense.ids.shape, -np.inf, dtype=np.float32)
        own_k = [min(p, n, k_one) for p in pool]
        in_sets = self.dense_filter_batch and not self.dense_expanded

        def alone(g, allow=None):                        # one request at its own pool
            dense.k_eff[g] = k = own_k[g]
            return self._search_requests(dense, [g], [k], lambda: self._search_one(ix, Q[qp[g]:qp[g + 1]], k, allow),
                                         f" for request {g}")
        allow = self._allow_sets(dense, reqs, rows, own_k, packed=in_sets)
        if allow and in_sets:
            self._search_sets(dense, Q, allow)
        else:
            for g, a in allow.items():
                dense.filter[g] = alone(g, a)
        plain = [g for g in range(B) if g not in allow and dense.error[g] is None]
        k_batch = min(max((pool[g] for g in plain), default=0), n, k_many)
        if self.dense_expanded:
            for g in [g for g in plain if sizes[g] * k_batch > 4096]:
                alone(g)
            plain = [g for g in plain if sizes[g] * k_batch <= 4096]

            def call():
                mine = np.concatenate([np.arange(qp[g], qp[g + 1]) for g in plain])
                return (*ix.search_groups(Q[mine], k_batch, sizes=[sizes[g] for g in plain]), None)
        elif self.dense_collapse is not None:
            def call():
                return self._search_collapsed(state, Q, min(max(pool[g] for g in plain), self._row_keys(state, self.dense_collapse)[1], k_many))
        else:
            def call():
                return (*ix.search(Q[plain] if len(plain) < B else Q, k_batch), None)
        if plain:
            dense.collapse = self._search_requests(dense, plain, [pool[g] for g in plain], call)

    @staticmethod
    def _fail(dense: _Dense, who, e: Exception, label: str = "") -> None:
        """the requests ``who`` report ``e`` and lose their rows; one log line"""
        for g in who:
            dense.error[g] = repr(e)
            dense.ids[g] = -1
        logger.error("[DenseRetrievalBackend] dense channel failed%s: %s", label, e)

    def _allow_sets(self, dense: _Dense, reqs, rows, own_k, packed: bool) -> Dict[int, Any]:
        """``dense_row_filter`` for every request of a batch -> ``{g: its allow-set}`` for those it restricts, which are then
        searched at their own ``k_eff = own_k[g]``; ``packed``: the sets as sorted row positions (``pack_sets``).  The
        callbacks do not touch the index; one that raises, or whose set cannot be packed, fails its own request only."""
        from .index import pack_sets
        allow: Dict[int, Any] = {}
        for g, r in enumerate(reqs if self.dense_row_filter is not None else []):
            try:
                got = self.dense_row_filter(r, rows)
                if got is not None:
                    dense.k_eff[g] = own_k[g]
                    allow[g] = pack_sets([got], len(rows))[1] if packed else got
            except Exception as e:
                self._fail(dense, [g], e, f" for request {g}")
        return allow

    def _search_sets(self, dense: _Dense, Q, packed: Dict[int, np.ndarray]) -> None:
        """``dense_filter_batch``: ONE ``search_sets`` for the filtered requests, at the largest of their ``k_eff``; sets of
        equal content are shared, and the diagnostics read ``dense_filter = {"path": "sets", "allowed": m}``."""
        who, set_of, set_list, index_of = list(packed), [], [], {}      # index_of: a set's content -> its position in set_list
        for g in who:
            at = index_of.setdefault(packed[g].tobytes(), len(set_list))
            if at == len(set_list):
                set_list.append(packed[g])
            set_of.append(at)
        caps = [dense.k_eff[g] for g in who]

        def call():
            return (*dense.state["index"].search_sets(Q[who], max(caps), set_list, set_of=np.asarray(set_of, dtype=np.int32)), True)
        if self._search_requests(dense, who, caps, call, " for the filtered requests"):
            for j, g in enumerate(who):
                dense.filter[g] = {"path": "sets", "allowed": int(set_list[set_of[j]].shape[0])}

    def _rerank_batch(self, reqs, pool, trace, model_hint: str, t_arrays, t_hits) -> _Dense:
        """The dense channel of a batch in rerank mode.  Own searcher: every question's leading ``min(n, pool[g])`` documents
        of the batch search are scored as corpus rows in ONE ``score_rows_batch`` after one ``_embed_texts`` of the queries
        (``ids`` = those documents, ``sc`` = their scores, for the array fusion).  Otherwise one ``HipDenseReranker.score_batch``
        over the requests' text hits (``hits``: its scores as dense hits).  The choice is :meth:`_rerank_one`'s.  Requests
        without candidates have an empty dense channel and no error; a failure is reported for the others, never raised."""
        B = len(reqs)
        dense = _Dense.empty(B)
        own = self._is_own_searcher()
        if t_arrays is not None:                     # a batched BM25 search: the backend's own searcher or an injected one
            n_c = [min(int(n), pool[g]) for g, n in enumerate(t_arrays[2].tolist())]
        elif own:
            n_c = [0] * B
        else:
            n_c = [len(t_hits[g][:pool[g]]) for g in range(B)]
        live = [g for g in range(B) if n_c[g] > 0]
        if not live:
            return dense
        try:
            by_row = False
            if own:
                dense.state = self._get_state(model_hint, trace[0])
                by_row = self._rows_are_docs(dense.state)
            if by_row:
                self._rerank_rows(dense, reqs, live, n_c, t_arrays, trace, model_hint)
            else:
                if t_arrays is not None:                 # an injected BM25 searcher, or documents that are not the state's
                    t_hits[:] = self._text_hits(t_arrays, pool)              # rows: the hits, scored by id and text
                cands = [t_hits[g][:pool[g]] for g in range(B)]
                rr = HipDenseReranker(self.router, max_pool=max(pool), embed_batch=self.embed_batch, device=self.device,
                                      corpus=self)
                scores = rr.score_batch(queries=[r.query for r in reqs], candidates=cands, trace_ids=trace)
                dense.hits = [self._scored_hits(c, s) for c, s in zip(cands, scores)]
                dense.k_eff = [len(h) for h in dense.hits]
        except Exception as e:
            error = [repr(e) if g in live and err is None else err for g, err in enumerate(dense.error)]
            dense = _Dense.empty(B)                      # what single requests reported before stays
            dense.error = error
            logger.error("[DenseRetrievalBackend] dense channel failed: %s", e)
        return dense

    def _rerank_rows(self, dense: _Dense, reqs, live, n_c, t_arrays, trace, model_hint: str) -> None:
        """the own searcher's documents ``t_arrays[0][g, :n_c[g]]`` of the requests ``live``, scored as corpus rows, into ``dense``"""
        state = dense.state
        try:
            Q = self._embed_texts([reqs[g].query for g in live], model_hint, trace[0], dim=state["dim"])
        except Exception:                                # one bad vector fails its chunk: find out whose, as run() would
            good, vecs = [], []
            for g in live:
                try:
                    vecs.append(self._embed_texts([reqs[g].query], model_hint, trace[g], dim=state["dim"])[0])
                    good.append(g)
                except Exception as e:
                    dense.error[g] = repr(e)
                    logger.error("[DenseRetrievalBackend] dense channel failed for request %d: %s", g, e)
            live, Q = good, np.asarray(vecs, dtype=np.float32).reshape(len(good), state["dim"])
        ptr = np.zeros(len(live) + 1, dtype=np.int64)
        np.cumsum([n_c[g] for g in live], out=ptr[1:])
        flat = np.concatenate([t_arrays[0][g, :n_c[g]] for g in live]) if live else np.zeros(0, dtype=np.int64)
        _, sc = state["index"].score_rows_batch(Q, (ptr, flat))
        dense.ids = np.full(t_arrays[0].shape, -1, dtype=np.int64)
        dense.sc = np.full(t_arrays[0].shape, -np.inf, dtype=np.float32)
        for j, g in enumerate(live):
            dense.ids[g, :n_c[g]], dense.sc[g, :n_c[g]] = flat[ptr[j]:ptr[j + 1]], sc[ptr[j]:ptr[j + 1]]
            dense.k_eff[g] = n_c[g]

    def _graph_batch(self, reqs, dense: _Dense, top_k, pool, trace) -> _Graph:
        """The device graph channel of a batch (``graph_channel="neighbors"``), after the dense stage that gives the seeds: ONE
        ``expand_neighbors`` call per distinct window of the batch (normally one) over every request's leading dense hits.  A
        seed row is padded with -1 beyond the request's own seeds, which changes nothing of its result, and the request takes
        its own ``m = min(pool, 4096)`` as a prefix of the call's (strict declared order).  A request whose dense channel
        failed has no seeds and reports that; a failing call is reported by the requests of its window."""
        B, on = len(reqs), self.graph_channel is not None
        rows = np.full((B, min(max(pool), 4096) if on else 0), -1, dtype=np.int64)
        graph = _Graph(on, [self._graph_window_of(r) for r in reqs] if on else [0] * B, [None] * B, [None] * B,
                       np.zeros(B, dtype=np.int64), rows, np.full(rows.shape, -1, dtype=np.int32))
        if not on:
            return graph
        win = graph.win
        with span("Backend/GraphExpand", self.sink, trace[0]):
            have = dense.state is not None and dense.state["index"] is not None and dense.ids.shape[1] > 0
            n_seeds = [0] * B
            for g in range(B):
                if dense.error[g] is not None:
                    graph.error[g] = repr(RuntimeError(f"no seeds, the dense channel failed: {dense.error[g]}"))
                elif have:
                    n_seeds[g] = self._graph_seeds_of(top_k[g], win[g], dense.k_eff[g])
            for w in sorted({win[g] for g in range(B) if n_seeds[g] > 0}):
                grp = [g for g in range(B) if n_seeds[g] > 0 and win[g] == w]
                try:
                    seeds = np.full((len(grp), max(n_seeds[g] for g in grp)), -1, dtype=np.int64)
                    for j, g in enumerate(grp):
                        seeds[j, :n_seeds[g]] = dense.ids[g, :n_seeds[g]]
                    ids, dist = self._graph_expand_rows(dense.state, seeds, w, min(max(pool[g] for g in grp), 4096))
                    for j, g in enumerate(grp):
                        c = min(pool[g], 4096)
                        graph.rows[g, :c], graph.dist[g, :c] = ids[j, :c], dist[j, :c]
                        graph.n[g] = int((ids[j, :c] >= 0).sum())
                except Exception as e:
                    for g in grp:
                        graph.error[g] = repr(e)
                        graph.rows[g], graph.dist[g], graph.n[g] = -1, -1, 0
                    logger.error("[DenseRetrievalBackend] graph channel failed: %s", e)
            graph.info = [self._graph_record(n_seeds[g], win[g]) if graph.error[g] is None else None for g in range(B)]
        return graph

    # -- fusion of a batch ------------------------------------------------------------------------------------------------
    def _norm_keys(self, state):
        """``fusion.corpus_norm_keys`` of the state's rows, built once per state and kept in it."""
        if "norm_keys" not in state:
            state["norm_keys"] = _fusion.corpus_norm_keys(state["rows"])
        return state["norm_keys"]

    def _alphas(self) -> Dict[str, float]:
        return dict(alpha_text=self.alpha_text, alpha_graph=self.alpha_graph, alpha_dense=self.alpha_dense)

    def _array_entries(self, dense: _Dense, graph: _Graph, t_arrays, pool):
        """The choice between the two fusion paths -> the entries of the array path (``fusion.batch_entries``), or None for
        the hit-dict path.  Arrays need every channel as corpus rows: the text channel is the searcher this backend made
        over ``index_path`` (only it numbers its documents as the dense state numbers its rows; an injected one, even of
        the same length, is fused by id strings), there is no injected ``graph_expand``, the dense index exists, and no
        request has more than ``FUSE_MAX_ENTRIES`` entries.  ``fuse_on_device`` plays no part in this choice."""
        state = dense.state
        if not (self._is_own_searcher() and self.graph_expand is None and state is not None and state["index"] is not None
                and (t_arrays is None or len(self.text_search.index.docs) == len(state["rows"]))):
            return None
        B = len(pool)
        if t_arrays is None:
            t_arrays = (np.full((B, 0), -1, dtype=np.int64), np.zeros((B, 0), dtype=np.float64), np.zeros(B, dtype=np.int32))
        graph_arrays = {}
        if graph.on:                                     # the reference's own fp64 decay values, looked up by distance
            from .index import reference_decay
            g_sc = np.zeros(graph.rows.shape, dtype=np.float64)
            for g in range(B):
                g_sc[g, :graph.n[g]] = reference_decay(graph.win[g])[graph.dist[g, :graph.n[g]]]
            graph_arrays = dict(graph_rows=graph.rows, graph_scores=g_sc, graph_n=graph.n)
        entries = _fusion.batch_entries(t_arrays[0], t_arrays[1], t_arrays[2], dense.ids, dense.sc, self._norm_keys(state)[0],
                                        pool=pool, **graph_arrays)
        chan_ptr = entries[0]
        sizes = chan_ptr[3::3] - chan_ptr[0:-1:3]
        return entries if int(sizes.max()) <= _fusion.FUSE_MAX_ENTRIES else None

    def _fuse_arrays(self, entries, state, graph: _Graph, top_k):
        """ONE ``mrag_fuse_topk_batch`` launch over :meth:`_array_entries` -> per request ``(hits, text candidates, dense
        candidates)``.  The meta comes from the corpus rows the payload names, overlaid as ``run`` overlays the channels."""
        chan_ptr, keys, scores, payload = entries
        rows, sorted_ids = state["rows"], self._norm_keys(state)[1]
        ok, osc, nt, ng, nd, op, n_out = _fusion.fuse_entries_device_batch(chan_ptr, keys, scores, payload, top_k=top_k,
                                                                          device=self.device, **self._alphas())
        results = []
        for g in range(len(top_k)):
            hits = []
            n_g = graph.n[g]
            dist_of = dict(zip(graph.rows[g, :n_g].tolist(), graph.dist[g, :n_g].tolist())) if n_g else {}
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
        return results

    def _fuse_hits(self, dense: _Dense, graph: _Graph, t_arrays, t_hits, g_hits, pool, top_k):
        """Fusion over hit dicts, as :meth:`run` fuses -> per request ``(hits, text candidates, dense candidates)``.  What
        the stages left as arrays becomes hits first (``t_hits`` / ``g_hits`` are filled in place); then one
        ``fuse_channels_device_batch`` with ``fuse_on_device``, else ``fuse_channels`` per request."""
        B, state = len(top_k), dense.state
        if t_arrays is not None:
            t_hits[:] = self._text_hits(t_arrays, pool)
        dense_norm, questions = [], []
        for g in range(B):
            n_g = graph.n[g]
            if n_g:
                g_hits[g] = self._graph_hits(state["rows"], graph.rows[g, :n_g], graph.dist[g, :n_g], graph.win[g])
            if dense.hits is not None:
                dense_hits = dense.hits[g]
            else:
                dense_hits = self._dense_hits(state["rows"], dense.sc[g].tolist(), dense.ids[g].tolist()) if state is not None else []
            dn = _fusion.dedupe_by_norm_id(dense_hits)
            dense_norm.append(dn)
            questions.append((t_hits[g], g_hits[g], {nid: h["score"] for nid, h in dn.items()}))
        if self.fuse_on_device:
            fused_all = _fusion.fuse_channels_device_batch(questions, top_k=10 ** 9, device=self.device, **self._alphas())
        else:
            fused_all = [_fusion.fuse_channels(*q, top_k=10 ** 9, **self._alphas()) for q in questions]
        return [(self._fuse_overlay(fused, dense_norm[g], top_k[g]), len(t_hits[g]), len(dense_norm[g]))
                for g, fused in enumerate(fused_all)]

    def retrieve(self, req) -> RetrievalOut:
        result = self.run(req)
        hits = [Hit(id=h["id"], score=h["score"], meta=h.get("meta") or {}) for h in result["hits"]]
        return RetrievalOut(hits=hits, diagnostics=result.get("diagnostics", {}))

    def retrieve_batch(self, reqs) -> List[RetrievalOut]:
        return [RetrievalOut(hits=[Hit(id=h["id"], score=h["score"], meta=h.get("meta") or {}) for h in result["hits"]],
                             diagnostics=result.get("diagnostics", {})) for result in self.run_batch(reqs)]
