"""BM25 text channel on the GPU behind the reference's own class shapes.

``HipBM25Index`` mirrors ``BM25LiteIndex`` (app/modules/retrieval/text_index.py:14-101: same constructor,
``N`` / ``avgdl`` / ``doc_lens`` / ``df`` / ``docs``, ``search(queries, top_k, alpha_merge)`` ->
``[(doc_idx, score)]``, ``doc_meta``); ``HipBM25TextSearcher`` mirrors ``BM25TextSearcher``
(retrieval_backend.py:102-128: ``search(queries=, top_k=)`` -> hits with the same ids and meta).

The index is built on the host like the reference builds it (same tokeniser, same counts) and uploaded once
as CSR postings; every search then runs on the device: scores are the reference's fp64 sums bit for bit, order is
(score desc, doc asc).  There is no CPU search path.

``search_batch`` answers many questions in one call (``mrag_bm25_search_batch``); ``search`` is that call for one
question.  Both take ``allow=``: the row filter of ``DenseIndex.search(allow=...)`` over the same docs.jsonl rows.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import re
from collections import Counter
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native as N
from .index import allow_bits

_SPLIT = re.compile(r"[^a-zA-Z0-9]+")


def tokenize(text: str) -> List[str]:
    """text_index.py:10-11."""
    return [t for t in _SPLIT.split((text or "").lower()) if t]


def build_postings(rows: Sequence[Dict[str, Any]], k1: float, b: float) -> Dict[str, Any]:
    """Host side of the index build: the reference's counts (text_index.py:36-52) as CSR postings --
    ``indptr`` [n_terms+1], ``post_doc`` (ascending inside a term), ``post_tf`` -- plus
    ``doc_norm[d] = k1 * (1 - b + b * dl_d / avgdl)``, the length term of ``_score_doc`` (:66) evaluated with
    the reference's own expression."""
    term_id: Dict[str, int] = {}
    doc_lens: List[int] = []
    t_idx: List[int] = []
    d_idx: List[int] = []
    tfs: List[int] = []
    for d, obj in enumerate(rows):
        toks = tokenize(obj.get("text", ""))
        doc_lens.append(len(toks))
        for t, c in Counter(toks).items():
            t_idx.append(term_id.setdefault(t, len(term_id)))
            d_idx.append(d)
            tfs.append(c)
    n_docs, n_terms = len(rows), len(term_id)
    avgdl = (sum(doc_lens) / n_docs) if n_docs else 0.0
    t_arr = np.asarray(t_idx, dtype=np.int64)
    order = np.argsort(t_arr, kind="stable")                     # stable: docs stay ascending inside a term
    counts = np.bincount(t_arr, minlength=n_terms) if n_terms else np.zeros(0, dtype=np.int64)
    indptr = np.zeros(n_terms + 1, dtype=np.int64)
    np.cumsum(counts, out=indptr[1:])
    inv: List[Optional[str]] = [None] * n_terms
    for t, i in term_id.items():
        inv[i] = t
    avg = avgdl or 1.0
    return {"term_id": term_id, "doc_lens": doc_lens, "N": n_docs, "avgdl": avgdl,
            "df": {inv[i]: int(counts[i]) for i in range(n_terms)},
            "indptr": indptr, "post_doc": np.ascontiguousarray(np.asarray(d_idx, dtype=np.int32)[order]),
            "post_tf": np.ascontiguousarray(np.asarray(tfs, dtype=np.int32)[order]),
            "doc_norm": np.asarray([k1 * (1 - b + b * (dl / avg)) for dl in doc_lens], dtype=np.float64)}


class HipBM25Index:
    def __init__(self, path: Optional[str] = None, k1: float = 1.5, b: float = 0.75, device: int = 0,
                 rows: Optional[Sequence[Dict[str, Any]]] = None):
        self.path = Path(path) if path is not None else None
        self.k1, self.b, self.device = k1, b, int(device)
        self.docs: List[Dict[str, Any]] = []
        self.N = 0
        self.avgdl = 0.0
        self.df: Dict[str, int] = {}
        self.doc_lens: List[int] = []
        self._term_id: Dict[str, int] = {}
        self._h = None
        self._lib = None
        if rows is not None:
            self._build(list(rows))
        elif self.path is not None and self.path.exists():       # text_index.py:32-33: a missing file is an empty index
            with self.path.open("r", encoding="utf-8") as f:
                self._build([json.loads(line) for line in (ln.strip() for ln in f) if line])

    # -- build (text_index.py:36-52) -------------------------------------------------------------------
    def _build(self, rows: List[Dict[str, Any]]):
        self.docs = rows
        p = build_postings(rows, self.k1, self.b)
        self._term_id, self.doc_lens, self.N, self.avgdl, self.df = p["term_id"], p["doc_lens"], p["N"], p["avgdl"], p["df"]
        if self.N:
            self._lib = N.load()
            h = C.c_uint64(0)
            N.check(self._lib.mrag_bm25_create(self.device, self.N, len(self._term_id), p["indptr"].ctypes.data,
                                               p["post_doc"].ctypes.data, p["post_tf"].ctypes.data, p["doc_norm"].ctypes.data,
                                               float(self.k1 + 1), C.byref(h)))
            self._h = h

    def close(self):
        if self._h is not None and self._h.value:
            self._lib.mrag_bm25_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- query side ------------------------------------------------------------------------------------
    def _idf(self, term: str) -> float:
        """text_index.py:54-56."""
        n = self.df.get(term, 0)
        return math.log((self.N - n + 0.5) / (n + 0.5) + 1.0) if self.N > 0 else 0.0

    def search(self, queries: List[str], top_k: int = 20, alpha_merge: str = "max", allow=None) -> List[Tuple[int, float]]:
        """text_index.py:71-97 on the device.  ``[(doc_idx, score)]``, best first: :meth:`search_batch` for the one
        question ``queries``.  ``allow`` (see there) restricts the candidates to some documents."""
        if not self.N or not queries or top_k <= 0:
            return []
        return self.search_batch([queries], top_k=top_k, alpha_merge=alpha_merge, allow=allow)[0]

    def _allow_words(self, allow) -> np.ndarray:
        """``allow`` -> the ABI's packed words (uint32 [ceil(N/32)], bit d%32 of word d/32).  A bool / uint8 mask over
        the documents or integer document positions go through ``index.allow_bits``, like ``DenseIndex.search(allow=)``
        on the host; an array of dtype uint32 is taken as the packed words themselves (what ``allow_bits`` returns), so
        positions must come in another integer dtype.  Bits past the last document are ignored."""
        words = (self.N + 31) // 32
        a = allow if isinstance(allow, np.ndarray) else None
        if a is not None and a.dtype == np.uint32:
            if a.ndim != 1 or a.shape[0] != words:
                raise ValueError(f"packed allow bits must be uint32 [{words}] for {self.N} documents, got shape {a.shape}")
            return np.ascontiguousarray(a)
        return np.ascontiguousarray(allow_bits(allow, self.N))

    def _plan(self, questions: List[List[str]]) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """``questions`` -> the call's ``(g_ptr, q_ptr, q_terms, q_idf)``: question g's expanded queries are
        ``g_ptr[g] .. g_ptr[g+1]``, query q's tokens ``q_ptr[q] .. q_ptr[q+1]`` of ``q_terms`` (-1 = not in the
        vocabulary) and ``q_idf``."""
        g_ptr, q_ptr, q_terms, q_idf = [0], [0], [], []
        known: Dict[str, Tuple[int, float]] = {}
        for qs in questions:
            for q in qs:
                for t in tokenize(q):
                    e = known.get(t)
                    if e is None:
                        e = known[t] = (self._term_id.get(t, -1), self._idf(t))
                    q_terms.append(e[0])
                    q_idf.append(e[1])
                q_ptr.append(len(q_terms))
            g_ptr.append(len(q_ptr) - 1)
        return (np.asarray(g_ptr, dtype=np.int32), np.asarray(q_ptr, dtype=np.int32),
                np.asarray(q_terms if q_terms else [0], dtype=np.int32), np.asarray(q_idf if q_idf else [0.0], dtype=np.float64))

    def _search_device(self, questions: List[List[str]], top_k: int, alpha_merge: str, allow):
        """``mrag_bm25_search_batch`` over a non-empty index: ``(docs int64 [B][k], scores float64 [B][k], n int32 [B])``
        with ``k = min(top_k, N)``."""
        bits = self._allow_words(allow) if allow is not None else None
        gp, qp, qt, qi = self._plan(questions)
        k, nq = int(min(top_k, self.N)), len(questions)
        docs = np.empty((nq, k), dtype=np.int64)
        scores = np.empty((nq, k), dtype=np.float64)
        n = np.zeros(nq, dtype=np.int32)
        N.check(self._lib.mrag_bm25_search_batch(self._h, nq, gp.ctypes.data, qp.ctypes.data, qt.ctypes.data, qi.ctypes.data,
                                                 1 if alpha_merge == "sum" else 0, k, bits.ctypes.data if bits is not None else None,
                                                 docs.ctypes.data, scores.ctypes.data, n.ctypes.data, None))
        return docs, scores, n

    def search_batch(self, questions: Sequence[Sequence[str]], top_k: int = 20, alpha_merge: str = "max",
                     allow=None) -> List[List[Tuple[int, float]]]:
        """Many questions in one call (``mrag_bm25_search_batch``).  ``questions[g]`` is the list of expanded query
        strings of question g; the result holds one ``[(doc_idx, score)]`` list per question, best first, and a
        question's answer does not depend on the batch it stands in.

        ``allow`` restricts every question's candidates to a set of documents: a bool / uint8 mask over the documents,
        integer document positions, or packed uint32 bits (:meth:`_allow_words`).  It changes no score -- idf and avgdl
        stay the corpus's -- and ``None`` or an all-allowed set is the plain search."""
        docs, scores, n = self.search_batch_arrays(questions, top_k=top_k, alpha_merge=alpha_merge, allow=allow)
        dl, sl = docs.tolist(), scores.tolist()
        return [list(zip(dl[g][:c], sl[g][:c])) for g, c in enumerate(n.tolist())]

    def search_batch_arrays(self, questions: Sequence[Sequence[str]], top_k: int = 20, alpha_merge: str = "max",
                            allow=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """:meth:`search_batch` as the call's own arrays: ``(docs int64 [B][k], scores float64 [B][k], n int32 [B])`` with
        ``k = min(top_k, N)`` (0 for an empty index or ``top_k <= 0``); question g's answer is its first ``n[g]`` slots,
        the others hold (-1, 0.0).  What the batched fusion reads without building a tuple per hit."""
        questions = [list(qs) for qs in questions]
        nq = len(questions)
        if not self.N or not questions or top_k <= 0:
            return np.full((nq, 0), -1, dtype=np.int64), np.zeros((nq, 0), dtype=np.float64), np.zeros(nq, dtype=np.int32)
        return self._search_device(questions, top_k, alpha_merge, allow)

    def set_scratch_limit(self, nbytes: int) -> None:
        """Bytes of fp64 score rows (8 * N per expanded query) one chunk of :meth:`search_batch` may use
        (``mrag_bm25_set_scratch_limit``); ``<= 0`` restores the default.  Results do not depend on it."""
        if self._h is not None:
            N.check(self._lib.mrag_bm25_set_scratch_limit(self._h, int(nbytes)))

    def doc_meta(self, doc_idx: int) -> Dict[str, Any]:
        return dict(self.docs[doc_idx]) if 0 <= doc_idx < len(self.docs) else {}


class HipBM25TextSearcher:
    """``BM25TextSearcher`` (retrieval_backend.py:102-128) over a :class:`HipBM25Index`; usable as the
    ``text_search`` channel of :class:`mrag_amd.backend.DenseRetrievalBackend`."""

    def __init__(self, index: HipBM25Index):
        self.index = index

    def _hits(self, ranked: List[Tuple[int, float]]) -> List[Dict[str, Any]]:
        out = []
        for doc_idx, s in ranked:
            meta = self.index.doc_meta(doc_idx)
            out.append({"id": "sent::%s::%s" % (meta.get("doc_id") or meta.get("title") or "doc", str(meta.get("sent_id") or "")),
                        "score": float(s),
                        "meta": {"kind": "sentence", "text": meta.get("text"), "doc": meta.get("title"),
                                 "sent_id": meta.get("sent_id"), "source": "bm25"}})
        return out

    def search(self, *, queries: List[str], top_k: int) -> List[Dict[str, Any]]:
        if self.index.N <= 0:
            return []
        return self._hits(self.index.search(queries, top_k=top_k, alpha_merge="max"))

    def search_batch(self, *, queries: Sequence[Sequence[str]], top_k: int, allow=None) -> List[List[Dict[str, Any]]]:
        """:meth:`search` for one list of expanded queries per question (``HipBM25Index.search_batch``); per question
        the hit list :meth:`search` returns.  ``allow``: the document filter of ``HipBM25Index.search_batch``."""
        if self.index.N <= 0:
            return [[] for _ in queries]
        return [self._hits(r) for r in self.index.search_batch(queries, top_k=top_k, alpha_merge="max", allow=allow)]

    __call__ = search
