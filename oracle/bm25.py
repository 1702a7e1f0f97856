"""CPU oracle of the BM25 text channel.  TEST INFRASTRUCTURE (oracle/__init__.py): only tests/,
__graft_entry__.smoke() and bench.py's cpu_baseline leg may import it.

Restates ``BM25LiteIndex`` (app/modules/retrieval/text_index.py) and the hit shaping of
``BM25TextSearcher.search`` (app/modules/retrieval/retrieval_backend.py:106-128) in plain Python, fp64,
same operation order.  PINNED by fixture F7 (tests/golden/f7_bm25.json, captured from the reference's
own classes by tests/golden/make_golden_bm25.py).

Declared tie-break where the reference's order is the iteration order of a ``set`` of ints
(text_index.py:79,88,95): equal scores are ordered by ascending document index.
"""
from __future__ import annotations

import math
import re
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np


def tokenize(text: str) -> List[str]:
    """text_index.py:10-11."""
    return [t for t in re.split(r"[^a-zA-Z0-9]+", (text or "").lower()) if t]


class Bm25Oracle:
    def __init__(self, rows: Sequence[Dict[str, Any]], k1: float = 1.5, b: float = 0.75):
        """text_index.py:36-52 over already-parsed docs.jsonl rows."""
        self.k1, self.b = k1, b
        self.docs = list(rows)
        self.tf: Dict[str, Dict[int, int]] = {}
        self.doc_lens: List[int] = []
        for i, obj in enumerate(self.docs):
            toks = tokenize(obj.get("text", ""))
            self.doc_lens.append(len(toks))
            for t in toks:
                bucket = self.tf.setdefault(t, {})
                bucket[i] = bucket.get(i, 0) + 1
        self.N = len(self.docs)
        self.avgdl = (sum(self.doc_lens) / self.N) if self.N else 0.0
        self.df = {t: len(p) for t, p in self.tf.items()}

    def idf(self, term: str) -> float:
        """text_index.py:54-56."""
        n = self.df.get(term, 0)
        return math.log((self.N - n + 0.5) / (n + 0.5) + 1.0) if self.N > 0 else 0.0

    def score_doc(self, q_terms: Sequence[str], d: int) -> float:
        """text_index.py:59-69: every token of the query (repeats included) adds its term, left to right."""
        score = 0.0
        dl = self.doc_lens[d] if d < len(self.doc_lens) else 0
        for t in q_terms:
            f = self.tf.get(t, {}).get(d, 0)
            if f == 0:
                continue
            denom = f + self.k1 * (1 - self.b + self.b * (dl / (self.avgdl or 1.0)))
            score += self.idf(t) * (f * (self.k1 + 1)) / (denom or 1.0)
        return score

    def search(self, queries: Sequence[str], top_k: int = 20, alpha_merge: str = "max") -> List[Tuple[int, float]]:
        """text_index.py:71-97; ties ordered by ascending doc (declared, see module docstring)."""
        if not self.N:
            return []
        q_terms_list = [tokenize(q) for q in queries]
        cands = set()
        for q_terms in q_terms_list:
            for t in set(q_terms):
                cands.update(self.tf.get(t, {}).keys())
        scores: Dict[int, float] = {}
        for d in cands:
            s_list = [self.score_doc(q_terms, d) for q_terms in q_terms_list]
            s = sum(s_list) if alpha_merge == "sum" else (max(s_list) if s_list else 0.0)
            if s > 0:
                scores[d] = s
        return sorted(scores.items(), key=lambda kv: (-kv[1], kv[0]))[:top_k]

    def hits(self, queries: Sequence[str], top_k: int) -> List[Dict[str, Any]]:
        """BM25TextSearcher.search, retrieval_backend.py:106-128."""
        out = []
        for d, s in self.search(queries, top_k=top_k, alpha_merge="max"):
            meta = dict(self.docs[d])
            out.append({"id": "sent::%s::%s" % (meta.get("doc_id") or meta.get("title") or "doc", str(meta.get("sent_id") or "")),
                        "score": float(s),
                        "meta": {"kind": "sentence", "text": meta.get("text"), "doc": meta.get("title"),
                                 "sent_id": meta.get("sent_id"), "source": "bm25"}})
        return out


# ---------------------------------------------------------------------------------------------------------
# The same search from CSR postings, vectorised: what makes corpora of several hundred thousand rows testable.
# ---------------------------------------------------------------------------------------------------------
SELECT_GRID = 1024 * 256        # documents one sweep of the device's 1024 x 256 selection grid covers

POSTINGS_MUTANTS = ("ties_doc_desc", "first_stride_only", "score_top5_bytes", "drop_repeats", "tokens_reversed",
                    "sum_is_max", "skip_255", "cut_before_filter")


def query_term_ids(postings: Dict[str, Any], queries: Sequence[str]) -> List[Tuple[List[int], List[float]]]:
    """Every query as (term ids, idfs), token by token in order, repeats included; an unknown term has id -1.
    ``postings`` is what ``build_postings`` returns; the idf is text_index.py:54-56 with its own expression."""
    n_docs, out = postings["N"], []
    for q in queries:
        ids, idfs = [], []
        for t in tokenize(q):
            n = postings["df"].get(t, 0)
            ids.append(postings["term_id"].get(t, -1))
            idfs.append(math.log((n_docs - n + 0.5) / (n + 0.5) + 1.0) if n_docs > 0 else 0.0)
        out.append((ids, idfs))
    return out


def merged_scores(postings: Dict[str, Any], queries, merge: str = "max", k1: float = 1.5,
                  mutant: Optional[str] = None) -> np.ndarray:
    """fp64 score of every document after the merge over the queries, before ``s > 0`` is asked.  Elementwise IEEE
    operations in the order of ``Bm25Oracle.score_doc`` and ``search``: a document receives its tokens' terms left to
    right, then the queries' scores are merged left to right."""
    indptr, post_doc, post_tf = postings["indptr"], postings["post_doc"], postings["post_tf"]
    doc_norm = np.asarray(postings["doc_norm"], dtype=np.float64)
    if queries and isinstance(queries[0], str):
        queries = query_term_ids(postings, queries)
    if mutant == "sum_is_max" and merge == "sum":
        merge = "max"
    fin = None
    for ids, idfs in queries:
        toks = list(zip(ids, idfs))
        if mutant == "drop_repeats":
            toks = list(dict(toks).items())                         # every term once, at its first position
        if mutant == "tokens_reversed":
            toks = toks[::-1]
        row = np.zeros(len(doc_norm), dtype=np.float64)
        for t, idf in toks:
            if t < 0:
                continue
            lo, hi = int(indptr[t]), int(indptr[t + 1])
            docs, tf = post_doc[lo:hi], post_tf[lo:hi].astype(np.float64)
            if mutant == "skip_255":
                keep = np.arange(hi - lo) % 256 != 255
                docs, tf = docs[keep], tf[keep]
            row[docs] = row[docs] + (float(idf) * (tf * (k1 + 1))) / (tf + doc_norm[docs])
        fin = row if fin is None else (fin + row if merge == "sum" else np.maximum(fin, row))
    return fin if fin is not None else np.zeros(len(doc_norm), dtype=np.float64)


def select_topk(fin: np.ndarray, k: int, mutant: Optional[str] = None) -> List[Tuple[int, float]]:
    """Keep ``s > 0``, order by (score descending, document ascending), cut at ``k``."""
    docs = np.arange(len(fin), dtype=np.int64)
    if mutant == "cut_before_filter":
        # the cut is made over the raw keys of every touched document (a negative double's bit pattern is above
        # every positive one's), s <= 0 is dropped afterwards
        bits = fin.view(np.uint64)
        cand = docs[bits != 0]
        cand = cand[np.lexsort((cand, ~bits[cand]))][:k]                              # negative scores first
        cand = cand[fin[cand] > 0]
        return [(int(d), float(fin[d])) for d in cand[np.lexsort((cand, -fin[cand]))]]
    cand = docs[fin > 0]
    if mutant == "first_stride_only":
        cand = cand[cand < SELECT_GRID]
    key = fin[cand]
    if mutant == "score_top5_bytes":
        key = (key.view(np.uint64) >> np.uint64(24)).astype(np.float64)                # 40 bits: exact in fp64
    tie = -cand if mutant == "ties_doc_desc" else cand
    order = np.lexsort((tie, -key))[:k]
    return [(int(d), float(s)) for d, s in zip(cand[order], fin[cand[order]])]


def search_postings(postings: Dict[str, Any], queries, k: int, merge: str = "max", k1: float = 1.5,
                    mutant: Optional[str] = None) -> List[Tuple[int, float]]:
    """``Bm25Oracle.search`` from the CSR arrays of ``build_postings`` (``indptr``, ``post_doc``, ``post_tf``,
    ``doc_norm``), bit for bit.  ``queries``: strings (``postings`` then carries ``term_id`` / ``df`` / ``N``), or
    one ``(term ids, idfs)`` pair per query for hand-made postings.  ``mutant`` makes one deliberate error
    (``POSTINGS_MUTANTS``); only the sensitivity test passes it."""
    assert mutant is None or mutant in POSTINGS_MUTANTS, mutant
    return select_topk(merged_scores(postings, queries, merge, k1, mutant), k, mutant)
