"""The orchestration of ``DenseRetrievalBackend`` on the host: ``run_batch(reqs)[g]`` is ``run(reqs[g])`` for the plain,
filtered, sets, grouped, collapsed, graph and rerank branches, over a numpy stand-in of ``DenseIndex`` (test infrastructure
only -- the product has no CPU path; the same branches run on the real index in the tests/test_gpu_*.py of each feature).
The stand-in answers with the restatements the other tests already have and logs every call, the provider logs its batch
sizes and a sink logs the spans: the index calls, embedding calls and spans of every configuration are written out below
as literals.  They were recorded from the backend as it stood before its ``run_batch`` was split into stages, so they pin
what a restructuring of ``backend.py`` must leave alone.  An injected ``text_search`` keeps the fusion on the host.
"""
import zlib
from typing import Optional

import numpy as np
import pytest

import filter_sets_cases as fs
import neighbors_cases as nc
import search_collapsed_cases as sc
import search_groups_cases as sg
import mrag_amd.index as index_mod
from mrag_amd import corpus, fusion
from mrag_amd.backend import DenseRetrievalBackend, HipDenseReranker
from mrag_amd.dto import RetrievalIn
from oracle import dense_search as ods
from oracle import ref_semantics as rs
from test_rerank_batch_host import Prov, Router


# ------------------------------------------------------------------------------------------------ the stand-in
class StageIndex:
    """numpy stand-in for mrag_amd.index.DenseIndex: fp16 storage, every search answered by its restatement.  The log and
    the failure switch are the class's: the backends of one test share one index (``corpus.shared``)."""
    log = []
    searches, fail_at = 0, None                       # the ``fail_at``-th search since arming raises

    def __init__(self, dim, metric="cosine", dtype="f16", device=0):
        self.dim = dim
        self._rows = np.zeros((0, dim), dtype=np.float16)
        self._keys, self._filter, self._collapsed = None, None, None

    def __len__(self):
        return self._rows.shape[0]

    def add(self, rows, normalize=None):
        self._rows = np.concatenate([self._rows, ods.normalize_round(np.asarray(rows, dtype=np.float32))])

    def close(self):
        pass

    def max_k(self, nq=1):
        return 256

    def _called(self, method, nq, k, **kw):
        """one log line: the method, its query rows, its k and the keyword arguments given (names, and what they held)"""
        StageIndex.log.append(f"{method} nq={nq} k={k}" + "".join(f" {name}={v}" for name, v in kw.items()))
        if method.startswith("search"):
            StageIndex.searches += 1
            if StageIndex.searches == StageIndex.fail_at:
                raise RuntimeError("injected index failure")

    def _q(self, q):
        return ods.normalize_round(np.asarray(q, dtype=np.float32).reshape(-1, self.dim))

    def _allowed(self, allow):
        return index_mod.pack_sets([allow], len(self))[1]

    def search(self, q, k, allow=None):
        q16 = self._q(q)
        if allow is None:
            self._called("search", len(q16), k)
            v, i = ods.brute_force_topk(q16, self._rows, k)
        else:
            rows = self._allowed(allow)
            self._called("search", len(q16), k, allow=len(rows))
            v, i = fs.oracle(q16, self._rows, [rows], np.zeros(len(q16), dtype=np.int32), k)
            self._filter = {"path": "mask", "allowed": int(len(rows))}
        return v.astype(np.float32), i

    def last_filter(self):
        self._called("last_filter", 0, 0)
        return dict(self._filter)

    def search_sets(self, q, k, sets, set_of=None):
        q16 = self._q(q)
        self._called("search_sets", len(q16), k, sets=[len(s) for s in sets], set_of=np.asarray(set_of).tolist())
        v, i = fs.oracle(q16, self._rows, [np.asarray(s, dtype=np.int64) for s in sets], np.asarray(set_of), k)
        return v.astype(np.float32), i

    def search_groups(self, q, k, group_ptr=None, sizes=None, allow=None):
        q16, sizes = self._q(q), [int(s) for s in sizes]
        rows = np.arange(len(self)) if allow is None else self._allowed(allow)
        self._called("search_groups", len(q16), k, sizes=sizes, **({} if allow is None else {"allow": len(rows)}))
        if max(sizes) * k > sg.MAX_ENTRIES:
            raise ValueError(f"{max(sizes)} queries x k = {k} exceed {sg.MAX_ENTRIES} entries")
        v, i = sg.oracle_groups(q16, self._rows[rows], sizes, k)
        if allow is not None:
            self._filter = {"path": "mask", "allowed": int(len(rows))}
        return v.astype(np.float32), np.where(i >= 0, rows[np.maximum(i, 0)], -1)

    def set_row_keys(self, keys):
        self._called("set_row_keys", len(keys), 0)
        self._keys = np.asarray(keys, dtype=np.int32)

    def search_collapsed(self, q, k, scan_k=None, return_keys=True):
        q16 = self._q(q)
        self._called("search_collapsed", len(q16), k, **({} if scan_k is None else {"scan_k": scan_k}), return_keys=return_keys)
        v, i, kk = sc.oracle_collapsed(q16, self._rows, self._keys, k)
        m = int(np.bincount(self._keys).max())
        self._collapsed = {"scan_k": index_mod.collapse_scan_k(k, m, len(self)), "redone_queries": 0, "redo_rounds": 0,
                           "max_rows_per_key": m, "distinct_keys": len(set(self._keys.tolist()))}
        return (v.astype(np.float32), i, kk) if return_keys else (v.astype(np.float32), i)

    def last_collapsed(self):
        self._called("last_collapsed", 0, 0)
        return dict(self._collapsed)

    def expand_neighbors(self, seeds, window, m=None, decay=None, return_from=False):
        seeds = np.asarray(seeds, dtype=np.int64)
        self._called("expand_neighbors", seeds.shape[0], seeds.shape[1], window=window, m=m, return_from=return_from)
        out = nc.expand(seeds, self._keys, window, m=m)
        return out if return_from else out[:2]

    def score_rows(self, q, ids):
        ids = np.asarray(ids, dtype=np.int64)
        self._called("score_rows", 1, len(ids))
        return (self._rows[ids].astype(np.float64) @ self._q(q)[0].astype(np.float64)).astype(np.float32)

    def score_rows_batch(self, queries, row_ids, normalize=None):
        q16 = self._q(queries)
        self._called("score_rows_batch", len(q16), sum(len(r) for r in row_ids))
        return [(self._rows[np.asarray(r, dtype=np.int64)].astype(np.float64) @ q.astype(np.float64)).astype(np.float32)
                for q, r in zip(q16, row_ids)]


@pytest.fixture()
def stage_index(monkeypatch):
    def reset():
        StageIndex.log, StageIndex.searches, StageIndex.fail_at = [], 0, None
        DenseRetrievalBackend._failed.clear()
        corpus.drop_shared("dense-index|")
    monkeypatch.setattr(index_mod, "DenseIndex", StageIndex)
    monkeypatch.setattr(HipDenseReranker, "_cosines", lambda self, qv, vecs: [rs.cosine(list(qv), list(v)) for v in vecs])
    reset()
    yield StageIndex
    reset()


class Sink:
    def __init__(self):
        self.events = []

    def record(self, evt):
        self.events.append((evt["event"], evt["node"], evt["trace_id"]))

    def spans(self):
        """(node, trace id) of every span in order; no span of the backend opens inside another"""
        assert [e[0] for e in self.events] == ["node_start", "node_end"] * (len(self.events) // 2)
        assert self.events[0::2] == [("node_start",) + e[1:] for e in self.events[1::2]]
        return [e[1:] for e in self.events[0::2]]


# ------------------------------------------------------------------------------------------------ corpus and requests
def doc_rows(n):
    """``n`` sentence rows over titles in runs of 1 .. 7 rows (``neighbors_cases.runs_1_to_7``)"""
    rng = np.random.default_rng(11)
    rows, at = [], {}
    for t in nc.runs_1_to_7(n).tolist():
        s = at[t] = at.get(t, -1) + 1
        rows.append({"doc_id": f"Title {t}#{s}", "title": f"Title {t}", "sent_id": s,
                     "text": " ".join(rng.choice(fs.WORDS, size=int(rng.integers(4, 10))))})
    return rows


N_SMALL, N_LARGE = 60, 200        # 15 titles; 53 titles: enough rows for 25 queries x the pool to pass 4096 entries
ROWS = {n: doc_rows(n) for n in (N_SMALL, N_LARGE)}


@pytest.fixture()
def docs(tmp_path):
    paths = {}
    for n, rows in ROWS.items():
        paths[n] = str(tmp_path / f"docs{n}.jsonl")
        corpus.write_docs_jsonl(paths[n], rows)
    return paths


class Req(RetrievalIn):
    graph_window: Optional[int] = None


# the queries' lengths % 4 give three_sets_or_none's four kinds: 0 3 1 2 1 0 2
QUERIES = ["king", "war", "alpha", "king album", "band film", "film war", "river city war"]
TOP_K = (1, 5, 30, 3, 8, 2, 12)                      # 30 is above dense_pool_k = 20
WINDOWS = (None, 0, None, None, 5, None, None)
TRACES = [f"t{g}" for g in range(7)]


def requests(top_k=TOP_K):
    return [Req(query=q, graph_id="", top_k=k, trace_id=t, graph_window=w) for q, k, t, w in zip(QUERIES, top_k, TRACES, WINDOWS)]


def text_search_over(rows):
    """an injected text channel with fixed hits: eleven rows from a start the first query names, scores falling"""
    def text_search(*, queries, top_k):
        at = zlib.crc32(queries[0].encode("utf-8")) % len(rows)
        pick = [(at + 5 * j) % len(rows) for j in range(11)]
        return [{"id": fusion.raw_hit_id(rows[i]), "score": 9.0 - 0.5 * j + 0.25 * len(queries), "meta": fusion.row_meta(rows[i], "bm25")}
                for j, i in enumerate(pick)][:top_k]
    return text_search


def three_sets_or_none(req, rows):
    """``filter_sets_cases.three_sets_or_none`` for a corpus of any size: by the query's length, no filter, the even rows (a
    mask), the first 20 rows (positions, unsorted and with a duplicate) or the rows of every fourth title (a mask)"""
    n, kind = len(rows), len(req.query) % 4
    if kind == 0:
        return None
    if kind == 1:
        return np.arange(n) % 2 == 0
    if kind == 2:
        return np.concatenate([np.arange(19, -1, -1), [5]])
    return np.asarray([int(r["title"].split()[1]) % 4 == 0 for r in rows])


def long_for_one(*, query, trace_id):
    """``long_expander`` (25 queries) for one request, the short ``expander`` (4 queries) for the others"""
    return (sg.long_expander if query == QUERIES[4] else sg.expander)(query=query, trace_id=trace_id)


def backend(path, rows, prov=None, sink=None, **kw):
    kw.setdefault("dense_pool_k", 20)
    return DenseRetrievalBackend(Router(prov or Prov()), sink=sink, index_path=path, text_search=text_search_over(rows), **kw)


def same(batch, single, B, but_k_eff=False):
    assert batch["hits"] == single["hits"]
    diag, want = dict(batch["diagnostics"]), dict(single["diagnostics"])
    assert diag.pop("batch_size") == B
    if but_k_eff:
        diag["pool"], want["pool"] = dict(diag["pool"], dense_pool_k_effective=None), dict(want["pool"], dense_pool_k_effective=None)
    assert diag == want


def k_eff(outs):
    return [o["diagnostics"]["pool"]["dense_pool_k_effective"] for o in outs]


# ------------------------------------------------------------------------------------------------ the configurations
# name -> (corpus rows, top_k of the requests, backend options)
CONFIGS = {
    "default": (N_SMALL, TOP_K, {}),
    "filter": (N_SMALL, TOP_K, dict(dense_row_filter=three_sets_or_none)),
    "filter-sets": (N_SMALL, TOP_K, dict(dense_row_filter=three_sets_or_none, dense_filter_batch=True)),
    "expanded": (N_SMALL, TOP_K, dict(query_expander=sg.expander, dense_expanded=True)),
    "expanded-filter": (N_SMALL, TOP_K, dict(query_expander=sg.expander, dense_expanded=True, dense_row_filter=three_sets_or_none)),
    # 200 rows, pools of 100 and one of 170: the batch's grouped search runs at k = 170, where the request with 25 queries
    # has 4250 entries and is searched alone at its own pool (2500 entries)
    "expanded-long": (N_LARGE, (1, 5, 170, 3, 8, 2, 12), dict(query_expander=long_for_one, dense_expanded=True, dense_pool_k=100)),
    "expanded-long-filter": (N_LARGE, (1, 5, 170, 3, 8, 2, 12), dict(query_expander=long_for_one, dense_expanded=True, dense_pool_k=100,
                                                                     dense_row_filter=three_sets_or_none)),
    "collapse": (N_SMALL, TOP_K, dict(dense_collapse="title")),
    "graph": (N_SMALL, TOP_K, dict(graph_channel="neighbors")),
    "graph-collapse": (N_SMALL, TOP_K, dict(graph_channel="neighbors", dense_collapse="title")),
    "rerank": (N_SMALL, TOP_K, dict(dense_mode="rerank")),
}


def observe(docs, name):
    """the loop of ``run``, then ``run_batch`` on the same backend -> (want, got, what both did)"""
    n, top_k, kw = CONFIGS[name]
    prov, sink = Prov(), Sink()
    be = backend(docs[n], ROWS[n], prov=prov, sink=sink, **kw)
    reqs = requests(top_k)
    be.run(reqs[0])                                  # builds the index: its embed calls are not the requests'
    seen = {}
    for which, call in (("run", lambda: [be.run(r) for r in reqs]), ("batch", lambda: be.run_batch(reqs))):
        StageIndex.log, sink.events, n0 = [], [], len(prov.calls)
        seen[which] = call()
        seen[which + "_index"], seen[which + "_embeds"], seen[which + "_spans"] = list(StageIndex.log), prov.calls[n0:], sink.spans()
    return seen


def per_request(*nodes):
    return [(node, t) for t in TRACES for node in nodes]


def each(node):
    return [(node, t) for t in TRACES]


LF, LC = "last_filter nq=0 k=0", "last_collapsed nq=0 k=0"
BATCH_SPANS = each("Backend/TextSearch") + [("Backend/DenseRerank", "t0")]
RUN_SPANS = per_request("Backend/TextSearch", "Backend/DenseRerank")
EXPANDED_SPANS = dict(batch_spans=each("Backend/Expand") + BATCH_SPANS,
                      run_spans=per_request("Backend/Expand", "Backend/TextSearch", "Backend/DenseRerank"))
GRAPH_SPANS = dict(batch_spans=BATCH_SPANS + [("Backend/GraphExpand", "t0")],             # after the dense span
                   run_spans=per_request("Backend/TextSearch", "Backend/DenseRerank", "Backend/GraphExpand"))
PLAIN_RUN = ["search nq=1 k=20", "search nq=1 k=20", "search nq=1 k=30", "search nq=1 k=20", "search nq=1 k=20", "search nq=1 k=20",
             "search nq=1 k=20"]
# requests 0 and 5 are not filtered: run_batch searches them together, after the filtered ones
FILTERED = ["search nq=1 k=20 allow=15", LF, "search nq=1 k=30 allow=30", LF, "search nq=1 k=20 allow=20", LF, "search nq=1 k=20 allow=30", LF]
FILTERED_RUN = ["search nq=1 k=20"] + FILTERED + ["search nq=1 k=20", "search nq=1 k=20 allow=20", LF]
G4, G4_30 = "search_groups nq=4 k=20 sizes=[4]", "search_groups nq=4 k=30 sizes=[4]"
GROUPS_FILTERED = [G4 + " allow=15", LF, G4_30 + " allow=30", LF, G4 + " allow=20", LF, G4 + " allow=30", LF]
L4, L4_170, L25 = "search_groups nq=4 k=100 sizes=[4]", "search_groups nq=4 k=170 sizes=[4]", "search_groups nq=25 k=100 sizes=[25]"
LONG_FILTERED = [L4 + " allow=52", LF, L4_170 + " allow=100", LF, L4 + " allow=20", LF, L25 + " allow=100", LF]
COLLAPSED = ["search_collapsed nq=1 k=17 return_keys=False", LC]
NEIGHBORS = ["expand_neighbors nq=1 k=1 window=2 m=20 return_from=True", "expand_neighbors nq=1 k=5 window=0 m=20 return_from=True",
             "expand_neighbors nq=1 k=30 window=2 m=30 return_from=True", "expand_neighbors nq=1 k=3 window=2 m=20 return_from=True",
             "expand_neighbors nq=1 k=8 window=5 m=20 return_from=True", "expand_neighbors nq=1 k=2 window=2 m=20 return_from=True",
             "expand_neighbors nq=1 k=12 window=2 m=20 return_from=True"]
# one expansion per distinct window of the batch, in ascending order; under dense_collapse a request has 17 dense hits at most
NEIGHBORS_BATCH = ["expand_neighbors nq=1 k=5 window=0 m=20 return_from=True", "expand_neighbors nq=5 k=30 window=2 m=30 return_from=True",
                   "expand_neighbors nq=1 k=8 window=5 m=20 return_from=True"]
# What the backend did in every configuration before run_batch was split into stages: the index calls (query rows, k and
# what the keyword arguments held; for expand_neighbors nq x k is the seed array), the provider's batch sizes, the spans.
EXPECT = {
    "default": dict(batch_index=["search nq=7 k=30"], batch_embeds=[7], batch_spans=BATCH_SPANS,
                    run_index=PLAIN_RUN, run_embeds=[1] * 7, run_spans=RUN_SPANS),
    "filter": dict(batch_index=FILTERED + ["search nq=1 k=20 allow=20", LF, "search nq=2 k=20"], batch_embeds=[7], batch_spans=BATCH_SPANS,
                   run_index=FILTERED_RUN, run_embeds=[1] * 7, run_spans=RUN_SPANS),
    "filter-sets": dict(batch_index=["search_sets nq=5 k=30 sets=[15, 30, 20] set_of=[0, 1, 2, 1, 2]", "search nq=2 k=20"], batch_embeds=[7],
                        batch_spans=BATCH_SPANS, run_index=FILTERED_RUN, run_embeds=[1] * 7, run_spans=RUN_SPANS),
    "expanded": dict(batch_index=["search_groups nq=28 k=30 sizes=[4, 4, 4, 4, 4, 4, 4]"], batch_embeds=[28],
                     run_index=[G4, G4, G4_30, G4, G4, G4, G4], run_embeds=[4] * 7, **EXPANDED_SPANS),
    "expanded-filter": dict(batch_index=GROUPS_FILTERED + [G4 + " allow=20", LF, "search_groups nq=8 k=20 sizes=[4, 4]"], batch_embeds=[28],
                            run_index=[G4] + GROUPS_FILTERED + [G4, G4 + " allow=20", LF], run_embeds=[4] * 7, **EXPANDED_SPANS),
    "expanded-long": dict(batch_index=[L25, "search_groups nq=24 k=170 sizes=[4, 4, 4, 4, 4, 4]"], batch_embeds=[49],
                          run_index=[L4, L4, L4_170, L4, L25, L4, L4], run_embeds=[4, 4, 4, 4, 25, 4, 4], **EXPANDED_SPANS),
    "expanded-long-filter": dict(batch_index=LONG_FILTERED + [L4 + " allow=20", LF, "search_groups nq=8 k=100 sizes=[4, 4]"], batch_embeds=[49],
                                 run_index=[L4] + LONG_FILTERED + [L4, L4 + " allow=20", LF], run_embeds=[4, 4, 4, 4, 25, 4, 4],
                                 **EXPANDED_SPANS),
    "collapse": dict(batch_index=["search_collapsed nq=7 k=17 return_keys=False", LC], batch_embeds=[7], batch_spans=BATCH_SPANS,
                     run_index=COLLAPSED * 7, run_embeds=[1] * 7, run_spans=RUN_SPANS),
    "graph": dict(batch_index=["search nq=7 k=30"] + NEIGHBORS_BATCH, batch_embeds=[7],
                  run_index=[x for pair in zip(PLAIN_RUN, NEIGHBORS) for x in pair], run_embeds=[1] * 7, **GRAPH_SPANS),
    "graph-collapse": dict(batch_index=["search_collapsed nq=7 k=17 return_keys=False", LC] + [x.replace("k=30", "k=17") for x in NEIGHBORS_BATCH],
                           batch_embeds=[7], run_index=[x for nb in NEIGHBORS for x in COLLAPSED + [nb.replace("k=30", "k=17")]],
                           run_embeds=[1] * 7, **GRAPH_SPANS),
    "rerank": dict(batch_index=["score_rows_batch nq=7 k=77"], batch_embeds=[7], batch_spans=BATCH_SPANS,
                   run_index=["score_rows nq=1 k=11"] * 7, run_embeds=[1] * 7, run_spans=RUN_SPANS),
}
K_EFF = {name: [170 if k == 170 else 100 for k in top_k] if n == N_LARGE else [max(k, 20) for k in top_k]
         for name, (n, top_k, _) in CONFIGS.items()}
K_EFF.update({"collapse": [17] * 7, "graph-collapse": [17] * 7, "rerank": [11] * 7})     # 17 titles; the text channel's 11 candidates


@pytest.mark.parametrize("name", list(CONFIGS))
def test_run_batch_is_run_and_makes_the_written_out_calls(stage_index, docs, name):
    seen = observe(docs, name)
    for g in range(7):
        got, want = seen["batch"][g], seen["run"][g]
        assert want["diagnostics"]["dense_error"] is None and want["hits"]
        if name == "filter-sets" and "dense_filter" in want["diagnostics"]:
            # the one documented difference: the shared call names its path "sets", the single search its own
            assert got["diagnostics"]["dense_filter"] == {"path": "sets", "allowed": want["diagnostics"]["dense_filter"]["allowed"]}
            got = dict(got, diagnostics=dict(got["diagnostics"], dense_filter=want["diagnostics"]["dense_filter"]))
        same(got, want, 7)
    for key, want in EXPECT[name].items():
        assert seen[key] == want, (name, key)
    assert k_eff(seen["run"]) == k_eff(seen["batch"]) == K_EFF[name]


# ------------------------------------------------------------------------------------------------ failures
def arm(fail_at):
    StageIndex.searches, StageIndex.fail_at = 0, fail_at


@pytest.mark.parametrize("name,failing", [("filter", [2]), ("filter-sets", [1, 2, 3, 4, 6]), ("expanded-filter", [2]),
                                          ("expanded-long", [0, 1, 2, 3, 5, 6])])
def test_a_failing_index_call_fails_the_requests_it_served_in_both_drivers(stage_index, docs, name, failing):
    """The second search of a ``run_batch`` raises.  The requests it served report the error, every other request is
    served; ``run`` reports the same for a request whose own search raises.  ``k_eff`` was set before the search of a
    filtered request and is reported nevertheless; the requests of a shared plain or grouped search have it from the
    result and report 0 (for those the test arms the FIRST search: "filter-sets" has them all in its first call)."""
    n, top_k, kw = CONFIGS[name]
    be = backend(docs[n], ROWS[n], **kw)
    reqs = requests(top_k)
    be.run(reqs[0])
    arm(1 if name == "filter-sets" else 2)
    got = be.run_batch(reqs)
    arm(None)
    assert [g for g in range(7) if got[g]["diagnostics"]["dense_error"] is not None] == failing
    want = []
    for g, r in enumerate(reqs):
        arm(1 if g in failing else None)
        want.append(be.run(r))
        arm(None)
    shared = name == "expanded-long"                  # the failing call is the grouped search the six requests share
    for g in range(7):
        same(got[g], want[g], 7, but_k_eff=shared and g in failing)
        assert (got[g]["diagnostics"]["dense_error"] == "RuntimeError('injected index failure')") == (g in failing)
        assert "dense_filter" not in got[g]["diagnostics"] or g not in failing
    assert k_eff(want) == K_EFF[name]
    assert k_eff(got) == ([0 if g in failing else k for g, k in enumerate(K_EFF[name])] if shared else K_EFF[name])


def test_a_failing_plain_search_fails_every_request(stage_index, docs):
    """the one search of the default ``run_batch`` raises: every request reports it and is served by the text channel alone.
    ``run`` has set ``k_eff`` before its search, ``run_batch`` takes it from the result: 20 / 30 there, 0 here"""
    be = backend(docs[N_SMALL], ROWS[N_SMALL])
    reqs = requests()
    be.run(reqs[0])
    arm(1)
    got = be.run_batch(reqs)
    want = []
    for r in reqs:
        arm(1)
        want.append(be.run(r))
    arm(None)
    for g in range(7):
        same(got[g], want[g], 7, but_k_eff=True)
        assert got[g]["diagnostics"]["dense_error"] == "RuntimeError('injected index failure')" and got[g]["hits"]
        assert got[g]["diagnostics"]["dense_scored"] == 0
    assert k_eff(got) == [0] * 7 and k_eff(want) == K_EFF["default"]


@pytest.mark.parametrize("name", ["filter", "filter-sets", "expanded-filter"])
def test_a_filter_callback_that_raises_fails_its_own_request_only(stage_index, docs, name):
    """``run`` has set ``k_eff`` when it calls the filter, ``run_batch`` has not: 20 there, 0 here, everything else alike"""
    n, top_k, kw = CONFIGS[name]

    def flaky(req, rows):
        if req.query == QUERIES[3]:
            raise KeyError("no tenant")
        return three_sets_or_none(req, rows)
    be = backend(docs[n], ROWS[n], **dict(kw, dense_row_filter=flaky))
    reqs = requests(top_k)
    want = [be.run(r) for r in reqs]
    got = be.run_batch(reqs)
    for g in range(7):
        if name == "filter-sets" and "dense_filter" in want[g]["diagnostics"]:
            want[g]["diagnostics"]["dense_filter"]["path"] = "sets"
        same(got[g], want[g], 7, but_k_eff=g == 3)
        assert (got[g]["diagnostics"]["dense_error"] == "KeyError('no tenant')") == (g == 3)
    assert got[3]["hits"] and got[3]["diagnostics"]["dense_scored"] == 0
    assert k_eff(want) == K_EFF[name] and k_eff(got) == [20, 20, 30, 0, 20, 20, 20]


@pytest.mark.parametrize("dense_expanded", [False, True])
def test_a_failing_expander_is_reported_and_the_request_runs_on_its_own_query(stage_index, docs, dense_expanded):
    sink = Sink()
    be = backend(docs[N_SMALL], ROWS[N_SMALL], sink=sink, query_expander=sg.failing_expander, dense_expanded=dense_expanded)
    reqs = requests()
    want = [be.run(r) for r in reqs]
    sink.events = []
    got = be.run_batch(reqs)
    assert sink.spans() == EXPANDED_SPANS["batch_spans"]
    for g in range(7):
        same(got[g], want[g], 7)
        d = got[g]["diagnostics"]
        assert d["expand_error"] == "RuntimeError('the expander is down')" and d["queries"] == [QUERIES[g]] and d["dense_error"] is None
    assert k_eff(got) == K_EFF["default"]
    plain = backend(docs[N_SMALL], ROWS[N_SMALL])
    assert [o["hits"] for o in got] == [o["hits"] for o in plain.run_batch(reqs)]


@pytest.mark.parametrize("name", ["default", "filter", "expanded", "collapse", "graph", "rerank"])
def test_a_missing_corpus_file_is_an_empty_dense_channel(stage_index, docs, name):
    n, top_k, kw = CONFIGS[name]
    be = backend(docs[n] + ".missing", ROWS[n], **kw)
    reqs = requests(top_k)
    want = [be.run(r) for r in reqs]
    got = be.run_batch(reqs)
    for g in range(7):
        same(got[g], want[g], 7)
        d = got[g]["diagnostics"]
        assert d["dense_error"] is None and got[g]["hits"] and "dense_filter" not in d and "dense_collapse" not in d
        assert d["graph_candidates"] == 0 and ("graph_channel" in d) == (name == "graph")
    assert [x for x in StageIndex.log if not x.startswith("score_rows")] == []
    assert k_eff(got) == ([11] * 7 if name == "rerank" else [0] * 7)      # rerank embeds the candidates it cannot look up


# ------------------------------------------------------------------------------------------------ the constructor
def _f(req, rows):
    return None


REFUSALS = [
    (dict(dense_row_filter=5), TypeError, "dense_row_filter must be callable or a 'pkg.mod:func' string, got <class 'int'>"),
    (dict(text_channel="tfidf"), ValueError, "unknown text_channel 'tfidf' (supported: 'bm25')"),
    (dict(dense_mode="bogus"), ValueError, "unknown dense_mode 'bogus' (supported: 'search', 'rerank')"),
    (dict(dense_mode="rerank", dense_row_filter=_f), ValueError,
     "dense_row_filter restricts the corpus-wide search: it has no meaning with dense_mode='rerank'"),
    (dict(query_expander=5), TypeError, "query_expander must be callable or a 'pkg.mod:func' string, got <class 'int'>"),
    (dict(dense_mode="rerank", dense_expanded=True), ValueError,
     "dense_mode='rerank' scores the candidates with req.query alone (retrieval_backend.py:333): it does not combine with dense_expanded=True"),
    (dict(dense_collapse=5), TypeError, "dense_collapse must be a row field name, a callable or a 'pkg.mod:func' string, got <class 'int'>"),
    (dict(dense_collapse="title", dense_mode="rerank"), ValueError,
     "dense_collapse does not combine with dense_mode='rerank', dense_row_filter or dense_expanded=True"),
    (dict(dense_collapse="title", dense_row_filter=_f), ValueError,
     "dense_collapse does not combine with dense_mode='rerank', dense_row_filter or dense_expanded=True"),
    (dict(dense_collapse=sc.title_of, dense_expanded=True), ValueError,
     "dense_collapse does not combine with dense_mode='rerank', dense_row_filter or dense_expanded=True"),
    (dict(graph_channel="bfs"), ValueError, "unknown graph_channel 'bfs' (supported: 'neighbors')"),
    (dict(graph_channel="neighbors", graph_expand=lambda **kw: []), ValueError,
     "graph_channel and an injected graph_expand both fill the graph channel: give one"),
    (dict(graph_channel="neighbors", dense_mode="rerank"), ValueError,
     "graph_channel seeds from the corpus-wide dense search: it does not combine with dense_mode='rerank'"),
    (dict(graph_doc=5), TypeError, "graph_doc must be a row field name, a callable or a 'pkg.mod:func' string, got <class 'int'>"),
    (dict(graph_doc=None), TypeError, "graph_doc must be a row field name, a callable or a 'pkg.mod:func' string, got <class 'NoneType'>"),
    (dict(graph_channel="neighbors", dense_collapse="title", graph_doc="doc_id"), ValueError,
     "graph_doc and dense_collapse must name the same row keys: the index holds one key array"),
    (dict(graph_window=-1), ValueError, "graph_window must be a non-negative integer, got -1"),
    (dict(graph_window=True), ValueError, "graph_window must be a non-negative integer, got True"),
    (dict(graph_window=2.0), ValueError, "graph_window must be a non-negative integer, got 2.0"),
    (dict(graph_seed_k=0), ValueError, "graph_seed_k must be a positive integer or None, got 0"),
    (dict(graph_seed_k=True), ValueError, "graph_seed_k must be a positive integer or None, got True"),
    # two rules violated at once: the first of the order above is the one reported
    (dict(dense_row_filter=5, text_channel="tfidf"), TypeError, "dense_row_filter must be callable or a 'pkg.mod:func' string, got <class 'int'>"),
    (dict(dense_mode="bogus", query_expander=5), ValueError, "unknown dense_mode 'bogus' (supported: 'search', 'rerank')"),
    (dict(dense_mode="rerank", dense_row_filter=_f, dense_expanded=True), ValueError,
     "dense_row_filter restricts the corpus-wide search: it has no meaning with dense_mode='rerank'"),
    (dict(dense_collapse="title", dense_expanded=True, graph_doc=5), ValueError,
     "dense_collapse does not combine with dense_mode='rerank', dense_row_filter or dense_expanded=True"),
    (dict(graph_channel="neighbors", dense_mode="rerank", graph_window=-1), ValueError,
     "graph_channel seeds from the corpus-wide dense search: it does not combine with dense_mode='rerank'"),
    (dict(graph_window=-1, graph_seed_k=0), ValueError, "graph_window must be a non-negative integer, got -1"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_the_constructor_refuses_with_the_type_and_the_message_it_always_had(case):
    """the literals are copied from the constructor as it stood before its option handling was gathered"""
    kw, exc, message = REFUSALS[case]
    with pytest.raises(exc) as e:
        DenseRetrievalBackend(object(), index_path="nowhere.jsonl", **kw)
    assert type(e.value) is exc and str(e.value) == message


def test_the_constructor_resolves_import_strings_and_keeps_field_names():
    b = DenseRetrievalBackend(object(), dense_row_filter="filter_sets_cases:three_sets_or_none", query_expander="search_groups_cases:expander")
    assert b.dense_row_filter is fs.three_sets_or_none and b.query_expander is sg.expander
    assert b.dense_collapse is None and b.graph_doc == "title"
    b = DenseRetrievalBackend(object(), dense_collapse="search_collapsed_cases:title_of", graph_doc="search_collapsed_cases:title_of",
                              graph_channel="neighbors")
    assert b.dense_collapse is sc.title_of and b.graph_doc is sc.title_of
    b = DenseRetrievalBackend(object(), dense_collapse="title", graph_doc=nc.title_of)
    assert b.dense_collapse == "title" and b.graph_doc is nc.title_of      # without graph_channel the two need not agree
