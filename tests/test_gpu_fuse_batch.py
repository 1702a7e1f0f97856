"""Batched hybrid retrieval on the GPU: ``mrag_fuse_topk_batch`` against the single call ``mrag_fuse_topk`` (bit for bit,
question by question), against ``fusion.fuse_channels`` (pinned to golden F3 elsewhere) and against the array restatement
of tests/fuse_batch_cases.py (payloads); ``DenseRetrievalBackend.run_batch`` against ``run``.  Everything is exact: no
tolerances.  The cases' own conditions are established on the CPU in tests/test_fuse_batch_host.py.
"""
import ctypes as C
import json
import zlib

import numpy as np
import pytest

import fuse_batch_cases as fc

pytestmark = pytest.mark.gpu
UNTOUCHED = 7777


def _args(alphas):
    return dict(alpha_text=alphas[0], alpha_graph=alphas[1], alpha_dense=alphas[2])


def raw_call(ptr, keys, scores, payload, top_k, stride, alphas=fc.ALPHAS, n_questions=None):
    """the C call itself, on output buffers pre-filled with UNTOUCHED -> (status, dict of arrays)"""
    from mrag_amd import _native as N
    B = len(top_k) if n_questions is None else n_questions
    ptr, keys = np.ascontiguousarray(ptr, dtype=np.int32), np.ascontiguousarray(keys, dtype=np.int32)
    scores, tk = np.ascontiguousarray(scores, dtype=np.float64), np.ascontiguousarray(top_k, dtype=np.int32)
    payload = None if payload is None else np.ascontiguousarray(payload, dtype=np.int32)
    width = max(stride, 0)
    o = {"key": np.full((len(top_k), width), UNTOUCHED, dtype=np.int32), "n": np.full(len(top_k), UNTOUCHED, dtype=np.int32),
         "pay": np.full((len(top_k), width, 3), UNTOUCHED, dtype=np.int32)}
    for name in ("fused", "nt", "ng", "nd"):
        o[name] = np.full((len(top_k), width), float(UNTOUCHED))
    st = N.load().mrag_fuse_topk_batch(0, B, ptr.ctypes.data, keys.ctypes.data, scores.ctypes.data,
                                       payload.ctypes.data if payload is not None else None, alphas[0], alphas[1], alphas[2],
                                       tk.ctypes.data, stride, o["key"].ctypes.data, o["fused"].ctypes.data, o["nt"].ctypes.data,
                                       o["ng"].ctypes.data, o["nd"].ctypes.data, o["pay"].ctypes.data if payload is not None else None,
                                       o["n"].ctypes.data, None)
    return st, o


def run_batch_arrays(questions, alphas=fc.ALPHAS, stride=None):
    ptr, keys, scores, payload, tk = fc.pack(questions)
    tk = np.minimum(tk, ptr[3::3] - ptr[0:-1:3])
    stride = int(tk.max()) if stride is None else stride
    st, o = raw_call(ptr, keys, scores, payload, tk, stride, alphas)
    assert st == 0
    return o


def single(q, alphas=fc.ALPHAS):
    """``mrag_fuse_topk`` on the question alone -> (keys, [fused, nt, ng, nd] as uint64 bit patterns)"""
    from mrag_amd import _native as N
    kk = min(q["top_k"], len(q["keys"]))
    ok = np.empty(max(kk, 1), dtype=np.int32)
    vals = [np.empty(max(kk, 1), dtype=np.float64) for _ in range(4)]
    n = C.c_int(0)
    keys, scores = np.asarray(q["keys"] or [0], dtype=np.int32), np.asarray(q["scores"] or [0.0], dtype=np.float64)
    N.check(N.load().mrag_fuse_topk(0, keys.ctypes.data, scores.ctypes.data, q["n"][0], q["n"][1], q["n"][2], alphas[0], alphas[1],
                                    alphas[2], kk, ok.ctypes.data, *[v.ctypes.data for v in vals], C.byref(n), None))
    return ok[:n.value].tolist(), [v[:n.value].view(np.uint64).tolist() for v in vals]


def check_row(o, g, q, alphas=fc.ALPHAS, against_single=True):
    """row g of a batch result is question q's answer: the restatement's (values, payloads), the single call's bits, and
    (-1, 0.0) behind it"""
    ref = fc.reference(q, alphas)
    n = int(o["n"][g])
    assert n == len(ref)
    assert o["key"][g, :n].tolist() == [r[0] for r in ref]
    for j, name in enumerate(("fused", "nt", "ng", "nd")):
        assert o[name][g, :n].tolist() == [r[1 + j] for r in ref], name
    assert [tuple(p) for p in o["pay"][g, :n].tolist()] == [r[5] for r in ref]
    if against_single:
        sk, sv = single(q, alphas)
        assert o["key"][g, :n].tolist() == sk
        for name, bits in zip(("fused", "nt", "ng", "nd"), sv):
            assert o[name][g, :n].view(np.uint64).tolist() == bits, name
    assert (o["key"][g, n:] == -1).all() and (o["pay"][g, n:] == -1).all()
    for name in ("fused", "nt", "ng", "nd"):
        assert (o[name][g, n:].view(np.uint64) == 0).all()


# ------------------------------------------------------------------------------------------------ golden F3
def test_golden_f3_as_one_batch(golden_dir):
    from mrag_amd import fusion
    cases = json.loads((golden_dir / "f3_hybrid_run.json").read_text())["cases"]
    groups = {}                                                    # one batch per set of alphas (they are arguments of the call)
    for c in cases:
        kw = c["backend_kwargs"]
        groups.setdefault((kw["alpha_text"], kw["alpha_graph"], kw["alpha_dense"]), []).append(c)
    for alphas_of, group in groups.items():
        qs = [(c["t_hits_raw"], c["g_hits_raw"], c["dense_scores_raw"]) for c in group]
        own = [int(c["req"]["top_k"] or c["backend_kwargs"]["default_top_k"]) for c in group]
        for tks in (own, 1, 10 ** 9):
            got = fusion.fuse_channels_device_batch(qs, top_k=tks, **_args(alphas_of))
            for g, c in enumerate(group):
                tk = tks[g] if isinstance(tks, list) else tks
                assert got[g] == fusion.fuse_channels(*qs[g], top_k=tk, **_args(alphas_of)), c["name"]
        got = fusion.fuse_channels_device_batch(qs, top_k=[len(c["run_out"]["hits"]) for c in group], **_args(alphas_of))
        for g, c in enumerate(group):
            assert [h["score"] for h in got[g]] == [h["score"] for h in c["run_out"]["hits"]], c["name"]


# ------------------------------------------------------------------------------------------------ sizes
def test_every_size_alone_and_all_sizes_in_one_shuffled_batch():
    qs = fc.size_questions()
    for q in qs:
        check_row(run_batch_arrays([q]), 0, q)
    order = np.random.default_rng(11).permutation(len(qs)).tolist()
    at = order.index(fc.SIZES.index(4096))                        # the 4096-entry question between an empty and a one-entry one
    rest = [i for i in order if fc.SIZES[i] not in (0, 1, 4096)]
    order = rest[:at] + [fc.SIZES.index(0), fc.SIZES.index(4096), fc.SIZES.index(1)] + rest[at:]
    o = run_batch_arrays([qs[i] for i in order])
    for g, i in enumerate(order):
        check_row(o, g, qs[i], against_single=False)              # the single call's bits: compared above, question by question


def test_a_question_above_the_limit_refuses_the_whole_batch():
    from mrag_amd import _native as N
    from mrag_amd import fusion
    qs = [fc.filler(0), fc.question(text=[(i % 3000, (i % 17) / 16.0) for i in range(4097)]), fc.filler(1)]
    ptr, keys, scores, payload, tk = fc.pack(qs)
    st, o = raw_call(ptr, keys, scores, payload, [4, 4, 4], 4)
    assert st == -5 and "question 1" in N.load().mrag_last_error().decode()
    assert (o["n"] == 0).all() and (o["key"] == UNTOUCHED).all() and (o["fused"] == UNTOUCHED).all() and (o["pay"] == UNTOUCHED).all()
    # the hit-dict form fuses such a question on the host instead
    big = fc.as_channels(qs[1])
    got = fusion.fuse_channels_device_batch([fc.as_channels(qs[0]), big, fc.as_channels(qs[2])], top_k=7, **_args(fc.ALPHAS))
    assert got == [fusion.fuse_channels(*fc.as_channels(q), top_k=7, **_args(fc.ALPHAS)) for q in qs]


# ------------------------------------------------------------------------------------------------ position
def test_a_question_row_does_not_depend_on_its_place_or_neighbours():
    qs = fc.position_questions()
    alone = [run_batch_arrays([q], stride=64) for q in qs]
    for j, q in enumerate(qs):
        check_row(alone[j], 0, q)
    for size in (2, 257):
        for place in (0, size // 2, size - 1):
            for j, q in enumerate(qs):
                batch = [fc.filler(g) for g in range(size)]
                batch[place] = q
                o = run_batch_arrays(batch, stride=64)
                for name in ("key", "pay", "n"):
                    assert np.array_equal(o[name][place], alone[j][name][0]), (size, place, j, name)
                for name in ("fused", "nt", "ng", "nd"):
                    assert np.array_equal(o[name][place].view(np.uint64), alone[j][name][0].view(np.uint64)), (size, place, j, name)


# ------------------------------------------------------------------------------------------------ channels, dedupe, ties
def test_channels_dedupe_and_signed_zeros():
    named = {**fc.channel_questions(), **fc.dedupe_questions()}
    for alphas in (fc.ALPHAS, fc.ZERO_ALPHAS):
        o = run_batch_arrays(list(named.values()), alphas)
        for g, (name, q) in enumerate(named.items()):
            check_row(o, g, q, alphas)
    # the payloads the cases were built for, spelled out
    o = run_batch_arrays(list(named.values()))
    row = {name: g for g, name in enumerate(named)}

    def kept(name, key, chan):
        g = row[name]
        return int(o["pay"][g, o["key"][g].tolist().index(key), chan])
    assert kept("five equal", 4, 0) == 1 and kept("later larger", 4, 2) == 3
    assert kept("zeros as duplicates, -0 first", 4, 0) == 0 and kept("zeros as duplicates, +0 first", 4, 0) == 0
    g = row["zeros as min, +0 first"]                             # key 2 holds -0.0, lo is the +0.0 met first: -0.0 - 0.0 = -0.0
    assert np.signbit(o["nd"][g, o["key"][g].tolist().index(2)])


def test_ties_cuts_and_the_tail_of_a_wide_stride():
    cuts, distinct = fc.cut_questions()
    qs = [fc.tie_question(3), fc.tie_question(10 ** 9)] + cuts
    o = run_batch_arrays(qs, stride=distinct + 9)                  # larger than every top_k
    assert o["key"][0, :4].tolist() == [1, 2, 4, -1] and o["n"][:2].tolist() == [3, 6]
    assert o["n"][2:].tolist() == [0, 1, distinct, distinct]
    for g, q in enumerate(qs):
        check_row(o, g, q)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_happen_before_any_output_is_written():
    from mrag_amd import _native as N
    qs = [fc.filler(0), fc.filler(1), fc.filler(2)]
    ptr, keys, scores, payload, _ = fc.pack(qs)

    def refused(st, o, code, *words):
        msg = N.load().mrag_last_error().decode()
        assert st == code and all(w in msg for w in words), msg
        assert (o["n"] == 0).all() and (o["key"] == UNTOUCHED).all() and (o["nd"] == UNTOUCHED).all()
    bad = scores.copy()
    bad[int(ptr[3]) + 1] = np.nan
    refused(*raw_call(ptr, keys, bad, payload, [2, 2, 2], 4), -1, "NaN", "entry 1", "question 1")
    down = ptr.copy()
    down[7] = down[6] - 1
    refused(*raw_call(down, keys, scores, payload, [2, 2, 2], 4), -1, "question 2")
    refused(*raw_call(ptr, keys, scores, payload, [2, 5, 2], 4), -1, "question 1")
    refused(*raw_call(ptr, keys, scores, payload, [2, 2, -1], 4), -1, "question 2")
    st, o = raw_call(ptr, keys, scores, payload, [2, 2, 2], -1)
    assert st == -1
    # nothing to do is not an error: no question, and only empty questions
    assert raw_call(np.zeros(1, dtype=np.int32), [0], [0.0], None, [], 4, n_questions=0)[0] == 0
    st, o = raw_call(np.zeros(7, dtype=np.int32), [0], [0.0], [0], [3, 0], 3)
    assert st == 0 and o["n"].tolist() == [0, 0] and (o["key"] == -1).all() and (o["fused"] == 0.0).all() and (o["pay"] == -1).all()


# ------------------------------------------------------------------------------------------------ run_batch against run
WORDS = ["alpha", "beta", "gamma", "delta", "river", "city", "born", "film", "band", "album", "war", "king"]
EMPTY_ROW = 123


def _pm1_vec(text, dim=64):
    """exactly 16 entries of +-1: every norm is 4, every stored value +-0.25, every cosine a multiple of 1/16 that fp32
    sums exactly in any order -- the batch kernel and the one-query kernel must agree bit for bit, with many exact ties"""
    rng = np.random.default_rng(zlib.crc32(("" if text.startswith("blank") else text).encode("utf-8")))
    v = np.zeros(dim, dtype=np.float32)
    v[rng.choice(dim, size=16, replace=False)] = rng.choice([-1.0, 1.0], size=16)
    return v.tolist()


def _gauss_vec(text, dim=64):
    return [float(x) for x in np.random.default_rng(zlib.crc32(text.encode("utf-8"))).standard_normal(dim)]


class _Router:
    def __init__(self, vec):
        self.vec = vec

    def embed(self, *, model_hint, texts, require=None):
        return {"vectors": [self.vec(t) for t in texts]}


class _BrokenRouter:
    def embed(self, *, model_hint, texts, require=None):
        raise RuntimeError("provider down")


def _rows():
    rng = np.random.default_rng(3)
    rows = [{"doc_id": f"Title {i // 4}#{i % 4}", "title": f"Title {i // 4}", "sent_id": i % 4,
             "text": " ".join(rng.choice(WORDS, size=int(rng.integers(4, 12))))} for i in range(800)]
    rows[EMPTY_ROW]["text"] = ""                                                # a row without text: its meta comes from the dense row
    rows[41]["title"], rows[41]["sent_id"] = rows[40]["title"], rows[40]["sent_id"]      # two rows, one normalised id
    return rows


def _reqs():
    from mrag_amd.dto import RetrievalIn
    rng = np.random.default_rng(17)
    queries = ["blank river king"] + [" ".join(rng.choice(WORDS, size=int(rng.integers(2, 5)))) for _ in range(32)]
    return [RetrievalIn(query=q, graph_id="", top_k=(1, 15, 300)[g % 3], trace_id=f"t{g}") for g, q in enumerate(queries)]


@pytest.fixture(scope="module")
def docs(tmp_path_factory):
    from mrag_amd import corpus
    path = tmp_path_factory.mktemp("fuse_batch") / "docs.jsonl"
    corpus.write_docs_jsonl(path, _rows())
    corpus.drop_shared("dense-index|"); corpus.drop_shared("bm25-index|")
    yield str(path)
    corpus.drop_shared("dense-index|"); corpus.drop_shared("bm25-index|")


def _ghosts(*, query, graph_id, top_k):
    h = zlib.crc32(query.encode("utf-8"))
    return [{"id": f"sent::Ghost {(h + j) % 7}::{j % 2}", "score": float((h >> j) % 5), "meta": {"doc": f"Ghost {(h + j) % 7}", "sent_id": j % 2}}
            for j in range(6)]


def _even_rows_for_some(req, rows):
    return np.arange(len(rows)) % 2 == 0 if len(req.query) % 2 else None


@pytest.mark.parametrize("fuse_on_device", [True, False])
@pytest.mark.parametrize("config", ["plain", "graph", "filter"])
def test_run_batch_is_run_for_every_request(docs, config, fuse_on_device):
    from mrag_amd.backend import DenseRetrievalBackend
    extra = {"graph": {"graph_expand": _ghosts}, "filter": {"dense_row_filter": _even_rows_for_some}}.get(config, {})
    be = DenseRetrievalBackend(_Router(_pm1_vec), index_path=docs, text_channel="bm25", dense_pool_k=100, fuse_on_device=fuse_on_device, **extra)
    reqs = _reqs()
    got = be.run_batch(reqs)
    assert len(got) == len(reqs) == 33
    filtered = 0
    for g, r in enumerate(reqs):
        want = be.run(r)
        assert want["diagnostics"]["dense_error"] is None and want["diagnostics"]["text_error"] is None
        assert got[g]["hits"] == want["hits"], (g, r.query)
        assert len(got[g]["hits"]) == r.top_k or r.top_k == 300
        diag = dict(got[g]["diagnostics"])
        assert diag.pop("batch_size") == 33 and diag == want["diagnostics"]
        filtered += "dense_filter" in diag
    assert (filtered > 0) == (config == "filter") and filtered < 33
    out = be.retrieve_batch(reqs[:2])
    assert [(h.id, h.score, h.meta) for h in out[1].hits] == [(h["id"], h["score"], h["meta"]) for h in got[1]["hits"]]


def test_the_empty_text_row_takes_its_meta_from_the_dense_row(docs):
    from mrag_amd import fusion
    from mrag_amd.backend import DenseRetrievalBackend
    from mrag_amd.dto import RetrievalIn
    be = DenseRetrievalBackend(_Router(_pm1_vec), index_path=docs, text_channel="bm25", dense_pool_k=100)
    req = RetrievalIn(query="blank river king", graph_id="", top_k=300, trace_id="t")
    got = be.run_batch([req])[0]["hits"]
    nid = fusion.normalize_id({"id": "", "meta": fusion.row_meta(_rows()[EMPTY_ROW], "dense")})[0]
    hit = [h for h in got if h["id"] == nid]
    assert len(hit) == 1 and hit[0]["meta"]["source"] == "dense" and hit[0]["meta"]["text"] == "" and hit[0]["meta"]["score_dense_norm"] == 1.0
    shared = fusion.normalize_id({"id": "", "meta": fusion.row_meta(_rows()[40], "dense")})[0]
    assert sum(h["id"] == shared for h in got) <= 1 and got == be.run(req)["hits"]


def test_run_batch_with_gaussian_embeddings_fuses_its_own_searches(tmp_path):
    """batch and one-query dense scores may differ in the last bit here, so ``run`` is no yardstick: the hits must be the
    host fusion of row g of the batch's own dense search and question g of the BM25 batch search"""
    from mrag_amd import fusion
    from mrag_amd.backend import DenseRetrievalBackend, resolve_embed_model
    from mrag_amd import corpus
    path = tmp_path / "docs.jsonl"                                              # a file of its own: indexes are shared per file
    corpus.write_docs_jsonl(path, _rows())
    router = _Router(_gauss_vec)
    be = DenseRetrievalBackend(router, index_path=str(path), text_channel="bm25", dense_pool_k=100)
    reqs = _reqs()
    got = be.run_batch(reqs)
    state = be._get_state(resolve_embed_model(router), "t")
    Q = np.asarray([_gauss_vec(r.query) for r in reqs], dtype=np.float32)
    k = min(300, state["index"].max_k(len(reqs)))
    sc, ids = state["index"].search(Q, k)
    text = be.text_search.search_batch(queries=[[r.query] for r in reqs], top_k=300)
    for g, r in enumerate(reqs):
        pool = max(r.top_k, 100)
        dense_hits = [{"id": fusion.raw_hit_id(state["rows"][int(i)]), "score": float(s), "meta": fusion.row_meta(state["rows"][int(i)], "dense")}
                      for s, i in zip(sc[g, :pool], ids[g, :pool]) if i >= 0]
        dn = fusion.dedupe_by_norm_id(dense_hits)
        fused = fusion.fuse_channels(text[g][:pool], [], {nid: h["score"] for nid, h in dn.items()}, top_k=10 ** 9, **_args(fc.ALPHAS))
        for h in fused:
            if not h["meta"].get("text") and h["id"] in dn:
                meta = dict(dn[h["id"]]["meta"])
                meta.update({key: v for key, v in h["meta"].items() if key.startswith("score_")})
                h["meta"] = meta
        assert got[g]["hits"] == fused[:r.top_k], (g, r.query)
        assert got[g]["diagnostics"]["dense_scored"] == len(dn) and got[g]["diagnostics"]["bm25_candidates"] == len(text[g][:pool])
    corpus.drop_shared("dense-index|"); corpus.drop_shared("bm25-index|")


def test_a_failing_embedder_degrades_to_text_only_hits(tmp_path):
    from mrag_amd import corpus, fusion
    from mrag_amd.backend import DenseRetrievalBackend
    path = tmp_path / "docs.jsonl"
    corpus.write_docs_jsonl(path, _rows()[:200])
    be = DenseRetrievalBackend(_BrokenRouter(), index_path=str(path), text_channel="bm25", dense_pool_k=50, fuse_on_device=True)
    reqs = _reqs()[:5]
    got = be.run_batch(reqs)                                                    # nothing is raised
    for g, r in enumerate(reqs):
        assert "provider down" in got[g]["diagnostics"]["dense_error"] and got[g]["diagnostics"]["dense_scored"] == 0
        t_hits = be.text_search.search(queries=[r.query], top_k=max(r.top_k, 50))
        assert got[g]["hits"] == fusion.fuse_channels(t_hits, [], {}, top_k=r.top_k, **_args(fc.ALPHAS)) and got[g]["hits"]
    corpus.drop_shared("bm25-index|")


def test_an_injected_bm25_searcher_is_fused_by_id_not_by_position(docs):
    """a searcher handed in over another corpus of the same length numbers its documents differently from the dense rows:
    its hits must be keyed by their ids, as ``run`` keys them, never by their positions"""
    from mrag_amd.backend import DenseRetrievalBackend
    from mrag_amd.text_index import HipBM25Index, HipBM25TextSearcher
    ix = HipBM25Index(rows=_rows()[::-1])                                       # same 800 rows, reversed positions
    be = DenseRetrievalBackend(_Router(_pm1_vec), index_path=docs, text_channel="bm25", dense_pool_k=100, fuse_on_device=True,
                               text_search=HipBM25TextSearcher(ix))
    reqs = _reqs()[:6]
    got = be.run_batch(reqs)
    for g, r in enumerate(reqs):
        want = be.run(r)
        assert got[g]["hits"] == want["hits"] and want["hits"], (g, r.query)
        assert got[g]["diagnostics"]["bm25_candidates"] == want["diagnostics"]["bm25_candidates"] > 0
    ix.close()
