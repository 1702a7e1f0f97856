"""The host side of the batched hybrid retrieval, and what its GPU tests can see -- no kernel runs here.  The new C entry
point is declared, bound and exported; ``corpus_norm_keys`` and the numpy entry assembly are checked against
``fusion.fuse_channels`` on the hit dicts ``run`` would have built; the degenerate calls need no device; and every case
of ``tests/fuse_batch_cases.py`` meets the condition it was built for, established with ``fuse_channels`` and the array
restatement tied to it.
"""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

import fuse_batch_cases as fc
from mrag_amd import fusion

ROOT = Path(__file__).resolve().parents[1]
NEW = {"mrag_fuse_topk_batch": 19}
ARGS = dict(alpha_text=fc.ALPHAS[0], alpha_graph=fc.ALPHAS[1], alpha_dense=fc.ALPHAS[2])


# ------------------------------------------------------------------------------------------------ ABI and binding
def test_abi_declares_binds_and_exports_the_batch_fusion():
    from mrag_amd import _native as N
    hdr = (ROOT / "include" / "mrag_fuse_batch.h").read_text()
    mrag_h = (ROOT / "include" / "mrag.h").read_text()
    assert '#include "mrag_fuse_batch.h"' in mrag_h and '#include "mrag_bm25_batch.h"' in mrag_h
    declared = {m.group(1): m.group(2) for m in re.finditer(r"^int\s+(mrag_\w+)\(([^;]*)\);", hdr, flags=re.M | re.S)}
    assert set(declared) == set(NEW) == set(N.FUSE_BATCH_SIGNATURES)
    for name, nargs in NEW.items():
        assert len(declared[name].split(",")) == nargs and len(N.FUSE_BATCH_SIGNATURES[name]) == nargs
    assert "retrieval_backend.py:336-372" in hdr
    assert len(N.SIGNATURES) == 64 and len(N.EXTENSION_SIGNATURES) == 2            # the earlier tables are as they were
    assert not set(NEW) & (set(N.SIGNATURES) | set(N.EXTENSION_SIGNATURES))
    assert N.lib_path().exists(), "libmrag_hip.so is not built"
    assert hasattr(ctypes.CDLL(str(N.lib_path())), "mrag_fuse_topk_batch")


# ------------------------------------------------------------------------------------------------ corpus_norm_keys
ROWS = [
    {"doc_id": "Title 9#0", "title": "Title 9", "sent_id": 0, "text": "a"},       # sent_id 0 is falsy: prints as ''
    {"doc_id": "Title 10#1", "title": "Title 10", "sent_id": 1, "text": "b"},     # "Title 10" < "Title 9" by code point
    {"doc_id": "Title 9#1", "title": "Title 9", "sent_id": 1, "text": ""},        # empty text
    {"doc_id": "Title 9#1 again", "title": "Title 9", "sent_id": 1, "text": "d"},  # same title and sent_id: same normalised id
    {"doc_id": "loose#3", "sent_id": 3, "text": "e"},                             # no title: the raw id is the normalised id
    {"doc_id": "Title 10#0", "title": "Title 10", "sent_id": 0, "text": "f"},
    {"doc_id": "Title 9#0 again", "title": "Title 9", "sent_id": 0, "text": "g"},  # duplicate of row 0's id
    {"doc_id": "Title 2#7", "title": "Title 2", "sent_id": 7, "text": "h"},
]


def _hit(row, source, score):
    return {"id": fusion.raw_hit_id(row), "score": score, "meta": fusion.row_meta(row, source)}


def test_corpus_norm_keys_are_order_isomorphic_to_the_normalised_ids():
    keys, sorted_ids = fusion.corpus_norm_keys(ROWS)
    assert keys.dtype == np.int32 and keys.shape == (len(ROWS),)
    nids = [fusion.normalize_id(_hit(r, "bm25", 1.0))[0] for r in ROWS]
    assert nids[0] == "sent::Title 9::" and nids[4] == "sent::loose#3::3" and nids[2] == nids[3] and nids[0] == nids[6]
    assert sorted_ids == sorted(set(nids)) and [sorted_ids[k] for k in keys] == nids
    for a in range(len(ROWS)):
        for b in range(len(ROWS)):
            assert (keys[a] < keys[b]) == (nids[a] < nids[b]) and (keys[a] == keys[b]) == (nids[a] == nids[b])
    assert keys[1] < keys[0] and nids[1] < nids[0]                                # code-point order, not numeric order
    k0, ids0 = fusion.corpus_norm_keys([])
    assert k0.shape == (0,) and ids0 == []


# ------------------------------------------------------------------------------------------------ entry assembly
def test_entries_from_result_arrays_fuse_like_the_hit_dicts_of_run():
    keys, sorted_ids = fusion.corpus_norm_keys(ROWS)
    # two questions; list widths 5 (text) and 6 (dense); question 1 has fewer text hits, a short pool and a missing dense slot
    t_docs = np.asarray([[3, 2, 0, 6, 7], [5, 1, -1, -1, -1]], dtype=np.int64)
    t_sc = np.asarray([[4.0, 4.0, 2.5, 2.5, 1.0], [3.0, 0.5, 0.0, 0.0, 0.0]])
    t_n = np.asarray([5, 2], dtype=np.int32)
    d_ids = np.asarray([[2, 3, 4, 0, 6, 1], [7, 5, 4, 1, -1, -1]], dtype=np.int64)
    d_sc = np.asarray([[0.75, 0.75, 0.5, 0.25, 0.3125, -0.5], [0.5, 0.25, 0.25, 0.125, -np.inf, -np.inf]], dtype=np.float32)
    pool = [6, 3]
    ptr, ek, es, ep = fusion.batch_entries(t_docs, t_sc, t_n, d_ids, d_sc, keys, pool=pool)
    assert ptr.dtype == np.int32 and ptr.tolist() == [0, 5, 5, 11, 13, 13, 16]
    assert ek.dtype == np.int32 and es.dtype == np.float64 and ep.dtype == np.int32
    for g in range(2):
        nt, nd = min(int(t_n[g]), pool[g]), int((d_ids[g, :pool[g]] >= 0).sum())
        # what run() builds: text hits, dense hits deduped by normalised id
        t_hits = [_hit(ROWS[int(d)], "bm25", float(s)) for d, s in zip(t_docs[g, :nt], t_sc[g, :nt])]
        dn = fusion.dedupe_by_norm_id([_hit(ROWS[int(i)], "dense", float(s)) for s, i in zip(d_sc[g, :pool[g]], d_ids[g, :pool[g]]) if i >= 0])
        want = fusion.fuse_channels(t_hits, [], {nid: h["score"] for nid, h in dn.items()}, top_k=10 ** 9, **ARGS)
        # the entries, decoded back through sorted_ids
        a, b, c = int(ptr[3 * g]), int(ptr[3 * g + 1]), int(ptr[3 * g + 3])
        assert (b - a, c - b, int(ptr[3 * g + 2])) == (nt, nd, b)
        assert ep[a:b].tolist() == t_docs[g, :nt].tolist() and [int(keys[r]) for r in ep[a:c]] == ek[a:c].tolist()
        e_hits = [{"id": sorted_ids[int(k)], "score": float(s), "meta": fusion.row_meta(ROWS[int(r)], "bm25")}
                  for k, s, r in zip(ek[a:b], es[a:b], ep[a:b])]
        e_dense = {}
        for k, s in zip(ek[b:c], es[b:c]):
            if sorted_ids[int(k)] not in e_dense or s > e_dense[sorted_ids[int(k)]]:
                e_dense[sorted_ids[int(k)]] = float(s)
        got = fusion.fuse_channels(e_hits, [], e_dense, top_k=10 ** 9, **ARGS)
        assert got == want and len(want) >= 4
    assert es[5:11].tolist() == [float(v) for v in d_sc[0]]                       # fp32 widened exactly
    empty = fusion.batch_entries(np.zeros((0, 4), dtype=np.int64), np.zeros((0, 4)), np.zeros(0, dtype=np.int32),
                                 np.zeros((0, 3), dtype=np.int64), np.zeros((0, 3), dtype=np.float32), keys)
    assert empty[0].tolist() == [0] and all(a.shape == (0,) for a in empty[1:])


# ------------------------------------------------------------------------------------------------ degenerate calls
def test_degenerate_calls_need_no_device():
    from mrag_amd.backend import DenseRetrievalBackend
    assert fusion.fuse_channels_device_batch([], top_k=5, **ARGS) == []
    assert fusion.fuse_channels_device_batch([([], [], {}), ([{"id": "a", "score": 1.0}], [], {})], top_k=[5, 0], **ARGS) == [[], []]
    be = DenseRetrievalBackend(router=None, index_path="/nonexistent/docs.jsonl", text_channel="bm25")
    assert be.run_batch([]) == [] and be.retrieve_batch([]) == []
    out = fusion.fuse_entries_device_batch(np.zeros(1, dtype=np.int32), [], [], None, top_k=3, **ARGS)
    assert [a.shape for a in out[:5]] == [(0, 0)] * 5 and out[5] is None and out[6].shape == (0,)
    with pytest.raises(ValueError):
        fusion.fuse_entries_device_batch(np.zeros(3, dtype=np.int32), [], [], None, top_k=3, **ARGS)


# ------------------------------------------------------------------------------------------------ the cases
def _host(q, alphas=fc.ALPHAS):
    t, g, d = fc.as_channels(q)
    return fusion.fuse_channels(t, g, d, alpha_text=alphas[0], alpha_graph=alphas[1], alpha_dense=alphas[2], top_k=q["top_k"])


def _same_as_host(q, alphas=fc.ALPHAS):
    ref, host = fc.reference(q, alphas), _host(q, alphas)
    assert [(fc.key_id(r[0]), r[1]) for r in ref] == [(h["id"], h["score"]) for h in host]
    assert [r[2:5] for r in ref] == [(h["meta"]["score_text_norm"], h["meta"]["score_graph_norm"], h["meta"]["score_dense_norm"]) for h in host]
    return ref


def test_the_array_restatement_is_fuse_channels():
    """on every case without a negative zero (a hit's -0.0 does not survive ``or 0.0`` on the host)"""
    qs = fc.size_questions() + fc.position_questions() + [fc.filler(g) for g in range(12)] + list(fc.channel_questions().values())
    qs += [fc.tie_question(k) for k in (1, 3, 6)] + fc.cut_questions()[0]
    qs += [q for name, q in fc.dedupe_questions().items() if "zeros" not in name]
    for q in qs:
        _same_as_host(q)
        _same_as_host(q, fc.ZERO_ALPHAS)


def test_size_cases_cover_the_limit_and_have_duplicates_and_ties():
    qs = fc.size_questions()
    assert [sum(q["n"]) for q in qs] == list(fc.SIZES) and max(fc.SIZES) == fusion.FUSE_MAX_ENTRIES == 4096
    for q in qs:
        if sum(q["n"]) >= 63:
            ref = fc.reference(q)
            assert all(q["n"]) and len(ref) < sum(q["n"])                          # every channel used; duplicates exist
            fused = [r[1] for r in ref]
            assert len(set(fused)) < len(fused)                                    # ties of the fused score


def test_channel_and_dedupe_cases_are_what_they_say():
    ch = fc.channel_questions()
    assert ch["only text"]["n"][1:] == (0, 0) and ch["only graph"]["n"][::2] == (0, 0) and ch["only dense"]["n"][:2] == (0, 0)
    for name in ("only text", "only graph", "only dense"):
        assert [r[0] for r in fc.reference(ch[name])] == [1, 3, 7]                 # key 1 deduped to its larger score
    assert all(r[2] == 0.0 for r in fc.reference(ch["all-equal channel"]))
    assert min(ch["negative scores"]["scores"]) < 0 and max(ch["negative scores"]["scores"]) < 0
    present = {r[0]: sum(p >= 0 for p in r[5]) for r in fc.reference(ch["one, two and three channels"])}
    assert sorted(present.values()) == [1, 1, 1, 1, 2, 3]
    # an alpha of 0 really reorders: the text-only key drops to the bottom
    q = ch["one, two and three channels"]
    assert [r[0] for r in fc.reference(q)] != [r[0] for r in fc.reference(q, fc.ZERO_ALPHAS)]
    dd = fc.dedupe_questions()
    assert {r[0]: r[5][0] for r in fc.reference(dd["five equal"])}[4] == 1          # first of the five equal entries
    assert {r[0]: r[5][2] for r in fc.reference(dd["later larger"])}[4] == 3        # the first of the two 2.0
    # signed zeros: the rule and a bitwise ordering disagree, visibly
    for name in ("zeros as duplicates, -0 first", "zeros as duplicates, +0 first"):
        assert {r[0]: r[5][0] for r in fc.reference(dd[name])}[4] == 0             # first met, in both orders
    assert {r[0]: r[5][0] for r in fc.reference(dd["zeros as duplicates, -0 first"], bitwise=True)}[4] == 1
    # as a channel's min: lo = +0.0, the first met, gives -0.0 - 0.0 = -0.0; the bitwise min -0.0 gives +0.0.  (As a max
    # the zero's sign cancels in hi - lo: those cases only have to come out like the single call's.)
    right, wrong = fc.reference(dd["zeros as min, +0 first"]), fc.reference(dd["zeros as min, +0 first"], bitwise=True)
    signs = lambda rows: [[math.copysign(1.0, v) for v in r[1:5]] for r in rows]       # noqa: E731
    assert right == wrong and signs(right) != signs(wrong)                         # equal as numbers, different as bits


def test_tie_and_cut_cases_straddle_top_k():
    full = fc.reference(fc.tie_question(10 ** 9))
    assert [r[0] for r in full] == [1, 2, 4, 6, 8, 9] and len({r[1] for r in full[1:5]}) == 1
    assert full[0][1] > full[1][1] > full[5][1]
    assert [r[0] for r in fc.reference(fc.tie_question(3))] == [1, 2, 4]            # the cut falls inside the tie group
    qs, distinct = fc.cut_questions()
    assert [len(fc.reference(q)) for q in qs] == [0, 1, distinct, distinct] and distinct > 5
