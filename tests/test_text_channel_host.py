"""What the text channel's GPU tests can see, established on the CPU with the oracle alone (no kernel runs here).

``oracle.bm25.search_postings`` is the expected value of every BM25 case of ``tests/test_gpu_text_channel.py``; here it is
pinned to ``Bm25Oracle.search`` and to F7 (the reference's own outputs) bit for bit.  Then, for every case of
``oracle/text_cases.py``: the condition the case was built for holds on its input, and each mutant it targets changes the
expected output.  Fusion and cosine cases get the same treatment with the host fusion and an exact cosine.  Conditions on
the inputs, not measurements of the code under test.  Run with ``-s`` for the tables.
"""
import json

import numpy as np
import pytest

from oracle import bm25 as ob
from oracle import text_cases as tc


def _build(rows, k1, b):
    from mrag_amd.text_index import build_postings
    return build_postings(rows, k1, b)


def _bits(ranked):
    return [(d, np.float64(s).view(np.uint64)) for d, s in ranked]


# ------------------------------------------------------------------------------------------------ the oracle itself
def test_search_postings_equals_the_dict_oracle_and_f7(golden_dir):
    f7 = json.loads((golden_dir / "f7_bm25.json").read_text())
    n_cases = 0
    for name, c in f7.items():
        o = ob.Bm25Oracle(c["rows"], k1=c["k1"], b=c["b"])
        p = _build(c["rows"], c["k1"], c["b"])
        for case in c["cases"]:
            for top_k in (case["top_k"], 10 ** 9):
                got = ob.search_postings(p, case["queries"], top_k, case["alpha_merge"], c["k1"])
                assert _bits(got) == _bits(o.search(case["queries"], top_k=top_k, alpha_merge=case["alpha_merge"]))
            assert sorted(_bits(got)) == sorted(_bits([tuple(x) for x in case["full"]]))      # F7: every candidate's score
            n_cases += 1
    assert n_cases >= 10
    rows = tc.rows_zipf(*tc.ZIPF_SMALL)
    o, p = ob.Bm25Oracle(rows), _build(rows, 1.5, 0.75)
    for queries in tc.ZIPF_SMALL_QUERIES:
        for merge in ("max", "sum"):
            for k in (1, 50, 6000):
                got = ob.search_postings(p, list(queries), k, merge)
                assert _bits(got) == _bits(o.search(list(queries), top_k=k, alpha_merge=merge)), (queries, merge, k)
    # term ids and idfs given directly are the same search
    ids = ob.query_term_ids(p, list(tc.ZIPF_SMALL_QUERIES[1]))
    assert ob.search_postings(p, ids, 50, "sum") == ob.search_postings(p, list(tc.ZIPF_SMALL_QUERIES[1]), 50, "sum")


# ------------------------------------------------------------------------------------------------ BM25 cases
def _expected(case, postings, mutant=None):
    """{(query set index, merge, k): ranking}; the merged scores are computed once per (query set, merge)."""
    out = {}
    for qi, qs in enumerate(case.query_sets):
        for merge in case.merges:
            fin = ob.merged_scores(postings, list(qs), merge, case.k1, mutant)
            for k in case.ks:
                out[(qi, merge, k)] = _bits(ob.select_topk(fin, k, mutant))
    return out


def _conditions(case, p, want):
    docs = lambda key: np.asarray([d for d, _ in want[key]], dtype=np.int64)
    if case.name.startswith("stride"):
        assert p["N"] == tc.STRIDE_N > tc.GRID
    if case.name.startswith("stride-a"):
        for k in case.ks:
            got = want[(0, "max", k)]
            assert [d for d, _ in got] == list(range(k)) and len({s for _, s in got}) == 1
    if case.name.startswith("stride-b"):
        d = docs((0, "max", 4096))
        assert sorted(d) == list(tc.RARE_DOCS) and len(d) == 37 and (d < tc.GRID).any() and (d >= tc.GRID).any()
    if case.name.startswith("stride-c"):
        for key, got in want.items():
            d, s = docs(key), [b for _, b in got]
            assert (d < tc.GRID).any() and (d >= tc.GRID).any() and len(d) == key[2]
            fin = ob.merged_scores(p, list(case.query_sets[0]), key[1], case.k1)
            groups = sorted(set(fin[fin > 0].view(np.uint64).tolist()), reverse=True)
            assert s[0] == groups[0] and s[-1] == groups[1]                       # the cut lands in the second tie group
            second = np.nonzero(fin.view(np.uint64) == groups[1])[0]
            assert second.min() < tc.GRID <= second.max()                         # which spans the boundary
            assert len(second) > sum(1 for b in s if b == groups[1]) > 0          # and is larger than what is taken
    if case.name.startswith("low-bytes"):
        for k in case.ks:
            fin = ob.merged_scores(p, list(case.query_sets[0]), "max", case.k1)
            top = np.asarray([b for _, b in _bits(ob.select_topk(fin, k + 1))], dtype=np.uint64)
            assert len(set(top.tolist())) == k + 1 and len(set((top >> np.uint64(24)).tolist())) == 1
    if case.name == "many-queries":
        qs = case.query_sets[0]
        assert len(qs) == tc.BM25_MAX_QUERIES and "" in qs and max(len(q.split()) for q in qs) == 12
        ids = ob.query_term_ids(p, list(qs))
        assert any(-1 in i for i, _ in ids) and sum(len(set(i)) < len(i) for i, _ in ids) > 100
        assert p["N"] == 20_000 and all(len(r) == 200 for r in want.values())
    if case.name == "negative-idf":
        for (qi, merge, k), got in want.items():
            fin = ob.merged_scores(p, list(case.query_sets[qi]), merge, case.k1)
            assert all(fin[d] > 0 for d, _ in got)
        assert any((ob.merged_scores(p, list(qs), "sum", case.k1) < 0).sum() > 50 for qs in case.query_sets)
    if case.name.startswith("small"):
        assert p["N"] == case.ks[0] and case.top_k == 10 ** 9
        assert want[(3, "max", p["N"])] == [] and want[(4, "sum", p["N"])] == []        # unknown terms only; empty strings only
        assert p["N"] < 200 or any(len(r) > 128 for r in want.values())


@pytest.mark.parametrize("case", tc.BM25_CASES, ids=lambda c: c.name)
def test_bm25_case_conditions_and_mutants(case):
    p = tc.bm25_postings(case, _build)
    want = _expected(case, p)
    _conditions(case, p, want)
    missed = []
    print(f"\n{case.name}: N = {p['N']}, {len(want)} searches")
    for m in ob.POSTINGS_MUTANTS:
        got = _expected(case, p, m)
        seen = [key for key in want if got[key] != want[key]]
        print(f"  {m:18s} {'seen in %d of %d' % (len(seen), len(want)) if seen else 'not seen':16s}"
              + ("" if m in case.targets else "   (not a target)"))
        if m in case.targets and not seen:
            missed.append(m)
    assert not missed, missed


def test_every_bm25_mutant_is_a_target_somewhere():
    for m in ob.POSTINGS_MUTANTS:
        assert any(m in c.targets for c in tc.BM25_CASES), m
    names = [c.name for c in tc.BM25_CASES]
    assert len(set(names)) == len(names)
    assert {c.ks[0] for c in tc.BM25_CASES if c.name.startswith("small")} == {1, 2, 257}
    assert {(c.k1, c.b) for c in tc.BM25_CASES if c.name.startswith("small")} >= {(0.0, 0.75), (1.5, 0.0), (1.5, 1.0)}


# ------------------------------------------------------------------------------------------------ fusion cases
@pytest.mark.parametrize("case", tc.FUSION_CASES, ids=lambda c: c.name)
def test_fusion_case_conditions(case):
    from mrag_amd import fusion
    text, graph, dense = case.make()
    n = tc.fusion_entries((text, graph, dense))
    tmap, gmap = fusion.dedupe_by_norm_id(text), fusion.dedupe_by_norm_id(graph)
    a = dict(zip(("alpha_text", "alpha_graph", "alpha_dense"), case.alphas))
    full = fusion.fuse_channels(text, graph, dense, top_k=10 ** 9, **a)
    assert len(full) == len(set(tmap) | set(gmap) | set(dense))
    print(f"\n{case.name}: {n} entries = {len(text)} / {len(graph)} / {len(dense)}, {len(full)} ids")
    if "n>1024" in case.wants:
        assert n > 1024            # some thread of the one 1024-thread workgroup takes a second element
    if "n==4096" in case.wants:
        assert n == tc.FUSE_MAX and tc.fusion_entries(tc.fusion_4097()) == tc.FUSE_MAX + 1
    if "duplicates" in case.wants:
        assert len(tmap) < len(text) // 2 and len(gmap) < len(graph) // 2         # the dense channel is a dict: no duplicates
    if "one-two-three" in case.wants:
        count = {nid: (nid in tmap) + (nid in gmap) + (nid in dense) for nid in (h["id"] for h in full)}
        assert {1, 2, 3} <= set(count.values())
    if "ties" in case.wants:
        for top_k in case.top_ks:
            kept = [h["score"] for h in full[:top_k]]
            tied = sum(1 for s in kept if kept.count(s) > 1)
            print(f"  top_k {top_k}: {tied} of {len(kept)} kept hits share their fused score with another")
            assert tied >= 20
            assert [h["id"] for h in full[:top_k]] == [h["id"] for h in sorted(full[:top_k], key=lambda h: (-h["score"], h["id"]))]
    if case.name == "flat-empty-negative":
        assert len({h["score"] for h in text}) == 1 and not graph and max(dense.values()) < 0
        assert any(h["score"] > 0 for h in full) and all(h["meta"]["score_text_norm"] == 0.0 for h in full)
    if case.name == "negative-flat-empty":
        assert max(h["score"] for h in text) < 0 and len({h["score"] for h in graph}) == 1 and not dense


# ------------------------------------------------------------------------------------------------ cosine cases
@pytest.mark.parametrize("dim", sorted(set(tc.COSINE_F64_DIM + tc.COSINE_MATRIX_DIM)))
def test_cosine_reference_sees_a_dropped_element_a_dropped_tail_and_the_wrong_row(dim):
    n = 5
    x, q = tc.cosine_vectors(n, dim, 1), tc.cosine_vectors(1, dim, 2)[0]
    exact = tc.exact_cosine(q, x)
    bar = 100 * tc.cosine_bound(dim)
    # the exact reference agrees with the fp64 formula inside the bound (math.fsum: correctly rounded sums)
    import math
    for e, v in zip(exact, x):
        f = math.fsum(q * v) / (math.sqrt(math.fsum(q * q)) * math.sqrt(math.fsum(v * v)))
        assert abs(f - float(e)) <= 8 * tc.U
    alts = {"last element dropped": tc.exact_cosine(np.append(q[:-1], 0.0), np.hstack([x[:, :-1], np.zeros((n, 1))])),
            "neighbouring row": tc.exact_cosine(q, np.roll(x, -1, axis=0))}
    if dim > 64:
        alts["elements >= 64 dropped"] = tc.exact_cosine(np.append(q[:64], np.zeros(dim - 64)),
                                                         np.hstack([x[:, :64], np.zeros((n, dim - 64))]))
    for what, alt in alts.items():
        if dim == 1 and what == "neighbouring row":
            continue                                   # a 1-dimensional cosine is a sign: a neighbour may share it
        move = min(abs(float(a - e)) for a, e in zip(alt, exact))
        print(f"\ndim {dim}: {what}: moves every value by at least {move:.3e}, bar {bar:.3e}")
        assert move > bar
    # the matrix and adjacent references are the same quotient
    m = tc.exact_matrix(x)
    assert [m[0][j] for j in range(n)] == tc.exact_cosine(x[0], x) and all(m[i][j] == m[j][i] for i in range(n) for j in range(n))
    adj = tc.exact_adjacent(x, 0.0)
    assert all(abs(float(adj[i] - m[i][i + 1])) < 1e-40 for i in range(n - 1))
    assert all(abs(a) < abs(b) for a, b in zip(tc.exact_adjacent(x, 0.5), adj))


def test_cosine_zero_rows_and_the_edge_threshold():
    x = tc.cosine_vectors(5, 7, 3, zero_rows=(0, 4))
    e = tc.exact_cosine(x[1], x)
    assert e[0] == 0 and e[4] == 0 and abs(float(e[1]) - 1.0) < 1e-30
    assert tc.exact_adjacent(x, 1e-9)[0] == 0 and tc.exact_adjacent(x, 1e-9)[3] == 0
    v = tc.clustered_vectors(45, 64, 9)
    m = tc.exact_matrix(v)
    pairs = [float(m[i][j]) for i in range(45) for j in range(i + 1, 45)]
    assert min(abs(p - 0.9) for p in pairs) >= 1e-9                 # >= cannot flip legitimately
    assert 20 < sum(p >= 0.9 for p in pairs) < len(pairs) - 20
    assert tc.cosine_bound(768) == 1544 * 2.0 ** -53
