"""GPU parity of the filtered search (DenseIndex.search(allow=...), mrag_index_search_filtered): the top-k of the allowed
rows only, on both execution paths (mask: the FILT kernel instances; compact: gathered rows + the unchanged search) and
AUTO, against the fp64 oracle over c16[allowed] with ids mapped through np.flatnonzero(allowed)."""
import os
import subprocess
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

from oracle import dense_search as ds
from oracle import ref_semantics as rs

pytestmark = pytest.mark.gpu
TOL = 1e-5
PATHS = ("mask", "compact", "auto")


def _index(c16, id_base=0, **kw):
    from mrag_amd.index import DenseIndex
    ix = DenseIndex(c16.shape[1], **kw)
    if id_base:
        ix.set_id_base(id_base)
    ix.add(c16, normalize=False)
    return ix


def _oracle(q16, c16, mask, k, id_base=0):
    rows = np.flatnonzero(mask)
    if rows.size == 0:
        return np.full((q16.shape[0], k), -np.inf), np.full((q16.shape[0], k), -1, dtype=np.int64)
    rv, ri = ds.brute_force_topk(q16, c16[rows], k)
    return rv, np.where(ri >= 0, rows[np.maximum(ri, 0)] + id_base, -1)


def _check_result(sc, ids, rv, ri, tol=TOL):
    assert sc.shape == rv.shape and ids.dtype == np.int64
    valid = ri >= 0
    assert ((ids >= 0) == valid).all()
    assert np.isneginf(sc[~valid]).all() and (ids[~valid] == -1).all()
    np.testing.assert_allclose(sc[valid], rv[valid], rtol=0, atol=tol)
    assert (np.diff(sc, axis=1)[valid[:, 1:]] <= 0).all()            # descending
    strict, bad = ds.gap_aware_id_match(ids, sc, ri, rv, tol=tol)
    assert bad == 0, (strict, bad)


def _check(ix, q16, c16, mask, k, path, id_base=0, allow=None):
    sc, ids = ix.search(q16, k, normalize=False, allow=mask if allow is None else allow, filter_path=path)
    rv, ri = _oracle(q16, c16, mask, k, id_base)
    _check_result(sc, ids, rv, ri)
    lf = ix.last_filter()
    assert lf["allowed"] == int(mask.sum())
    if path != "auto":
        assert lf["path"] == path
    return sc, ids


def _mask(n, sel, seed):
    rng = np.random.default_rng(seed)
    m = rng.random(n) < sel
    if not m.any():
        m[rng.integers(0, n)] = True
    return m


# (nq, n, d, k): streaming (nq <= 16, and nq <= 8 with k > 32), dense batch (nq > 16, k <= 64; 17 000 queries = two
# launches of the query-batch loop), wide batch (nq > 32, 64 < k <= 256, >= 64 corpus tiles); dims not multiples of 64
SHAPES = [(1, 20000, 384, 10), (5, 30000, 200, 100), (16, 5000, 96, 20),
          (300, 20000, 768, 10), (40, 3000, 130, 64), (17000, 4000, 64, 5),
          (100, 20000, 72, 200)]
SELS = (0.002, 0.1, 0.6)


@pytest.fixture(scope="module")
def grid_data():
    cache = {}

    def get(nq, n, d):
        if (nq, n, d) not in cache:
            c16 = ds.normalize_round(ds.make_gaussian(n, d, 1000 + d))
            q16 = ds.normalize_round(ds.make_gaussian(nq, d, 2000 + nq))
            cache[(nq, n, d)] = (c16, q16, _index(c16))
        return cache[(nq, n, d)]
    yield get
    for c16, q16, ix in cache.values():
        ix.close()


@pytest.mark.parametrize("nq,n,d,k", SHAPES)
@pytest.mark.parametrize("sel", SELS)
def test_filtered_grid(grid_data, nq, n, d, k, sel):
    c16, q16, ix = grid_data(nq, n, d)
    mask = _mask(n, sel, seed=nq + n + int(sel * 1000))
    rv, ri = _oracle(q16, c16, mask, k)
    for path in PATHS:
        sc, ids = ix.search(q16, k, normalize=False, allow=mask, filter_path=path)
        _check_result(sc, ids, rv, ri)
        lf = ix.last_filter()
        assert lf["allowed"] == int(mask.sum())
        assert lf["path"] == path if path != "auto" else lf["path"] in ("mask", "compact")


@pytest.mark.parametrize("path", ("mask", "compact"))
def test_fewer_allowed_than_k_and_none(path):
    c16 = ds.normalize_round(ds.make_gaussian(3000, 128, 11))
    q16 = ds.normalize_round(ds.make_gaussian(40, 128, 12))
    ix = _index(c16)
    mask = np.zeros(3000, dtype=bool)
    mask[[5, 700, 701, 2999, 1234]] = True
    for nq, k in ((40, 10), (1, 10), (40, 100)):
        _check(ix, q16[:nq], c16, mask, k, path)
    none = np.zeros(3000, dtype=bool)
    for nq, k in ((40, 10), (1, 200)):
        sc, ids = ix.search(q16[:nq], k, normalize=False, allow=none, filter_path=path)
        assert np.isneginf(sc).all() and (ids == -1).all()
        assert ix.last_filter() == {"path": path, "allowed": 0}
    ix.close()


@pytest.mark.parametrize("nq,n,d,k", [(1, 20000, 384, 10), (8, 20000, 128, 200), (300, 20000, 256, 10),
                                      (40, 3000, 130, 64), (100, 20000, 72, 200)])
def test_all_allowed_is_bit_identical(nq, n, d, k):
    c16 = ds.normalize_round(ds.make_gaussian(n, d, 21))
    q16 = ds.normalize_round(ds.make_gaussian(nq, d, 22))
    ix = _index(c16, id_base=77)
    s0, i0 = ix.search(q16, k, normalize=False)
    everything = np.ones(n, dtype=bool)
    for path in ("mask", "compact"):
        s1, i1 = ix.search(q16, k, normalize=False, allow=everything, filter_path=path)
        assert np.array_equal(s0, s1) and np.array_equal(i0, i1), path
    ix.close()


@pytest.mark.parametrize("path", ("mask", "compact"))
def test_one_allowed_row_per_tile(path):
    """Every 256-row tile has ONE allowed row: no lane has two, so the first-tile certificate is -inf on every tile."""
    n, d = 20000, 128
    c16 = ds.normalize_round(ds.make_gaussian(n, d, 31))
    q16 = ds.normalize_round(ds.make_gaussian(300, d, 32))
    ix = _index(c16)
    mask = np.zeros(n, dtype=bool)
    rng = np.random.default_rng(33)
    for t0 in range(0, n, 256):
        mask[t0 + rng.integers(0, min(256, n - t0))] = True
    for nq, k in ((300, 10), (300, 64), (1, 10), (40, 100)):
        _check(ix, q16[:nq], c16, mask, k, path)
    ix.close()


@pytest.mark.parametrize("path", ("mask", "compact"))
def test_allowed_only_in_partial_last_tile(path):
    n, d = 5000, 96                                  # last tile: rows 4864 .. 4999
    c16 = ds.normalize_round(ds.make_gaussian(n, d, 41))
    q16 = ds.normalize_round(ds.make_gaussian(64, d, 42))
    ix = _index(c16)
    mask = np.zeros(n, dtype=bool)
    mask[4870:5000:3] = True
    for nq, k in ((64, 10), (1, 10), (64, 100)):
        _check(ix, q16[:nq], c16, mask, k, path)
    ix.close()


@pytest.mark.parametrize("path", ("mask", "compact"))
def test_identical_rows_tie_break_row_ascending(path):
    """Identical rows score identically: ids must follow the row-ascending tie-break through the compaction."""
    d = 64
    base = ds.normalize_round(ds.make_gaussian(50, d, 51))
    c16 = np.repeat(base, 80, axis=0)[np.random.default_rng(52).permutation(4000)]
    q16 = ds.normalize_round(ds.make_gaussian(30, d, 53))
    ix = _index(c16)
    mask = _mask(4000, 0.4, 54)
    for nq, k in ((30, 16), (1, 16), (30, 120)):
        sc, ids = ix.search(q16[:nq], k, normalize=False, allow=mask, filter_path=path)
        rv, ri = _oracle(q16[:nq], c16, mask, k)
        _check_result(sc, ids, rv, ri)
        for srow, irow in zip(sc, ids):                # equal scores: rows ascending
            same = srow[1:] == srow[:-1]
            assert (irow[1:][same] > irow[:-1][same]).all()
        assert (ids == ri).mean() > 0.99
    ix.close()


@pytest.mark.parametrize("path", ("mask", "compact"))
def test_adversarial_increasing_scores_filtered(path):
    """test_adversarial_increasing_scores_large_k's layout (every tile beats the last), every third row allowed."""
    d, n, nq, k = 64, 6000, 300, 48
    u = ds.l2_normalize(ds.make_gaussian(1, d, 9))[0]
    a = np.linspace(0.05, 1.0, n, dtype=np.float32)
    c = (a[:, None] * u[None, :]).astype(np.float16)
    q = ds.normalize_round(u[None, :] + 0.01 * ds.make_gaussian(nq, d, 10))
    from mrag_amd.index import DenseIndex
    ix = DenseIndex(d, metric="ip")
    ix.add(c, normalize=False)
    mask = np.zeros(n, dtype=bool)
    mask[::3] = True
    _check(ix, q, c, mask, k, path)
    _check(ix, q[:4], c, mask, k, path)
    ix.close()


@pytest.mark.parametrize("path", PATHS)
def test_bf16_and_id_base(path):
    n, d = 9000, 192
    x = ds.make_gaussian(n, d, 61)
    c = ds.l2_normalize(x)
    from mrag_amd.index import DenseIndex
    ix = DenseIndex(d, dtype="bf16")
    ix.set_id_base(123_456)
    ix.add(c.astype(np.float32), normalize=False)
    cb = ix.rows()                                   # the stored bf16 values, widened
    q = ds.l2_normalize(ds.make_gaussian(50, d, 62)).astype(np.float32)
    qb = ix_round_bf16(q)
    mask = _mask(n, 0.05, 63)
    for nq, k in ((50, 10), (2, 100)):
        sc, ids = ix.search(qb[:nq], k, normalize=False, allow=mask, filter_path=path)
        rv, ri = _oracle(qb[:nq], cb, mask, k, id_base=123_456)
        _check_result(sc, ids, rv, ri)
    ix.close()


def ix_round_bf16(x):
    """fp32 -> bf16 (round to nearest even) -> fp32: the query bits the index prepares from fp32 input."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32)


def test_device_queries_device_mask_stream_out_reuse():
    import torch
    n, d, k = 20000, 256, 10
    c16 = ds.normalize_round(ds.make_gaussian(n, d, 71))
    q16 = ds.normalize_round(ds.make_gaussian(500, d, 72))
    ix = _index(c16, id_base=10)
    mask = _mask(n, 0.03, 73)
    rv, ri = _oracle(q16, c16, mask, k, id_base=10)
    q = torch.from_numpy(q16).cuda()
    s = torch.cuda.Stream()
    out = (torch.empty((500, k), dtype=torch.float32, device="cuda"), torch.empty((500, k), dtype=torch.int64, device="cuda"))
    for path in PATHS:
        for dt in (torch.bool, torch.uint8):
            am = torch.from_numpy(mask).to(dtype=dt).cuda()
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                out[0].fill_(7.0)
                sc, ids = ix.search(q, k, normalize=False, allow=am, filter_path=path, stream=s, out=out)
            assert sc.data_ptr() == out[0].data_ptr() and ids.data_ptr() == out[1].data_ptr()
            s.synchronize()
            _check_result(sc.cpu().numpy(), ids.cpu().numpy(), rv, ri)
            assert ix.last_filter()["allowed"] == int(mask.sum())
            # single-query streaming regime with a device mask
            with torch.cuda.stream(s):
                s1, i1 = ix.search(q[:1], 50, normalize=False, allow=am, filter_path=path, stream=s)
            s.synchronize()
            r1v, r1i = _oracle(q16[:1], c16, mask, 50, id_base=10)
            _check_result(s1.cpu().numpy(), i1.cpu().numpy(), r1v, r1i)
    ix.close()


@pytest.mark.parametrize("path", PATHS)
def test_host_row_positions(path):
    n, d = 12000, 128
    c16 = ds.normalize_round(ds.make_gaussian(n, d, 81))
    q16 = ds.normalize_round(ds.make_gaussian(70, d, 82))
    ix = _index(c16)
    pos = np.random.default_rng(83).choice(n, size=900, replace=False)
    mask = np.zeros(n, dtype=bool)
    mask[pos] = True
    _check(ix, q16, c16, mask, 10, path, allow=pos)
    _check(ix, q16[:3], c16, mask, 10, path, allow=pos.astype(np.int32))
    ix.close()


def test_unfiltered_after_filtered_is_unchanged():
    n, d = 20000, 128
    c16 = ds.normalize_round(ds.make_gaussian(n, d, 91))
    q16 = ds.normalize_round(ds.make_gaussian(300, d, 92))
    ix = _index(c16)
    before = {(nq, k): ix.search(q16[:nq], k, normalize=False) for nq, k in ((300, 10), (1, 10), (100, 200), (4, 100))}
    for path in ("mask", "compact"):
        for nq, k in before:
            ix.search(q16[:nq], k, normalize=False, allow=_mask(n, 0.01, nq + k), filter_path=path)
        for (nq, k), (s0, i0) in before.items():
            s1, i1 = ix.search(q16[:nq], k, normalize=False)
            assert np.array_equal(s0, s1) and np.array_equal(i0, i1), (path, nq, k)
    ix.close()


SHARDED_WORKER = r"""
import os, sys
sys.path.insert(0, os.environ["MRAG_ROOT"])
import numpy as np, torch, torch.distributed as dist
from mrag_amd.sharded import ShardedDenseIndex, shard_bounds
from mrag_amd.index import DenseIndex
from oracle import dense_search as ds
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo")
torch.cuda.set_device(0)
n, nq, d, k = 50_001, 300, 128, 10
c16 = ds.normalize_round(ds.make_gaussian(n, d, 1234)); q16 = ds.normalize_round(ds.make_gaussian(nq, d, 5678))
lo, hi = shard_bounds(n, world, rank)
sh = ShardedDenseIndex(d, n, rank, world, device=0)
sh.add_local(torch.from_numpy(c16[lo:hi]).cuda(), normalize=False)
one = DenseIndex(d); one.add(torch.from_numpy(c16).cuda(), normalize=False)
q = torch.from_numpy(q16).cuda()
rng = np.random.default_rng(7)
mask = rng.random(n) < 0.02
only_first = np.zeros(n, dtype=bool); only_first[100:400] = True          # ranks 1 and 2 have no allowed row
for allow, kk in ((mask, 10), (np.flatnonzero(mask), 10), (only_first, 10), (mask, 200)):
    m = np.zeros(n, dtype=bool); m[allow] = True
    rs_, ri_ = one.search(q, kk, normalize=False, allow=m, filter_path="mask"); torch.cuda.synchronize()
    rs_, ri_ = rs_.cpu().numpy(), ri_.cpu().numpy()
    for mode in ("device", "host"):
        for pipe in (False, True):
            s_, i_ = sh.search(q, kk, merge=mode, pipeline=pipe, normalize=False, allow=allow)
            assert (i_ == ri_).all() and np.array_equal(s_, rs_), (mode, pipe, kk, "sharded filtered != one index")
rows = np.flatnonzero(mask)
ov, oi = ds.brute_force_topk(q16[:64], c16[rows], 10)
s_, i_ = sh.search(q, 10, normalize=False, allow=mask)
assert ds.gap_aware_id_match(i_[:64], s_[:64], rows[oi], ov, tol=1e-5)[1] == 0
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_three_ranks_filtered_on_one_gpu(tmp_path):
    root = Path(__file__).resolve().parent.parent
    script = tmp_path / "ranks_filtered.py"
    script.write_text(SHARDED_WORKER)
    env = dict(os.environ, MRAG_ROOT=str(root), MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3",
                        "--master-addr", "127.0.0.1", "--master-port", "29653", str(script)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == 3


def _title_filter(req, rows):
    """Module-level so that the "pkg.mod:func" form can name it: only passages whose title ends in 3."""
    return np.array([str(r.get("title", "")).endswith("3") for r in rows], dtype=bool)


def test_backend_dense_row_filter(tmp_path):
    from mrag_amd import corpus, fusion
    from mrag_amd.backend import DenseRetrievalBackend
    from mrag_amd.dto import RetrievalIn
    dim = 96

    def text_vec(text):
        rng = np.random.default_rng(zlib.crc32(text.encode("utf-8")))
        return [float(x) for x in rng.standard_normal(dim)]

    class Prov:
        kwargs = {"embed_model": "fake-embed"}
        def embed(self, *, model, texts, require):
            return {"vectors": [text_vec(t) for t in texts]}

    class Router:
        providers, policy = {"hip": Prov()}, {"embedding_provider": "hip"}
        def embed(self, *, model_hint, texts, require=None):
            return rs.router_embed(self.providers, self.policy, model_hint=model_hint, texts=texts, require=require)

    rows = [{"doc_id": f"T{i // 4}#{i % 4}", "title": f"T{i // 4}", "sent_id": i % 4,
             "text": f"sentence {i} about topic {i % 37} and {i % 11}"} for i in range(1500)]
    docs = tmp_path / "docs.jsonl"
    corpus.write_docs_jsonl(docs, rows)
    kw = dict(index_path=str(docs), embed_batch=256, dense_pool_k=200)
    req = RetrievalIn(query="topic 3 and 4", graph_id="", top_k=20, trace_id="t")
    corpus.drop_shared("dense-index|")
    plain = DenseRetrievalBackend(Router(), **kw).run(req)
    assert "dense_filter" not in plain["diagnostics"] and plain["diagnostics"]["dense_error"] is None
    mask = _title_filter(req, rows)
    c16 = ds.normalize_round(np.asarray([text_vec(r["text"]) for r in rows], dtype=np.float32))
    q16 = ds.normalize_round(np.asarray([text_vec(req.query)], dtype=np.float32))
    sv, si = _oracle(q16, c16, mask, 200)
    dense_hits = [{"id": fusion.raw_hit_id(rows[int(i)]), "score": float(v), "meta": fusion.row_meta(rows[int(i)], "dense")}
                  for v, i in zip(sv[0], si[0]) if i >= 0]
    dn = rs.norm_map(dense_hits)
    want = rs.fuse([], [], {key: v["score"] for key, v in dn.items()}, alpha_text=0.4, alpha_graph=0.2, alpha_dense=0.4, top_k=20)
    allowed_ids = set(rs.norm_map([{"id": fusion.raw_hit_id(rows[i]), "score": 0.0, "meta": fusion.row_meta(rows[i], "dense")}
                                   for i in np.flatnonzero(mask)]))     # fused hits carry the normalised ids
    for flt in (_title_filter, "test_gpu_filtered:_title_filter", lambda req, rows: np.flatnonzero(_title_filter(req, rows))):
        b = DenseRetrievalBackend(Router(), dense_row_filter=flt, **kw)
        out = b.run(req)
        dg = out["diagnostics"]
        assert dg["dense_error"] is None
        assert dg["dense_filter"]["allowed"] == int(mask.sum()) and dg["dense_filter"]["path"] in ("mask", "compact")
        assert out["hits"] and all(h["id"] in allowed_ids for h in out["hits"])
        assert [h["id"] for h in out["hits"]] == [h["id"] for h in want]
        np.testing.assert_allclose([h["score"] for h in out["hits"]], [h["score"] for h in want], rtol=0, atol=1e-4)
    # a filter that returns None leaves run() exactly as without one
    none = DenseRetrievalBackend(Router(), dense_row_filter=lambda req, rows: None, **kw).run(req)
    assert none == plain
