"""GPU tests of the dense and IVF searches on negative, zero and sign-crossing scores (tests/signed_scores_cases.py): every
selection path -- K2's certificate and radix compactions, K2s narrow and wide, K4 / K4s / K4w, the wide batch's verifier
and redo, the filtered, range, fp8 and per-question-set forms, and the IVF select kernel's register, streamed and serial
paths with its fused regime -- against the fp64 oracle, on exact shifted integers (``==``) and on rounded cosine rows
whose scores are negative or cross zero (1e-5, as tests/test_gpu_bruteforce.py::_check).  What the inputs are and which
mistakes they catch is checked on the CPU in tests/test_signed_scores_host.py."""
import functools
import os
import subprocess
import sys
import tempfile
import textwrap
from pathlib import Path

import numpy as np
import pytest

import signed_scores_cases as sc
from oracle import dense_search as ds

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
DTYPES = ("f16", "bf16")
DENSE_A = [(r[0], k) for r in sc.DENSE for k in r[5]]
DENSE_B = [(r[0], k, s) for r in sc.DENSE for k in r[5] for s in r[6]]
FILTERED_B = [(name, k) for name, k in sc.FILTERED if sc.DENSE_BY_NAME[name][6]]


@pytest.fixture(scope="module", autouse=True)
def _release():
    """the indexes and problems this module caches live as long as the module"""
    yield
    for cached in (_dense_a_index, _dense_b_index, _ivf_a_index, _ivf_b_index):
        cached.cache_clear()                                   # the last reference: the index closes itself
    for cached in (sc.family_a, sc.family_a_masked, sc.family_b, sc.ivf_a, sc.ivf_b, sc.ivf_a_filtered, sc.wide_sorted):
        cached.cache_clear()


def _store(x, dtype):
    """family-A values are exact in both storage types: fp16 bits for an f16 index, fp32 (rounded on the device) for bf16"""
    return np.asarray(x, dtype=np.float16 if dtype == "f16" else np.float32)


@functools.lru_cache(maxsize=None)
def _dense_a_index(n, nq, d, amp, dtype):
    from mrag_amd.index import DenseIndex
    c, _ = sc.int_base(n, nq, d, amp, sc.SEED_A)
    ix = DenseIndex(d, metric="ip", dtype=dtype)
    ix.add(_store(c, dtype), normalize=False)
    return ix


@functools.lru_cache(maxsize=None)
def _dense_b_index(n, nq, d, spread, fp8=False):
    from mrag_amd.index import DenseIndex
    ix = DenseIndex(d, fp8_scan=fp8)
    ix.add(sc.family_b(n, nq, d, spread, 1)["c"], normalize=False)
    return ix


def _assert_exact(got_v, got_i, ref_v, ref_i, what=""):
    bad = np.flatnonzero((got_i != ref_i).any(1) | (got_v != ref_v).any(1))
    assert sc.accept_exact(got_v, got_i, ref_v, ref_i), \
        (what, f"{bad.size} queries differ, first {bad[:8]} (kinds {(bad[:8] % 5)})",
         got_i[bad[0]][:12], ref_i[bad[0]][:12], got_v[bad[0]][:12], ref_v[bad[0]][:12])


def _assert_tol(got_v, got_i, ref_v, ref_i):
    """tests/test_gpu_bruteforce.py::_check on given results"""
    valid = ref_i >= 0
    assert got_v.shape == ref_v.shape and got_i.dtype == np.int64
    assert ((got_i >= 0) == valid).all() and np.isneginf(got_v[~valid]).all()
    np.testing.assert_allclose(got_v[valid], ref_v[valid], rtol=0, atol=sc.TOL)
    with np.errstate(invalid="ignore"):                        # (-inf) - (-inf) among the empty slots
        assert (np.diff(got_v, axis=1)[valid[:, 1:]] <= 0).all()
    strict, bad = ds.gap_aware_id_match(got_i, got_v, ref_i, ref_v, tol=sc.TOL)
    assert bad == 0, (strict, bad)


# ------------------------------------------------------------------------------------------------ dense, plain search
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,k", DENSE_A)
def test_dense_family_a(name, k, dtype):
    _, nq, n, d, amp = sc.DENSE_BY_NAME[name][:5]
    a = sc.family_a(n, nq, d, amp, k)
    ix = _dense_a_index(n, nq, d, amp, dtype)
    v, i = ix.search(_store(a["q"], dtype), k, normalize=False)
    _assert_exact(v, i, a["rv"], a["ri"], name)


@pytest.mark.parametrize("name,k,spread", DENSE_B)
def test_dense_family_b(name, k, spread):
    _, nq, n, d = sc.DENSE_BY_NAME[name][:4]
    b = sc.family_b(n, nq, d, spread, k)
    v, i = _dense_b_index(n, nq, d, spread).search(b["q"], k, normalize=False)
    _assert_tol(v, i, b["rv"], b["ri"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", sc.WIDE[5])
def test_wide_batch_verifier_and_redo(k, dtype):
    """The wide batch: as generated, and with the rows stored by descending score of query 0, so that its whole top-k sits
    in the first split, where the k' = 64 lists of the batch kernel cannot hold it: the verifier must flag it."""
    from mrag_amd.index import DenseIndex
    _, nq, n, d, amp, _ = sc.WIDE
    a = sc.family_a(n, nq, d, amp, k)
    ix = _dense_a_index(n, nq, d, amp, dtype)
    v, i = ix.search(_store(a["q"], dtype), k, normalize=False)
    _assert_exact(v, i, a["rv"], a["ri"], "as generated")
    w = sc.wide_sorted(k)
    ix2 = DenseIndex(d, metric="ip", dtype=dtype)
    ix2.add(_store(w["c"], dtype), normalize=False)
    v, i = ix2.search(_store(w["q"], dtype), k, normalize=False)
    redone = ix2.last_wide_redone()
    ix2.close()
    _assert_exact(v, i, w["rv"], w["ri"], "sorted by query 0")
    assert redone >= 1


_K4W_CHILD = textwrap.dedent(r'''
    import sys
    sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
    import numpy as np
    import signed_scores_cases as sc
    from mrag_amd.index import DenseIndex
    for name in sc.K4W:
        _, nq, n, d, amp, ks, _ = sc.DENSE_BY_NAME[name]
        for dtype in ("f16", "bf16"):
            st = np.float16 if dtype == "f16" else np.float32
            for k in ks:
                a = sc.family_a(n, nq, d, amp, k)
                ix = DenseIndex(d, metric="ip", dtype=dtype)
                ix.add(a["c"].astype(st), normalize=False)
                v, i = ix.search(a["q"].astype(st), k, normalize=False)
                assert sc.accept_exact(v, i, a["rv"], a["ri"]), (name, dtype, k, "A")
                ix.close()
        for spread in sc.SPREADS_B:
            for k in ks:
                b = sc.family_b(n, nq, d, spread, k)
                ix = DenseIndex(d)
                ix.add(b["c"], normalize=False)
                v, i = ix.search(b["q"], k, normalize=False)
                assert sc.accept_tol(v, i, b["rv"], b["ri"]), (name, spread, k, "B")
                ix.close()
    print("ok")
''')


def test_k4w_for_every_query():
    """MRAG_K4S_CAP=0 (read once per process: a child) sends every query of the wide stream rows through the
    global-memory radix select K4w, as tests/test_gpu_backend.py::test_online_merge_fallback_path_matches does."""
    env = dict(os.environ, MRAG_K4S_CAP="0")
    r = subprocess.run([sys.executable, "-c", _K4W_CHILD, str(ROOT)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])


# ------------------------------------------------------------------------------------------------ dense, filtered
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", ["mask", "compact"])
@pytest.mark.parametrize("name,k", sc.FILTERED)
def test_dense_filtered_family_a(name, k, path, dtype):
    _, nq, n, d, amp = sc.DENSE_BY_NAME[name][:5]
    ix = _dense_a_index(n, nq, d, amp, dtype)
    for mname, mask in sc.allow_masks(n, k).items():
        a = sc.family_a_masked(n, nq, d, amp, k, mname)
        v, i = ix.search(_store(a["q"], dtype), k, normalize=False, allow=mask, filter_path=path)
        assert ix.last_filter() == {"path": path, "allowed": int(mask.sum())}
        _assert_exact(v, i, a["rv"], a["ri"], (name, mname))
        if mname == "few":
            assert (i[:, -1] == -1).all() and np.isneginf(v[:, -1]).all()      # the (-inf, -1) tail


@pytest.mark.parametrize("path", ["mask", "compact"])
@pytest.mark.parametrize("crossing", [0, 1])
@pytest.mark.parametrize("name,k", FILTERED_B)
def test_dense_filtered_family_b(name, k, crossing, path):
    _, nq, n, d = sc.DENSE_BY_NAME[name][:4]
    spread = sc.DENSE_BY_NAME[name][6][crossing]
    b = sc.family_b(n, nq, d, spread, k)
    ix = _dense_b_index(n, nq, d, spread)
    S = sc.S_of(b)
    for mname, mask in sc.allow_masks(n, k).items():
        rv, ri = sc.topk_of(np.where(mask[None, :], S, -np.inf), k)
        v, i = ix.search(b["q"], k, normalize=False, allow=mask, filter_path=path)
        assert ix.last_filter()["path"] == path
        _assert_tol(v, i, rv, ri)


# ------------------------------------------------------------------------------------------------ dense, range search
def _check_floors(search, S, top, k, what):
    """``top``: the problem's own top-k (rv, ri) at this k; the rows listed under a floor are its entries that reach it"""
    got = {}
    for floor in sc.FLOORS_A:
        got[repr(floor)] = g = search(floor)
        rv, ri, rc = sc.range_from_topk(S, top[0], top[1], floor)
        assert np.array_equal(g[2], rc), (what, floor, g[2][:10], rc[:10])
        _assert_exact(g[0], g[1], rv, ri, (what, floor))
    for x, y in zip(got["0.0"], got["-0.0"]):
        assert np.array_equal(x, y)
    zeros = (S == 0).sum(1)
    assert zeros.max() > 0 and (got["0.0"][2] == (S > 0).sum(1) + zeros).all()     # the rows at exactly 0.0 count
    assert (got["-1000.0"][2] == (S > -np.inf).sum(1)).all()
    assert S.shape[0] < 5 or (got["2.0"][2] == 0).any()        # (a batch of five or more holds an all-negative query)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,k", sc.FILTERED)
def test_dense_range_family_a(name, k, dtype):
    _, nq, n, d, amp = sc.DENSE_BY_NAME[name][:5]
    ix = _dense_a_index(n, nq, d, amp, dtype)
    a = sc.family_a(n, nq, d, amp, k)
    q = _store(a["q"], dtype)
    _check_floors(lambda f: ix.range_search(q, f, k, normalize=False), sc.S_of(a), (a["rv"], a["ri"]), k, name)
    m = sc.family_a_masked(n, nq, d, amp, k, "half")
    qm, mask = _store(m["q"], dtype), m["mask"]
    _check_floors(lambda f: ix.range_search(qm, f, k, normalize=False, allow=mask, filter_path="mask"), sc.S_of(m),
                  (m["rv"], m["ri"]), k, (name, "mask"))
    assert ix.last_filter()["path"] == "mask"


@pytest.mark.parametrize("name,k", FILTERED_B)
def test_dense_range_family_b(name, k):
    from test_gpu_range import _check_range
    _, nq, n, d = sc.DENSE_BY_NAME[name][:4]
    spread = sc.DENSE_BY_NAME[name][6][1]                       # the spread at which the row's lists cross zero
    b = sc.family_b(n, nq, d, spread, k)
    ix = _dense_b_index(n, nq, d, spread)
    S = sc.S_of(b)
    cnt = _check_range(*ix.range_search(b["q"], sc.FLOOR_B, k, normalize=False), S, sc.FLOOR_B, k)
    assert (cnt > 0).any()
    mask = sc.allow_masks(n, k)["half"]
    S = np.where(mask[None, :], S, -np.inf)
    _check_range(*ix.range_search(b["q"], sc.FLOOR_B, k, normalize=False, allow=mask, filter_path="mask"), S, sc.FLOOR_B, k)


# ------------------------------------------------------------------------------------------------ dense, fp8 scan
@pytest.mark.parametrize("spread", sc.SPREADS_B)
@pytest.mark.parametrize("nq,d", sc.FP8)
def test_dense_fp8_family_b(nq, d, spread):
    from test_gpu_fp8 import _sim_fp8_scores
    n, k = sc.FP8_N, sc.FP8_K
    b = sc.family_b(n, nq, d, spread, k)
    ix = _dense_b_index(n, nq, d, spread, fp8=True)
    _, ids = ix.search(b["q"], k, normalize=False, precision="fp8", refine=k)      # refine = k: the candidate set itself
    assert ix.last_fp8() == {"refine": k, "regime": "stream" if nq <= 16 else "batch"}
    assert ((ids >= 0) & (ids < n)).all() and all(len(set(r.tolist())) == k for r in ids)
    s8 = _sim_fp8_scores(b["q"], ix.rows_fp8())
    kth = np.sort(s8, axis=1)[:, -k]
    got = np.take_along_axis(s8, ids, axis=1)
    assert (got >= kth[:, None] - 1e-5 * np.abs(s8).max()).all(), float((kth[:, None] - got).max())
    v, ids = ix.search(b["q"], k, normalize=False, precision="fp8")                # default pool: exact scores of its rows
    assert ((ids >= 0) & (ids < n)).all() and all(len(set(r.tolist())) == k for r in ids)
    np.testing.assert_allclose(v, np.take_along_axis(sc.S_of(b), ids, axis=1), rtol=0, atol=sc.TOL)
    dv = np.diff(v, axis=1)
    assert (dv <= 0).all() and (np.diff(ids, axis=1)[dv == 0] > 0).all()


# ------------------------------------------------------------------------------------------------ dense, one set per question
@pytest.mark.parametrize("dtype", DTYPES)
def test_search_sets_family_a(dtype):
    p = sc.SETS
    sets, set_of, a = sc.sets_case()
    ix = _dense_a_index(p["n"], p["nq"], p["d"], p["amp"], dtype)
    v, i = ix.search_sets(_store(a["q"], dtype), p["k"], sets, set_of, normalize=False)
    assert ix.last_sets()["scanned"] == p["nq"]
    _assert_exact(v, i, a["rv"], a["ri"], "sets")


# ------------------------------------------------------------------------------------------------ IVF-flat
@functools.lru_cache(maxsize=None)
def _ivf_a_index(name, cl, dtype):
    from mrag_amd.index import IVFFlatIndex
    _, n, nq, d, amp, nlist, nprobe, ks, _, q_cols = sc.IVF_BY_NAME[name]
    a = sc.ivf_a(n, nq, d, amp, nlist, nprobe, ks[0], cl, q_cols=q_cols)
    ix = IVFFlatIndex(d, nlist, metric="ip", dtype=dtype)
    ix.set_centroids(_store(a["cen"], dtype), normalize=False)
    ix.add(_store(a["c"], dtype), normalize=False)
    assert np.array_equal(ix.assignments(), a["assign"])       # exact integer scores: the argmax, lowest list on ties
    return ix


def _ivf_case(name, k, cl):
    _, n, nq, d, amp, nlist, nprobe, _, _, q_cols = sc.IVF_BY_NAME[name]
    return sc.ivf_a(n, nq, d, amp, nlist, nprobe, k, cl, q_cols=q_cols), nprobe


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cl", [0, 1])
@pytest.mark.parametrize("name,k", [(r[0], k) for r in sc.IVF for k in r[7]])
def test_ivf_family_a(name, k, cl, dtype):
    a, nprobe = _ivf_case(name, k, cl)
    ix = _ivf_a_index(name, cl, dtype)
    v, i = ix.search(_store(a["q"], dtype), k, nprobe, normalize=False)
    _assert_exact(v, i, a["rv"], a["ri"], (name, cl))
    assert ix.last_timing()["scanned_rows"] > 0


@functools.lru_cache(maxsize=None)
def _ivf_b_index(spread, fp8=False):
    from mrag_amd.index import IVFFlatIndex
    _, n, nq, d, _, nlist, nprobe = sc.IVF_BY_NAME["register"][:7]
    b = sc.ivf_b(n, nq, d, nlist, nprobe, spread)
    ix = IVFFlatIndex(d, nlist, fp8_scan=fp8)
    ix.set_centroids(b["cen"], normalize=False)
    ix.add(b["c"], normalize=False)
    return ix, b, nprobe


@pytest.mark.parametrize("spread", sc.SPREADS_B)
@pytest.mark.parametrize("k", sc.IVF_BY_NAME["register"][7])
def test_ivf_family_b_register_path(k, spread):
    ix, b, nprobe = _ivf_b_index(spread)
    assert b["n_clear"] == b["q"].shape[0] == sc.IVF_BY_NAME["register"][2]
    v, i = ix.search(b["q"], k, nprobe, normalize=False)
    rv, ri = ds.ivf_search(b["q"], b["c"], b["cen"], ix.assignments().astype(np.int64), nprobe, k)
    assert (rv < 0).all() if spread == 0.1 else (rv[:, 0].max() > 0 > rv[:, -1].min())
    _assert_tol(v, i, rv, ri)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("frac", sc.IVF_FILTER_FRACS)
def test_ivf_filtered_family_a(frac, dtype):
    k, nprobe = sc.IVF_FILTER_K, sc.IVF_BY_NAME["register"][6]
    case = sc.ivf_a_filtered(frac)
    mask = case["mask"]
    ix = _ivf_a_index("register", 1, dtype)
    for path in ("probe", "exact"):
        q, rv, ri = case[path]
        v, i = ix.search(_store(q, dtype), k, nprobe, normalize=False, allow=mask, filter_path=path)
        f = ix.last_filter()
        assert f["path"] == path and f["allowed"] == int(mask.sum())
        _assert_exact(v, i, rv, ri, (frac, path))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cl", [0, 1])
def test_ivf_range_family_a(cl, dtype):
    k = 10
    a, nprobe = _ivf_case("register", k, cl)
    ix = _ivf_a_index("register", cl, dtype)
    best = a["ri"][:, 0].copy()
    S = a["S"].copy()
    S[np.arange(S.shape[0]), best] = -np.inf                   # the excluded row is neither listed nor counted
    q = _store(a["q"], dtype)
    top = sc.topk_of(S, k)
    _check_floors(lambda f: ix.range_search(q, f, k, nprobe, normalize=False, exclude=best), S, top, k, ("ivf", cl))


@pytest.mark.parametrize("spread", sc.SPREADS_B)
def test_ivf_fp8_family_b(spread):
    from test_gpu_ivf_fp8 import _sim_fp8_scores
    k = 10
    ix, b, nprobe = _ivf_b_index(spread, fp8=True)
    n = b["c"].shape[0]
    _, ids = ix.search(b["q"], k, nprobe, normalize=False, precision="fp8", refine=k)
    assert ix.last_fp8() == {"refine": k}
    assert ((ids >= 0) & (ids < n)).all() and all(len(set(r.tolist())) == k for r in ids)
    inside = sc.probed_mask(sc.probes_of(b["q"], b["cen"], nprobe), ix.assignments().astype(np.int64))
    assert np.take_along_axis(inside, ids, axis=1).all()                           # rows of the probed lists only
    full = _sim_fp8_scores(b["q"], ix.rows_fp8())
    s8 = np.where(inside, full, -np.inf)
    kth = np.sort(s8, axis=1)[:, -k]
    got = np.take_along_axis(s8, ids, axis=1)
    assert (got >= kth[:, None] - 1e-5 * np.abs(full).max()).all(), float((kth[:, None] - got).max())
    v, ids = ix.search(b["q"], k, nprobe, normalize=False, precision="fp8")
    S = sc.scores64(b["q"], b["c"])
    assert np.take_along_axis(inside, ids, axis=1).all() and all(len(set(r.tolist())) == k for r in ids)
    np.testing.assert_allclose(v, np.take_along_axis(S, ids, axis=1), rtol=0, atol=sc.TOL)
    dv = np.diff(v, axis=1)
    assert (dv <= 0).all() and (np.diff(ids, axis=1)[dv == 0] > 0).all()


_FUSED_CHILD = textwrap.dedent(r'''
    import sys
    sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
    import numpy as np
    import signed_scores_cases as sc
    from mrag_amd.index import IVFFlatIndex
    _, n, nq, d, amp, nlist, nprobe = sc.IVF_BY_NAME["register"][:7]
    out = {}
    for k in sc.IVF_FUSED_KS:
        for dtype in ("f16", "bf16"):
            st = np.float16 if dtype == "f16" else np.float32
            a = sc.ivf_a(n, nq, d, amp, nlist, nprobe, k, 1)
            ix = IVFFlatIndex(d, nlist, metric="ip", dtype=dtype)
            ix.set_centroids(a["cen"].astype(st), normalize=False)
            ix.add(a["c"].astype(st), normalize=False)
            out[f"a_{k}_{dtype}_v"], out[f"a_{k}_{dtype}_i"] = ix.search(a["q"].astype(st), k, nprobe, normalize=False)
            ix.close()
        b = sc.ivf_b(n, nq, d, nlist, nprobe, 0.1)
        ix = IVFFlatIndex(d, nlist)
        ix.set_centroids(b["cen"], normalize=False)
        ix.add(b["c"], normalize=False)
        out[f"b_{k}_v"], out[f"b_{k}_i"] = ix.search(b["q"], k, nprobe, normalize=False)
        out["b_assign"] = ix.assignments()
        ix.close()
    np.savez(sys.argv[2], **out)
''')


def test_ivf_fused_regime_bit_for_bit():
    """MRAG_IVF_SCORES_MB=0 (read once per process: a child) runs the list scan as K2's descriptor instance, with its own
    bootstrap for k < 16; its answers are the default regime's bit for bit, and the default regime's are the oracle's."""
    _, n, nq, d, amp, nlist, nprobe = sc.IVF_BY_NAME["register"][:7]
    with tempfile.TemporaryDirectory() as td:
        res = {}
        for regime, env in (("segments", {}), ("fused", {"MRAG_IVF_SCORES_MB": "0"})):
            path = os.path.join(td, regime + ".npz")
            r = subprocess.run([sys.executable, "-c", _FUSED_CHILD, str(ROOT), path], env={**os.environ, **env},
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, (regime, r.stdout[-500:], r.stderr[-1500:])
            res[regime] = dict(np.load(path))
    seg, fus = res["segments"], res["fused"]
    assert set(seg) == set(fus)
    for key in seg:
        same = np.array_equal(seg[key].view(np.uint32), fus[key].view(np.uint32)) if key.endswith("_v") else np.array_equal(seg[key], fus[key])
        assert same, key
    for k in sc.IVF_FUSED_KS:
        a = sc.ivf_a(n, nq, d, amp, nlist, nprobe, k, 1)
        for dtype in DTYPES:
            _assert_exact(fus[f"a_{k}_{dtype}_v"], fus[f"a_{k}_{dtype}_i"], a["rv"], a["ri"], ("fused", k, dtype))
        b = sc.ivf_b(n, nq, d, nlist, nprobe, 0.1)
        rv, ri = ds.ivf_search(b["q"], b["c"], b["cen"], fus["b_assign"].astype(np.int64), nprobe, k)
        _assert_tol(fus[f"b_{k}_v"], fus[f"b_{k}_i"], rv, ri)
