"""Handles free what they hold: build, use and destroy one handle of every kind, over and over.

One cycle builds a dense index (fp8 copy, a filtered search with a host allow-set, search_groups, search_collapsed,
expand_neighbors), an IVF-flat index over the same rows (2 iterations of training; search, filtered search with a host
allow-set and a host list_allowed on both paths, range search with host exclude_rows, self-join, fp8 search, its fp8 rows
read to the host), a BM25 index and the smallest encoder the encoder tests use, and closes them all.  Rows are added in two
halves, with the fp8 copies switched on in between: the growth paths, which keep the stored contents, run in every cycle.

After one warm-up cycle five cycles run.
(a) Every result of cycles 2 to 5 equals cycle 1's bit for bit.
(b) The device's free memory after the five cycles lies at most 12.8 MB below its value after the warm-up: half of
    n * ld * 2 = 25.6 MB, the stored rows of ONE dense handle, so one handle in five that kept only its rows fails.

k-means sums the rows of a list with float atomics, whose order is not defined: two trainings from the same seed may differ
in the last bit of a few centroid elements (tests/test_gpu_ivf.py: "reproducible up to float-atomic order").  Every cycle
trains, so that training's buffers live and die in it, and then sets the centroids the warm-up cycle trained: the searches
compared in (a) run over the same lists in every cycle.
"""
import numpy as np
import pytest

N_ROWS, DIM, NLIST, NQ, K = 100_000, 128, 16, 64, 10
BOUND_BYTES = N_ROWS * DIM * 2 // 2


def _inputs():
    from oracle import dense_search as ods
    rows = ods.normalize_round(ods.make_gaussian(N_ROWS, DIM, 1234))
    q = ods.normalize_round(ods.make_gaussian(NQ, DIM, 5678))
    rng = np.random.default_rng(7)
    allow = rng.random(N_ROWS) < 0.3                     # host allow-set (bool mask)
    keys = (np.arange(N_ROWS) // 5).astype(np.int32)     # documents of five consecutive rows
    docs = [{"text": " ".join(f"w{(7 * d + j) % 97}" for j in range(3 + d % 5))} for d in range(300)]
    ids = rng.integers(0, 1000, size=(4, 16)).astype(np.int32)
    return dict(rows=rows, q=q, allow=allow, keys=keys, docs=docs, ids=ids, mask=np.ones_like(ids))


def _dense(x):
    from mrag_amd.index import DenseIndex
    half = N_ROWS // 2
    ix = DenseIndex(DIM, device=0)
    ix.add(x["rows"][:half], normalize=False)
    ix.enable_fp8()                                      # built from the stored rows ...
    ix.add(x["rows"][half:], normalize=False)            # ... and grown with them
    out = list(ix.search(x["q"], K, normalize=False))
    out += ix.search(x["q"], K, normalize=False, precision="fp8")
    out += ix.search(x["q"], K, normalize=False, allow=x["allow"])
    out += ix.search_groups(x["q"], K, sizes=[4] * (NQ // 4), normalize=False)
    ix.set_row_keys(x["keys"])
    out += ix.search_collapsed(x["q"], K, normalize=False)
    out += ix.expand_neighbors(out[1][:, :4], window=2)
    out.append(ix.rows_fp8(half - 8, 16))
    ix.close()
    return out


def _ivf(x, centroids):
    """-> (results, the centroids this cycle trained)"""
    from mrag_amd.index import IVFFlatIndex
    half = N_ROWS // 2
    ix = IVFFlatIndex(DIM, NLIST, device=0)
    ix.train(x["rows"], iters=2, seed=3, normalize=False)
    trained = ix.centroids()
    ix.set_centroids(trained if centroids is None else centroids, normalize=False)
    ix.add(x["rows"][:half], normalize=False)
    out = list(ix.search(x["q"], K, 4, normalize=False))
    ix.enable_fp8()                                      # next to the regrouped rows ...
    ix.add(x["rows"][half:], normalize=False)            # ... and rebuilt with the next regroup
    out += ix.search(x["q"], K, 4, normalize=False)
    per_list = ix.allowed_per_list(x["allow"])
    out.append(per_list)
    out += ix.search(x["q"], K, 4, normalize=False, allow=x["allow"], filter_path="probe", list_allowed=per_list)
    out += ix.search(x["q"], K, 4, normalize=False, allow=x["allow"], filter_path="exact")
    out += ix.range_search(x["q"], 0.2, 16, 4, normalize=False, exclude=np.arange(NQ, dtype=np.int64))
    out += [t.cpu().numpy() for t in ix.self_join(0.3, 2, k=8, batch=16384)]
    out += ix.search(x["q"], K, 4, normalize=False, precision="fp8")
    out.append(ix.rows_fp8(half - 8, 16))
    ix.close()
    return out, trained


def _bm25(x):
    from mrag_amd.text_index import HipBM25Index
    ix = HipBM25Index(rows=x["docs"])
    hits = ix.search(["w3 w10", "w96"], top_k=5)
    ix.close()
    return [np.array([d for d, _ in hits], dtype=np.int64), np.array([s for _, s in hits], dtype=np.float64)]


def _encoder(x):
    from mrag_amd.encoder import HipSentenceEncoder
    enc = HipSentenceEncoder.from_seed("tiny", seed=3)
    out = enc.forward(x["ids"], x["mask"])
    enc.close()
    return [out]


def _cycle(x, centroids):
    ivf, trained = _ivf(x, centroids)
    return _dense(x) + ivf + _bm25(x) + _encoder(x), trained


@pytest.mark.gpu
def test_handles_free_what_they_hold():
    import torch
    x = _inputs()
    _, centroids = _cycle(x, None)                        # warm-up: the allocator's pools, the kernels' code objects
    torch.cuda.synchronize()
    free_before = torch.cuda.mem_get_info(0)[0]
    runs = [_cycle(x, centroids)[0] for _ in range(5)]
    torch.cuda.synchronize()
    free_after = torch.cuda.mem_get_info(0)[0]
    print(f"free memory: {free_before} B after the warm-up, {free_after} B after five cycles, "
          f"drop {free_before - free_after} B (bound {BOUND_BYTES} B)")
    first = [np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in runs[0]]
    assert len(first) >= 30 and all(a.size for a in first)
    for c, run in enumerate(runs[1:], start=2):
        for i, (a, b) in enumerate(zip(first, run)):
            b = np.asarray(b.cpu() if hasattr(b, "cpu") else b)
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"cycle {c}, result {i}"
    assert free_before - free_after <= BOUND_BYTES, (free_before, free_after)
