"""GPU parity of the index build path: row preparation (K1, csrc/common.hip) and IVF training (mrag_ivf_train), against
the fp64 oracle of ``oracle/build_cases.py``.  The cases, their expected bits and the tolerance of each comparison live
there; ``tests/test_build_sensitivity.py`` shows on the CPU what these comparisons tell apart.  The reference ships no
index: PARITY UNPINNED by the reference."""
import numpy as np
import pytest

from oracle import build_cases as bc
from oracle import dense_search as ds

pytestmark = pytest.mark.gpu


def _compare(case, got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint16
    share, worst = bc.share_and_max(got, want)
    print(f"\n{case.name} [{what}]: share of differing elements {share:.3e}, worst {worst} ulp")
    if case.mode == "share":
        assert bc.within_bar(got, want), (what, share, worst)
    else:
        assert np.array_equal(got, want), (what, share, worst, np.argwhere(got != want)[:5].tolist())


# ---------------------------------------------------------------------------------------------- row preparation
@pytest.mark.parametrize("case", bc.PREP_CASES, ids=lambda c: c.name)
def test_prep_matches_oracle(case):
    from mrag_amd.index import DenseIndex, IVFFlatIndex
    x, want = case.source(), case.expected()
    n, dim = want.shape
    ix = DenseIndex(dim, dtype=case.storage)
    ix.add(x, normalize=case.normalize)
    assert len(ix) == n
    got = ix.stored_bits()
    assert np.array_equal(bc.values_to_bits(ix.rows(), case.storage), got)
    _compare(case, got, want, "dense")
    if not case.normalize and case.src == case.storage:
        src_bits = x.view(np.uint16) if case.src == "f16" else x.view(bc._torch().int16).numpy().view(np.uint16)
        assert np.array_equal(got, src_bits)                                # stored verbatim
    ix.close()
    if case.ivf:
        iv = IVFFlatIndex(dim, n, dtype=case.storage)
        iv.set_centroids(x, normalize=True)
        _compare(case, bc.values_to_bits(iv.centroids(), case.storage), want, "ivf centroids")
        iv.close()


@pytest.mark.parametrize("storage", bc.STORAGES)
def test_misaligned_device_source_gives_the_same_bits(storage):
    """A device fp32 source that is 4-byte but not 16-byte aligned cannot take 16-byte loads: same bits as the aligned copy."""
    import torch
    from mrag_amd.index import DenseIndex
    n, dim = 301, 384
    vals = torch.from_numpy(bc.gen_gauss(n, dim, 8).astype(np.float32))
    flat = torch.empty(n * dim + 1, dtype=torch.float32, device="cuda")
    flat[1:] = vals.reshape(-1).cuda()
    view = flat[1:].view(n, dim)
    aligned = vals.cuda()
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and aligned.data_ptr() % 16 == 0
    out = []
    for src in (view, aligned):
        for normalize in (True, False):
            ix = DenseIndex(dim, dtype=storage)
            ix.add(src, normalize=normalize)
            torch.cuda.synchronize()
            out.append(ix.stored_bits())
            ix.close()
    assert np.array_equal(out[0], out[2]) and np.array_equal(out[1], out[3])
    assert np.array_equal(out[2], bc.prep_reference(vals.numpy(), storage, True))
    assert np.array_equal(out[3], bc.prep_reference(vals.numpy(), storage, False))


@pytest.mark.parametrize("storage", bc.STORAGES)
def test_pad_columns_are_zero(storage):
    """dim 100 in rows of 128: scores of device-prepared rows against device-prepared queries equal the oracle's over
    the 100 columns (a non-zero pad column would add to them), and the fp8 copy follows the stored rows bit for bit."""
    import torch
    from mrag_amd.index import DenseIndex
    n, nq, dim, k = 257, 33, 100, 10
    x, q = bc.gen_gauss(n, dim, 41).astype(np.float32), bc.gen_gauss(nq, dim, 42).astype(np.float32)
    ix = DenseIndex(dim, dtype=storage, fp8_scan=True)
    ix.add(x[:130])
    ix.add(x[130:])                                                          # the second add starts mid-tile
    want = bc.prep_reference(x, storage, True)
    assert np.array_equal(ix.stored_bits(), want)
    sc, ids = ix.search(q, k)
    c64, q64 = bc.bits_to_f64(want, storage), bc.bits_to_f64(bc.prep_reference(q, storage, True), storage)
    rv, ri = ds.brute_force_topk(q64, c64, k)
    np.testing.assert_allclose(sc, rv, rtol=0, atol=1e-5)
    assert ds.gap_aware_id_match(ids, sc, ri, rv, tol=1e-5)[1] == 0
    # tests/test_gpu_fp8.py's rule: torch's e4m3fn (nearest even) of clip(256 x, +-448)
    scaled = np.clip(ix.rows() * np.float32(256.0), -448.0, 448.0)
    ref8 = torch.from_numpy(scaled).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(ix.rows_fp8(), ref8)


# ---------------------------------------------------------------------------------------------- IVF training
@pytest.mark.parametrize("case", bc.TRAIN_CASES, ids=lambda c: c.name)
def test_train_matches_oracle(case):
    from mrag_amd.index import IVFFlatIndex
    exp = bc.train_expected(case)
    rows = exp["rows"]
    if case.iters and case.kind != "ints":
        assert exp["min_margin"] >= 1e-4                                    # a condition on the input, not on the device
    ix = IVFFlatIndex(case.dim, case.nlist, metric=case.metric, dtype=case.storage)
    ix.train(bc.bits_to_source(rows, case.storage), iters=case.iters, seed=case.seed, normalize=False)
    got = bc.values_to_bits(ix.centroids(), case.storage)
    if case.iters == 0:
        assert np.array_equal(got, rows[exp["picks"]])                       # the picked rows, ascending, bit for bit
    else:
        ok, ndiff, worst = bc.train_matches(got, exp)
        print(f"\n{case.name}: {ndiff} of {got.size} elements differ (share {ndiff / got.size:.2e}, worst {worst} ulp); "
              f"emulated {exp['emu_diff']}, allowed {exp['allowed_diff']}")
        assert ok, (ndiff, worst, exp["allowed_diff"])
        if case.kind == "ints":
            assert exp["emu_diff"] == 0 and np.array_equal(got, exp["centroids"])   # exact fp32 sums: no order to differ in
        if case.kind == "empty":
            hi = bc.EMPTY_LISTS[1]
            assert exp["counts"][hi] == 0 and np.array_equal(got[hi], exp["start"][hi])
    # the add path assigns against the device's own final centroids
    ix.add(bc.bits_to_source(rows, case.storage), normalize=False)
    a_ref, margin = bc._assign(bc.bits_to_f64(rows, case.storage), got, case.storage)
    clear = margin >= 1e-5
    assert (ix.assignments()[clear] == a_ref[clear]).all() and clear.mean() > 0.5
    ix.close()
