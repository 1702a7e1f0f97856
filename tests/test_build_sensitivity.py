"""What the build path's GPU tests can see, established on the CPU with the oracle alone (no kernel runs here).

For every case of ``oracle/build_cases.py`` that ``tests/test_gpu_build_paths.py`` runs on the device: the comparison the
GPU test makes accepts the oracle recomputed in the device's own summation order (the only legitimate difference), and
each mutant the case targets breaks that comparison -- bit cases by a changed bit, share and training cases by more than
1 ulp somewhere or ``MUTANT_FACTOR`` x the allowed share.  Conditions on the inputs, not measurements of the code under
test.  Run with ``-s`` for the tables (the shares DESIGN.md quotes come from them).
"""
import numpy as np
import pytest

from oracle import build_cases as bc


@pytest.mark.parametrize("case", bc.PREP_CASES, ids=lambda c: c.name)
def test_prep_case_discriminates(case):
    x = case.source()
    want = case.expected()
    assert want.dtype == np.uint16 and want.shape == x.shape
    vals = bc.bits_to_f64(want, case.storage)
    assert np.isfinite(vals).all() and np.abs(vals).max() <= 65504          # no NaN, no infinity, nothing above fp16's range
    if case.normalize:
        # the device's order of the fp64 partial sums, both kernels (a misaligned source sends any shape to the scalar one)
        kernels = {bc.prep_kernel(case.src, x.shape[1]), "scalar"}
        for kern in sorted(kernels):
            lane = bc.prep_reference(x, case.storage, True, ss=bc.lane_order_ss(x, kern))
            share, worst = bc.share_and_max(lane, want)
            print(f"\n{case.name}: {kern} lane order: share {share:.2e}, worst {worst} ulp")
            if case.mode == "share":
                assert bc.within_bar(lane, want)
            else:
                assert np.array_equal(lane, want)
    missed = []
    for m in bc.PREP_MUTANTS:
        got = bc.prep_reference(x, case.storage, case.normalize, mutant=m)
        share, worst = bc.share_and_max(got, want)
        seen = bc.exceeds_bar(got, want) if case.mode == "share" else not np.array_equal(got, want)
        print(f"  {m:18s} share {share:.2e}  worst {worst:6d} ulp  {'seen' if seen else 'not seen'}"
              + ("" if m in case.targets else "   (not a target)"))
        if m in case.targets and not seen:
            missed.append((m, share, worst))
    assert not missed, missed


def test_every_prep_mutant_is_a_target_somewhere():
    for m in bc.PREP_MUTANTS:
        assert any(m in c.targets for c in bc.PREP_CASES), m
    # the cases the issue lists: every source x storage x normalize, both kernels around the 4096 boundary, the share shape
    assert {(c.src, c.storage, c.normalize) for c in bc.PREP_CASES if c.name.startswith("types-")} == \
        {(s, t, nm) for s in bc.SOURCES for t in bc.STORAGES for nm in (True, False)}
    assert {bc.prep_kernel("f32", d) for d in (8, 64, 384, 4096)} == {"vec"}
    assert {bc.prep_kernel("f32", d) for d in (100, 4104, 8192)} == {"scalar"}
    assert all(c.values().shape == (3001, 384) for c in bc.PREP_CASES if c.mode == "share")


def test_rounding_helpers():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(4000) * np.exp(rng.uniform(-12, 8, 4000))
    for st in bc.STORAGES:
        b = bc.round_bits(x.astype(np.float32), st)
        v = bc.bits_to_f64(b, st)
        assert np.array_equal(bc.values_to_bits(v.astype(np.float32), st), b)
        assert np.array_equal(bc.round_bits(v.astype(np.float32), st), b)             # idempotent
        # the one-step grid rounding agrees with the format's own rounding on fp32 inputs
        assert np.array_equal(bc._round_fmt(x.astype(np.float32).astype(np.float64), st), v)
        t = bc._round_fmt(x, st, np.trunc)
        assert (np.abs(t) <= np.abs(x)).all() and (np.abs(bc.ulp_diff(bc.round_bits(t.astype(np.float32), st), b)) <= 1).all()
        # halfway points go to the even neighbour; double rounding differs from direct rounding on exactly half of the set
        h = bc.gen_halfway(st)
        hb = bc.prep_reference(h, st, False)
        assert ((hb[h != 0] & 1) == 0).all()
        d = bc.gen_double_rounding(st)
        two, one = bc.prep_reference(d, st, False), bc.prep_reference(d, st, False, mutant="no_f32_step")
        assert (two != one)[d != 0].mean() == 0.5
    sub = bc.prep_reference(bc.gen_subnormals(), "f16", False)
    assert ((sub & 0x7C00) == 0).sum() > 100 and ((sub & 0x7FFF) != 0).sum() > 100


def test_train_picks_is_the_librarys_choice():
    """Pinned values (computed from the definition: splitmix64, Floyd's sampling, ascending) and the properties."""
    for seed, n, nlist in ((0, 10, 10), (5, 1000, 8), (12, 777, 300), (2 ** 63 + 9, 50, 7)):
        p = bc.train_picks(seed, n, nlist)
        assert len(p) == nlist and (np.diff(p) > 0).all() and p[0] >= 0 and p[-1] < n
    assert bc.train_picks(0, 10, 10).tolist() == list(range(10))
    # splitmix64's published first outputs for seed 0
    s, z0 = bc._splitmix64(0)
    s, z1 = bc._splitmix64(s)
    assert (z0, z1) == (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4)
    # Floyd by hand: n = 4, nlist = 2 -> j = 2 draws z0 % 3, j = 3 draws z1 % 4 (a repeat takes j itself)
    t0 = z0 % 3
    t1 = z1 % 4
    assert bc.train_picks(0, 4, 2).tolist() == sorted({t0, 3 if t1 == t0 else t1})


@pytest.mark.parametrize("case", bc.TRAIN_CASES, ids=lambda c: c.name)
def test_train_case_discriminates(case):
    exp = bc.train_expected(case)
    bits, picks = exp["rows"], exp["picks"]
    vals = bc.bits_to_f64(bits, case.storage)
    assert np.isfinite(vals).all()
    if case.iters == 0:
        assert np.array_equal(exp["centroids"], bits[picks])
        # a wrong choice of rows shows: the rows at the picked positions are pairwise distinct and differ from their neighbours
        other = bits[np.minimum(picks + 1, case.n - 1)] if case.n > case.nlist else bits[picks][::-1]
        assert not np.array_equal(other, bits[picks])
        assert len(np.unique(bits[picks], axis=0)) == case.nlist
        return
    size = exp["centroids"].size
    print(f"\n{case.name}: min margin {exp['min_margin']:.3e}; emulated fp32 orders move at most {exp['emu_diff']} of {size} "
          f"elements (share {exp['emu_diff'] / size:.2e}, {exp['emu_ulp']} ulp); allowed {exp['allowed_diff']}")
    if case.kind != "ints":
        assert exp["min_margin"] >= 1e-4                                    # no assignment hangs on a rounding
    assert exp["emu_ulp"] <= 1
    ok, _, _ = bc.train_matches(exp["centroids"], exp)
    assert ok
    if case.kind == "ints":
        assert exp["emu_diff"] == 0                                         # every fp32 sum is exact: order-independent
        assert (exp["counts"] > 0).all()
    if case.kind == "empty":
        lo, hi = bc.EMPTY_LISTS
        assert np.array_equal(bits[picks[lo]], bits[picks[hi]])
        assert exp["counts"][hi] == 0 and exp["counts"][lo] > 2
        assert np.array_equal(exp["centroids"][hi], exp["start"][hi])
        assert np.array_equal(exp["centroids"][lo], exp["start"][lo])       # many copies of one point: the list stays where it is
        assert exp["centroids"][hi].any()
    missed = []
    for m in case.mutants:
        got = bc.train_mutant(case, m)
        d = np.abs(bc.ulp_diff(got, exp["centroids"]))
        ndiff, worst = int((d != 0).sum()), int(d.max())
        seen = worst > 1 or ndiff >= bc.MUTANT_FACTOR * exp["allowed_diff"]
        print(f"  {m:12s} moves {ndiff:6d} elements, worst {worst:6d} ulp  {'seen' if seen else 'not seen'}")
        if not seen:
            missed.append((m, ndiff, worst))
    assert not missed, missed


def test_every_train_mutant_is_a_target_somewhere():
    for m in bc.TRAIN_MUTANTS:
        assert any(m in c.mutants for c in bc.TRAIN_CASES), m
    grid = {(c.metric, c.storage, c.dim, c.n, c.iters) for c in bc.TRAIN_CASES if c.kind == "clusters" and c.iters}
    assert grid == {(m, s, d, n, i) for m in ("cosine", "ip") for s in bc.STORAGES for d in (64, 100) for n in (2003, 4999)
                    for i in (1, 3)}
