"""What the encoder's GPU parity tests can see, established on the CPU with the oracle alone (no kernel runs here).

For every case of ``oracle/encoder_cases.py``: the rounding noise of a 16-bit pipeline (``forward_rounded`` against the fp64
oracle), the tolerance the GPU test uses (``TOL_FACTOR x noise``), and the effect of each structural mutant of the forward
pass.  A GPU case compares four quantities -- mean and CLS pooling, normalised and not -- each at its own tolerance; a mutant
counts as seen when it moves at least one of them by ``MUTANT_MARGIN x`` that quantity's tolerance.  These are conditions on
the inputs (lengths, masks, query / key gain), not measurements of the code under test.  Run with ``-s`` for the table.
"""
import numpy as np
import pytest

from oracle import encoder as oe
from oracle import encoder_cases as ec


def _tag(q):
    return f"{q[0]}{'' if q[1] else '-raw'}"


@pytest.mark.parametrize("case", ec.CASES, ids=lambda c: c.name)
def test_case_discriminates(case):
    spec, w = case.spec, case.weights()
    ids, mask = case.oracle_batch()
    probs = []
    x = ec._run(spec, w, ids, mask, probs=probs)
    base = ec.quantities(x, mask)
    # the private copy is the oracle: all four compared quantities, to the last bits
    for pool, norm in ec.QUANTITIES:
        ref = oe.forward(spec, w, ids, mask, pool=pool, normalize=norm)
        assert np.abs(ref - base[(pool, norm)]).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    print(f"\n{case.name} [{case.note}]  B x S = {mask.shape[0]} x {mask.shape[1]}  mean max probability per layer: "
          + " ".join(f"{p:.2f}" for p in probs))
    assert all(ec.PROB_BAND[0] <= p <= ec.PROB_BAND[1] for p in probs), probs

    effects = {}
    for m in ec.MUTANTS + ec.REPORTED_MUTANTS:
        xm = ec._run(spec, w, ids, mask, mut=m)
        if xm is None:                      # the mutant changes nothing on this batch (no masked key, S below the boundary, ...)
            continue
        eff = {q: float(np.abs(ec.pooled(xm, mask, *q, mut=m) - base[q]).max()) for q in ec.QUANTITIES}
        if m == "pool_div_S" and max(eff.values()) == 0.0:      # no padded row
            continue
        effects[m] = eff
    applicable = set(effects) & set(ec.MUTANTS)
    assert {"drop_last_valid", "pos_shift", "swap_v_heads"} <= applicable
    if (mask == 0).any():
        assert {"attend_first_masked", "pool_div_S"} <= applicable
    failures = []
    for dtype in case.dtypes:
        ex = ec.case_expected(case.name, dtype)
        print(f"  {dtype}: " + "  ".join(f"{_tag(q)} noise {ex.noise[q]:.2e} tol {ex.tol[q]:.2e}" for q in ec.QUANTITIES))
        for q in ec.QUANTITIES:
            assert ex.noise[q] > 0.0
        for m, eff in effects.items():
            q = max(ec.QUANTITIES, key=lambda q: eff[q] / ex.tol[q])
            ratio = eff[q] / ex.tol[q]
            asserted = m in ec.MUTANTS or (m == "scale_dh_plus_1" and (case.name, dtype) in ec.SCALE_MUTANT_ASSERTED)
            print(f"    {m:20s} effect / tol {ratio:8.2f}  (effect / noise {ratio * ec.TOL_FACTOR:8.1f}, on {_tag(q)})"
                  + ("" if asserted else "   reported only"))
            if asserted and ratio < ec.MUTANT_MARGIN:
                failures.append((dtype, m, ratio))
            elif m == "scale_dh_plus_1" and not asserted:
                # the asserted list is complete: a pair that reaches the margin belongs on it
                assert ratio < ec.MUTANT_MARGIN, (case.name, dtype, ratio, "add to SCALE_MUTANT_ASSERTED")
    assert not failures, failures


def test_attention_cases_cover_every_dispatch_cell():
    """Every (head dim, key padding or general kernel) pair of ``launch_attention`` has a case on each side of its boundaries,
    and each runs in both dtypes."""
    cells = {(c.geometry, c.note) for c in ec.ATTENTION_CASES}
    assert len(cells) == 8 and all(c.dtypes == ("f16", "bf16") for c in ec.ATTENTION_CASES)
    assert {c.S for c in ec.ATTENTION_CASES} == {16, 64, 65, 128, 129, 256, 257, 300, 511, 512}
    for c in ec.ATTENTION_CASES:
        _, mask = c.batch()
        n = (mask != 0).sum(1)
        assert {1, 2, c.S - 1, c.S} <= set(n.tolist())
        if c.S > 256:                       # the general kernel's first two key blocks fully masked in one row
            assert any(m[:128].max() == 0 and m.any() for m in mask)
        assert ((mask != 0) & (mask != 1)).any()


def test_mask_generators():
    rng = np.random.default_rng(0)
    assert ec.mask_row("trailing", 8, 3).tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
    assert ec.mask_row("left", 8, 3).tolist() == [0, 0, 0, 0, 0, 1, 1, 1]
    assert ec.mask_row("pair", 70, 64).nonzero()[0].tolist() == [0, 64]
    assert not ec.mask_row("empty", 8).any()
    h = ec.mask_row("holes", 200, 0, rng)
    assert h[0] and h[-1] and 60 < h.sum() < 180
    v = ec.mask_row("values", 50, 20, rng)
    assert (v[:20] != 0).all() and not v[20:].any() and (v[:20] != 1).any()


def test_rounding_model_rounds():
    """bf16 rounding goes through torch.bfloat16; fp16 through numpy: both idempotent, bf16 the coarser."""
    a = np.random.default_rng(1).standard_normal(1000)
    for dt in ("f16", "bf16"):
        r = ec._rounder(dt)(a)
        assert np.array_equal(ec._rounder(dt)(r), r) and 0 < np.abs(r - a).max()
    assert np.abs(ec._rounder("bf16")(a) - a).max() > 4 * np.abs(ec._rounder("f16")(a) - a).max()
