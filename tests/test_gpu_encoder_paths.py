"""GPU parity of the HIP sentence encoder over its whole dispatch (csrc/encoder.hip ``forward`` and the launchers of
csrc/enc_*.hip): every attention instance in both dtypes, the mask families, the three GEMM kernels and both LayerNorm
flows, against the fp64 oracle.

Inputs, tolerances and the reasons for both come from ``oracle/encoder_cases.py``: query / key weights scaled until attention
is neither uniform nor saturated, and a tolerance of 4 x the rounding noise of a 16-bit pipeline, computed from the oracle
for each case and dtype.  ``tests/test_encoder_sensitivity.py`` shows on the CPU that at these tolerances a dropped key, an
attended padding key, a wrong pooling divisor, shifted positions or swapped heads fail a case with a factor 2 to spare.

Case -> attention kernel (``Case.note``), read off the dispatch in ``launch_attention`` (csrc/enc_attention.hip):
  S <= 64          enc_attention_s128_kernel<DT, dh, 64, 4>         S = 16, 64
  65 .. 128        enc_attention_s128_kernel<DT, dh, 128, 4>        S = 65, 128
  129 .. 256       enc_attention_s128_kernel<DT, dh, 256, 8>        S = 129, 256
  S > 256          enc_attention_kernel<DT, dh, 8>                  S = 257, 300 (3 query blocks), 511, 512 (4 query blocks)
each for dh = 32 and 64 and DT = fp16 and bf16.
"""
import numpy as np
import pytest

from oracle import encoder_cases as ec

pytestmark = pytest.mark.gpu

_ENCODERS = {}


def _encoder(geometry, S, seed, dtype):
    """One encoder per (geometry, gain, seed, dtype), shared by the tests of this module."""
    from mrag_amd.encoder import HipSentenceEncoder, EncoderSpec
    key = (geometry, ec.qk_gain(geometry, S), seed, dtype)
    if key not in _ENCODERS:
        if len(_ENCODERS) >= 6:
            _ENCODERS.pop(next(iter(_ENCODERS))).close()
        spec = ec.GEOMETRIES[geometry]
        _ENCODERS[key] = HipSentenceEncoder(EncoderSpec(**spec), ec._weights(geometry, seed, key[1]), dtype=dtype)
    return _ENCODERS[key]


def _check(got, want, tol, what):
    """Print the figure, then assert it."""
    err = float(np.abs(got - want).max())
    print(f"  {what}: max |gpu - oracle| {err:.2e}  tol {tol:.2e}  ({err / tol:.2f} of it)")
    assert np.isfinite(got).all(), what
    assert err <= tol, (what, err, tol)


def _compare_case(case, dtype, enc=None, tag=""):
    enc = enc or _encoder(case.geometry, case.S, case.seed, dtype)
    ids, mask = case.batch()
    sub = case.sample()
    ex = ec.case_expected(case.name, dtype)
    print(f"\n{case.name} {dtype}{tag} [{case.note}]")
    for pool, norm in ec.QUANTITIES:
        got = enc.forward(ids, mask, pool=pool, normalize=norm)
        assert got.shape == (len(ids), case.spec["hidden"]) and np.isfinite(got).all()
        _check(got[sub], ex.want[(pool, norm)], ex.tol[(pool, norm)], f"{pool}{'' if norm else '-raw'}")


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", ec.ATTENTION_CASES, ids=lambda c: c.name)
def test_attention_instances(case, dtype):
    """All 16 (head dim, key padding / general kernel, dtype) cells, S on both sides of 64 / 128 / 256 and up to max_position;
    every batch holds trailing and left padding, holes, mask values other than 0 / 1, rows of length 1 and 2, and single keys
    on the tile boundaries."""
    _compare_case(case, dtype)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", ec.GEMM_CASES, ids=lambda c: c.name)
def test_gemm_paths_small(case, dtype):
    """Skinny K-split GEMM at NFR 1 / 2 / 4 (M = 9, 16, 32, 64), the 128 x 128 kernel just past it (M = 65) and at M = 512."""
    _compare_case(case, dtype)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", ec.LARGE_CASES, ids=lambda c: c.name)
def test_fused_and_plain_256_flows(case, dtype, monkeypatch):
    """The fused-LayerNorm flow and the plain 256 x 256 flow (MRAG_ENC_NO_FUSED_LN=1) on the same batch, each against the oracle
    on a row sample that holds the first, the last, the shortest and the longest row; the bge batch is ragged (M_pad > M)."""
    ids, mask = case.batch()
    sub = case.sample()
    n = (mask != 0).sum(1)
    assert {0, len(ids) - 1, int(n.argmin()), int(n.argmax())} <= set(sub.tolist())
    enc = _encoder(case.geometry, case.S, case.seed, dtype)
    monkeypatch.delenv("MRAG_ENC_NO_FUSED_LN", raising=False)
    _compare_case(case, dtype, enc, " fused")
    fused = enc.forward(ids, mask, pool="mean")
    monkeypatch.setenv("MRAG_ENC_NO_FUSED_LN", "1")
    _compare_case(case, dtype, enc, " plain")
    plain = enc.forward(ids, mask, pool="mean")
    assert not np.array_equal(fused, plain)          # (the two flows did run)


_EMPTY = [("dh32", 48), ("dh64", 48), ("dh32", 100), ("dh64", 200), ("dh32", 300), ("dh64", 300)]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("geometry,S", _EMPTY)
def test_row_without_valid_token(geometry, S, dtype):
    """An all-zero mask row inside a normal batch: finite everywhere; the other rows as without it; the empty row as the oracle
    has it -- the zero vector for mean pooling, the even softmax over all S keys for CLS (S below the kernels' key padding:
    padding slots must not join that average)."""
    rows = (("trailing", S), ("trailing", S // 2), ("empty", 0), ("left", S // 3), ("holes", 0))
    case = ec.Case(f"empty-{geometry}-S{S}", geometry, S, rows, seed=5)
    ids, mask = case.batch()
    spec, w = case.spec, case.weights()
    ex = ec.expected(spec, w, ids, mask, dtype)
    keep = np.array([0, 1, 3, 4])
    enc = _encoder(geometry, S, case.seed, dtype)
    print(f"\n{case.name} {dtype}")
    for pool, norm in ec.QUANTITIES:
        what = f"{pool}{'' if norm else '-raw'}"
        got = enc.forward(ids, mask, pool=pool, normalize=norm)
        assert np.isfinite(got).all()
        _check(got, ex.want[(pool, norm)], ex.tol[(pool, norm)], what)
        _check(got[2:3], ex.want[(pool, norm)][2:3], ex.tol[(pool, norm)], what + " empty row")
        if pool == "mean":
            assert not got[2].any()
        without = enc.forward(ids[keep], mask[keep], pool=pool, normalize=norm)
        _check(got[keep], without, ex.tol[(pool, norm)], what + " other rows, with against without the empty row")


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("geometry", ["dh32", "dh64"])
@pytest.mark.parametrize("S", [60, 100, 200, 300])
def test_masked_token_ids_do_not_matter(geometry, S, dtype):
    """Other token ids at masked positions (slot 0 apart, which CLS pooling reads): every output bit unchanged (same kernels,
    same shapes), all four key-padding regimes."""
    case = ec.Case(f"inv-{geometry}-S{S}", geometry, S, tuple(ec.mixed_rows(S)), seed=5)
    ids, mask = case.batch()
    other = np.where(mask != 0, ids, (ids + 17) % case.spec["vocab_size"]).astype(np.int32)
    other[:, 0] = ids[:, 0]                 # CLS pooling returns slot 0 whether it is masked or not: its own token does matter
    assert (other != ids).any()
    enc = _encoder(geometry, S, case.seed, dtype)
    for pool, norm in ec.QUANTITIES:
        a = enc.forward(ids, mask, pool=pool, normalize=norm)
        b = enc.forward(other, mask, pool=pool, normalize=norm)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (pool, norm)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("geometry", ["dh32", "dh64"])
def test_padding_length_does_not_matter(geometry, dtype):
    """The same valid tokens padded to S = 60 / 64 / 100 / 128 / 200 / 256 / 300 (more trailing masked slots): the SP 64 / 128 /
    256 and the general attention kernels agree with one another within the tolerance of the S = 60 batch.  One gain for all
    lengths here: the weights must be the same."""
    from mrag_amd.encoder import HipSentenceEncoder, EncoderSpec
    spec = ec.GEOMETRIES[geometry]
    w = ec.sharp_weights(spec, 9, ec.qk_gain(geometry, 60))
    rng = np.random.default_rng(3)
    lens = [60, 1, 2, 59, 31, 17]
    ids60 = rng.integers(3, spec["vocab_size"], size=(len(lens), 60)).astype(np.int32)
    mask60 = np.stack([ec.mask_row("trailing", 60, L) for L in lens])
    mask60[4, 7:12] = 0                                          # a hole as well
    ex = ec.expected(spec, w, ids60, mask60, dtype)
    enc = HipSentenceEncoder(EncoderSpec(**spec), w, dtype=dtype)
    print(f"\npadding length {geometry} {dtype}")
    outs = {}
    for S in (60, 64, 100, 128, 200, 256, 300):
        ids = rng.integers(3, spec["vocab_size"], size=(len(lens), S)).astype(np.int32)
        mask = np.zeros((len(lens), S), dtype=np.int32)
        ids[:, :60], mask[:, :60] = ids60, mask60
        outs[S] = {q: enc.forward(ids, mask, pool=q[0], normalize=q[1]) for q in ec.QUANTITIES}
    enc.close()
    for S, out in outs.items():
        for q in ec.QUANTITIES:
            what = f"S {S} {q[0]}{'' if q[1] else '-raw'}"
            _check(out[q], ex.want[q], ex.tol[q], what + " against the oracle")
            if S != 60:
                _check(out[q], outs[60][q], ex.tol[q], what + " against S 60")


def test_ids_outside_the_vocabulary_are_rejected():
    """``forward`` raises on an id below 0 or at / above vocab_size (the embedding kernel would clamp it to a wrong row
    silently); the batch next to it still runs."""
    case = ec.CASE_BY_NAME["dh32-S16"]
    enc = _encoder(case.geometry, case.S, case.seed, "f16")
    ids, mask = case.batch()
    vocab = case.spec["vocab_size"]
    for bad in (-1, vocab, vocab + 5, np.iinfo(np.int32).max):
        broken = ids.copy()
        broken[1, 3] = bad                                       # a masked slot: rejected all the same
        with pytest.raises(ValueError, match="vocab"):
            enc.forward(broken, mask)
    edge = ids.copy()
    edge[0, 0], edge[0, 1] = 0, vocab - 1
    assert np.isfinite(enc.forward(edge, mask)).all()


# ---------------------------------------------------------------------------------------------- the C entry points directly
def _create(spec, dtype="f16"):
    """``mrag_encoder_create`` -> (library, handle): no parameter set yet."""
    import ctypes as C
    from mrag_amd import _native as N
    lib = N.load()
    cfg = N.EncoderConfig(spec["vocab_size"], spec["hidden"], spec["layers"], spec["heads"], spec["intermediate"],
                          spec["max_position"], spec["type_vocab_size"], spec["layer_norm_eps"],
                          N.MRAG_F16 if dtype == "f16" else N.MRAG_BF16)
    h = C.c_uint64(0)
    N.check(lib.mrag_encoder_create(C.byref(cfg), 0, C.byref(h)))
    return lib, h


def _set_param(lib, h, name, arr, numel=None):
    """``mrag_encoder_set_param`` from a host array -> status (0 = accepted)."""
    a = np.ascontiguousarray(arr, dtype=np.float32)
    return lib.mrag_encoder_set_param(h, name.encode(), a.ctypes.data, a.size if numel is None else numel, 0, None)


def _missing(lib, h):
    import ctypes as C
    from mrag_amd import _native as N
    miss = C.c_int(-1)
    N.check(lib.mrag_encoder_missing_params(h, C.byref(miss)))
    return miss.value


def _forward(lib, h, ids, mask, hidden, pool, normalize):
    """``mrag_encoder_forward`` on host buffers -> (status, output)."""
    from mrag_amd import _native as N
    ids, mask = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(mask, dtype=np.int32)
    out = np.zeros((len(ids), hidden), dtype=np.float32)
    st = lib.mrag_encoder_forward(h, ids.ctypes.data, mask.ctypes.data, ids.shape[0], ids.shape[1], out.ctypes.data,
                                  N.POOL_CLS if pool == "cls" else N.POOL_MEAN, int(normalize), 0, None)
    return st, out


def test_parameter_table():
    """``mrag_encoder_set_param`` / ``mrag_encoder_missing_params`` on the ``tiny`` architecture (geometry dh32): the count of
    missing parameters starts at 5 + 16 x layers and drops by one per distinct accepted name; a wrong element count (a matrix, a
    bias, one of the q / k / v blocks), an unknown suffix, a layer past the last and a layer prefix without its second dot are
    rejected and set nothing; a forward with one parameter missing is refused.  With all of them set the case meets the oracle;
    with the key and value weights of layer 0 swapped at upload it misses it by more than the case's tolerance (the swap moves
    the fp64 oracle by 15 x tol or more in every quantity): the order of the three row blocks of the fused QKV Linear."""
    case = ec.CASE_BY_NAME["dh32-S16"]
    spec, w = case.spec, case.weights()
    H, I, layers = spec["hidden"], spec["intermediate"], spec["layers"]
    ids, mask = case.batch()
    lib, h = _create(spec, "f16")
    try:
        left = 5 + 16 * layers
        assert len(w) == left and _missing(lib, h) == left
        wrong = (("encoder.layer.0.intermediate.dense.weight", I * H - 1), ("encoder.layer.1.output.dense.bias", H + 1),
                 ("encoder.layer.1.attention.self.key.weight", H * H + H), ("encoder.layer.0.attention.self.value.bias", H - 1))
        for name, numel in wrong:                                     # wrong size: an error, and the name stays missing
            assert _set_param(lib, h, name, np.zeros(numel), numel) != 0, name
            assert _missing(lib, h) == left, name
        some = w["encoder.layer.0.output.dense.bias"]
        for name in ("encoder.layer.0.output.dense.gain", "encoder.layer.0.output.dense.bias.", "output.dense.bias",
                     f"encoder.layer.{layers}.output.dense.bias", "encoder.layer.-1.output.dense.bias",
                     "encoder.layer.", "encoder.layer.0", "encoder.layer.0output.dense.bias", "embeddings.LayerNorm", ""):
            assert _set_param(lib, h, name, some) != 0, name
            assert _missing(lib, h) == left, name
        names = list(w)
        last = "encoder.layer.1.attention.self.value.weight"
        names.remove(last)
        for name in names:
            assert _set_param(lib, h, name, w[name]) == 0, name
            left -= 1
            assert _missing(lib, h) == left, name
            if name.endswith("query.bias") or name.endswith("LayerNorm.weight"):
                assert _set_param(lib, h, name, w[name]) == 0, name     # the same name again: accepted, counted once
                assert _missing(lib, h) == left, name
        assert left == 1
        st, _ = _forward(lib, h, ids, mask, H, "mean", True)
        assert st != 0                                                  # one parameter missing: refused
        assert _set_param(lib, h, last, w[last]) == 0 and _missing(lib, h) == 0
        ex = ec.case_expected(case.name, "f16")
        print(f"\nparameter table, {case.name} f16")
        for q in ec.QUANTITIES:
            st, got = _forward(lib, h, ids, mask, H, *q)
            assert st == 0
            _check(got, ex.want[q], ex.tol[q], f"{q[0]}{'' if q[1] else '-raw'}")
        k, v = "encoder.layer.0.attention.self.key.weight", "encoder.layer.0.attention.self.value.weight"
        assert _set_param(lib, h, k, w[v]) == 0 and _set_param(lib, h, v, w[k]) == 0 and _missing(lib, h) == 0
        for q in ec.QUANTITIES:
            st, got = _forward(lib, h, ids, mask, H, *q)
            assert st == 0 and np.isfinite(got).all()
            err = float(np.abs(got - ex.want[q]).max())
            print(f"  key / value swapped, {q[0]}{'' if q[1] else '-raw'}: max |gpu - oracle| {err:.2e} = {err / ex.tol[q]:.1f} tol")
            assert err > ex.tol[q], (q, err, ex.tol[q])
    finally:
        lib.mrag_encoder_destroy(h)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_refold_after_parameter_change(dtype, monkeypatch):
    """The folded copies of the fused-LayerNorm flow follow a parameter change.  MiniLM widths, 2 layers, 512 x 32 tokens
    (M_pad = 16384: the smallest batch whose fused flow engages on 256 CUs).  Handle A runs a forward (which folds), then gets
    another ``encoder.layer.0.output.LayerNorm.bias`` -- a parameter the fused flow reads only through the folded QKV bias and
    the beta-augmented attention-output bias of layer 1 -- and runs again; handle B is created with the changed weights.  A's
    second output equals B's bit for bit (the same kernels on the same inputs, partial sums added in slot order) and differs
    from A's first."""
    from mrag_amd.encoder import HipSentenceEncoder, EncoderSpec
    case = ec.CASE_BY_NAME["large-minilm-512x32"]
    monkeypatch.delenv("MRAG_ENC_NO_FUSED_LN", raising=False)
    ids, mask = case.batch()
    w = dict(case.weights())
    name = "encoder.layer.0.output.LayerNorm.bias"
    a = HipSentenceEncoder(EncoderSpec(**case.spec), w, dtype=dtype)
    b = None
    try:
        first = a.forward(ids, mask, pool="mean")
        w[name] = (w[name] + np.linspace(-0.5, 0.5, w[name].size)).astype(np.float32)
        assert _set_param(a._lib, a._h, name, w[name]) == 0
        second = a.forward(ids, mask, pool="mean")
        b = HipSentenceEncoder(EncoderSpec(**case.spec), w, dtype=dtype)
        fresh = b.forward(ids, mask, pool="mean")
        again = b.forward(ids, mask, pool="mean")
    finally:
        a.close()
        if b is not None:
            b.close()
    assert np.isfinite(second).all() and np.isfinite(fresh).all()
    print(f"\nre-fold {dtype}: max |second - first| {float(np.abs(second - first).max()):.2e}, "
          f"max |second - fresh handle| {float(np.abs(second - fresh).max()):.2e}, "
          f"fresh handle twice {float(np.abs(again - fresh).max()):.2e}")
    assert np.array_equal(fresh.view(np.uint32), again.view(np.uint32))        # (a handle reproduces itself)
    assert np.array_equal(second.view(np.uint32), fresh.view(np.uint32))
    assert not np.array_equal(second, first)
