"""HBM-resident dense indexes over the C ABI (include/mrag.h).

``DenseIndex`` is the corpus-scale form of the reference's dense scoring
(app/modules/retrieval/retrieval_backend.py:245,371-372: cosine every candidate, sort
descending, truncate): rows are L2-normalised and rounded once to fp16/bf16, kept in
HBM, and every search is one fused MFMA similarity + top-k pass.  Tie-break: score
descending, then row ascending.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from typing import Optional, Tuple

import numpy as np

from . import _native as N

_NP_DT = {np.dtype(np.float32): N.MRAG_F32, np.dtype(np.float16): N.MRAG_F16, np.dtype(np.float64): N.MRAG_F64}


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def _torch_dtype_code(t) -> int:
    import torch
    return {torch.float32: N.MRAG_F32, torch.float16: N.MRAG_F16, torch.bfloat16: N.MRAG_BF16,
            torch.float64: N.MRAG_F64}[t.dtype]


def _as_buffer(x, dim: int):
    """-> (keepalive, pointer, n_rows, dtype_code, is_device)."""
    if _is_torch(x):
        if x.dim() != 2 or x.shape[1] != dim:
            raise ValueError(f"expected [n, {dim}] rows, got {tuple(x.shape)}")
        x = x.contiguous()
        if x.is_cuda:
            return x, x.data_ptr(), x.shape[0], _torch_dtype_code(x), 1
        if x.dtype.is_floating_point and str(x.dtype) == "torch.bfloat16":
            return x, x.data_ptr(), x.shape[0], N.MRAG_BF16, 0
        x = x.numpy()
    a = np.ascontiguousarray(x)
    if a.ndim != 2 or a.shape[1] != dim:
        raise ValueError(f"expected [n, {dim}] rows, got {a.shape}")
    if a.dtype not in _NP_DT:
        a = a.astype(np.float32)
    return a, a.ctypes.data, a.shape[0], _NP_DT[a.dtype], 0


FILTER_PATHS = {"auto": N.FILTER_AUTO, "mask": N.FILTER_MASK, "compact": N.FILTER_COMPACT}
_FILTER_NAMES = {N.FILTER_MASK: "mask", N.FILTER_COMPACT: "compact"}


def allow_bits(allow, n: int) -> np.ndarray:
    """Host allow-set -> the ABI's MRAG_ALLOW_BITS32 words (uint32 [ceil(n/32)], bit r%32 of word r/32).

    ``allow`` is a bool / uint8 mask of length ``n`` (nonzero = allowed) or a 1-D array of row positions
    ``0 .. n-1`` (any other integer dtype).  A wrong length, a position outside the rows or an input that is not
    1-D raises ``ValueError``; nothing is clamped."""
    if _is_torch(allow):
        allow = allow.cpu().numpy()
    a = np.asarray(allow)
    if a.ndim != 1:
        raise ValueError(f"allow must be 1-D, got shape {a.shape}")
    if a.dtype == np.bool_ or a.dtype == np.uint8:
        if a.shape[0] != n:
            raise ValueError(f"allow mask has {a.shape[0]} entries, the index holds {n} rows")
        mask = a.astype(np.bool_, copy=False)
    elif np.issubdtype(a.dtype, np.integer):
        if a.size and (int(a.min()) < 0 or int(a.max()) >= n):
            raise ValueError(f"allow row positions must lie in [0, {n}), got [{int(a.min())}, {int(a.max())}]")
        mask = np.zeros(n, dtype=np.bool_)
        mask[a] = True
    else:
        raise ValueError(f"allow must be a bool/uint8 mask or integer row positions, got dtype {a.dtype}")
    words = (n + 31) // 32
    packed = np.zeros(words * 4, dtype=np.uint8)
    packed[:(n + 7) // 8] = np.packbits(mask, bitorder="little")
    return packed.view("<u4")


def _allow_buffer(allow, n: int, device: int):
    """-> (keepalive, pointer, allow_format, is_device).  Device tensors (bool / uint8, on the index's device) go to the
    ABI as a byte mask, packed on the device; everything else is packed here."""
    if _is_torch(allow) and allow.is_cuda:
        import torch
        if allow.dim() != 1 or allow.shape[0] != n:
            raise ValueError(f"device allow mask must be 1-D with {n} entries, got {tuple(allow.shape)}")
        if allow.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"device allow must be a bool/uint8 mask (row positions: pass a host array), got {allow.dtype}")
        if allow.device.index != device:
            raise ValueError(f"allow mask is on {allow.device}, the index on cuda:{device}")
        t = allow.contiguous()
        return t, t.data_ptr(), N.ALLOW_BYTES, 1
    bits = np.ascontiguousarray(allow_bits(allow, n))
    return bits, bits.ctypes.data, N.ALLOW_BITS32, 0


def pack_sets(sets, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """Host allow-sets -> the CSR of ``mrag_index_search_sets``: ``(set_ptr int64 [len(sets) + 1], set_rows int64)``.

    Every entry of ``sets`` is what :func:`allow_bits` takes: a bool / uint8 mask of length ``n`` or a 1-D array of row
    positions ``0 .. n-1``.  Positions come out sorted and deduplicated, as a mask gives them; a wrong mask length, a
    position outside the rows or an input that is not 1-D raises ``ValueError``.  No GPU is needed."""
    rows = []
    for s, one in enumerate(sets):
        if _is_torch(one):
            one = one.cpu().numpy()
        a = np.asarray(one)
        if a.ndim != 1:
            raise ValueError(f"set {s} must be 1-D, got shape {a.shape}")
        if a.dtype == np.bool_ or a.dtype == np.uint8:
            if a.shape[0] != n:
                raise ValueError(f"set {s}: the mask has {a.shape[0]} entries, the index holds {n} rows")
            r = np.flatnonzero(a).astype(np.int64)
        elif np.issubdtype(a.dtype, np.integer) or a.size == 0:
            r = np.unique(a.astype(np.int64))
            if r.size and (int(r[0]) < 0 or int(r[-1]) >= n):
                raise ValueError(f"set {s}: row positions must lie in [0, {n}), got [{int(r[0])}, {int(r[-1])}]")
        else:
            raise ValueError(f"set {s} must be a bool/uint8 mask or integer row positions, got dtype {a.dtype}")
        rows.append(r)
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    if rows:
        np.cumsum([r.shape[0] for r in rows], out=ptr[1:])
    flat = np.ascontiguousarray(np.concatenate(rows)) if rows else np.zeros(0, dtype=np.int64)
    return ptr, flat.astype(np.int64, copy=False)


def group_ptr_of(group_ptr, sizes, nq: int) -> np.ndarray:
    """The ``group_ptr`` of ``mrag_index_search_groups`` (int64 [n_groups + 1]) from itself or from the questions' group
    ``sizes`` (exactly one of the two), checked against ``nq`` query rows: it starts at 0, never decreases and ends at
    ``nq``.  ``ValueError`` otherwise.  No GPU is needed."""
    if (group_ptr is None) == (sizes is None):
        raise ValueError("pass exactly one of group_ptr and sizes")
    a = np.asarray(group_ptr if sizes is None else sizes)
    if a.ndim != 1 or not (np.issubdtype(a.dtype, np.integer) or a.size == 0) or a.dtype == np.bool_:
        raise ValueError(f"group_ptr / sizes must be 1-D integers, got shape {a.shape} dtype {a.dtype}")
    a = a.astype(np.int64)
    if sizes is not None:
        if a.size and int(a.min()) < 0:
            raise ValueError(f"question {int(np.flatnonzero(a < 0)[0])} has a negative group size")
        a = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(a, dtype=np.int64)])
    if a.size == 0 or a[0] != 0:
        raise ValueError("group_ptr must start at 0")
    if (np.diff(a) < 0).any():
        raise ValueError(f"group_ptr decreases at question {int(np.flatnonzero(np.diff(a) < 0)[0])}")
    if int(a[-1]) != nq:
        raise ValueError(f"the groups hold {int(a[-1])} queries, {nq} were given")
    return np.ascontiguousarray(a)


def row_keys_of(values) -> Tuple[np.ndarray, int, int]:
    """One hashable value per row (a title, a document id, a tenant) -> ``(keys, n_keys, m)``: int32 keys numbered in order
    of first appearance (the form ``mrag_index_set_row_keys`` takes), the number of distinct keys and the largest number
    of rows that share one.  No GPU is needed."""
    seen: dict = {}
    keys = np.empty(len(values), dtype=np.int32)
    for r, v in enumerate(values):
        keys[r] = seen.setdefault(v, len(seen))
    m = int(np.bincount(keys).max()) if len(keys) else 0
    return keys, len(seen), m


def collapse_scan_k(k: int, m: int, n: int) -> int:
    """The default scan depth of :meth:`DenseIndex.search_collapsed` for ``k`` keys over ``n`` rows of which at most ``m``
    share a key: ``min(256, n, max(k, (k - 1) * m + 1))``, never below ``k``.  The first ``(k - 1) * m + 1`` rows of the
    declared order hold ``k`` keys, so below the 256 cap this depth never needs a redo round.  Nobody has measured
    whether it, or a shallower scan with an occasional redo, is the faster default (``tools/perf_search_collapsed.py``
    times both)."""
    k = _check_k(k, 256)
    return max(k, min(256, int(n), max(k, (k - 1) * int(m) + 1)))


NEIGHBORS_MAX_WINDOW, NEIGHBORS_MAX_SEEDS, NEIGHBORS_MAX_ENTRIES = 16, 256, 4096


def reference_decay(window: int) -> np.ndarray:
    """The reference's score of a sentence at hop distance ``0 .. window`` from a matching sentence (graph_utils.py:87-94)
    -> fp64 ``[window + 1]``: 1.0, 0.7, 0.5, then ``max(0.5 - 0.1 * (d - 2), 0.1)``, computed in Python floats as the
    reference computes them (0.19999999999999996 at d = 5, the 0.1 floor from d = 6 on).  No GPU is needed."""
    if isinstance(window, (bool, np.bool_)) or not isinstance(window, numbers.Integral) or int(window) < 0:
        raise ValueError(f"window must be a non-negative integer, got {window!r}")
    first = (1.0, 0.7, 0.5)
    return np.asarray([first[d] if d < 3 else max(0.5 - 0.1 * (d - 2), 0.1) for d in range(int(window) + 1)], dtype=np.float64)


IVF_FILTER_PATHS = {"auto": N.IVF_FILTER_AUTO, "probe": N.IVF_FILTER_PROBE, "exact": N.IVF_FILTER_EXACT}
_IVF_FILTER_NAMES = {N.IVF_FILTER_PROBE: "probe", N.IVF_FILTER_EXACT: "exact"}


def ivf_choose_filter_path(nq: int, k: int, nprobe: int, nlist: int, total_rows: int, allowed_rows: int, dim: int) -> str:
    """AUTO's rule of the filtered IVF search (``mrag_ivf_choose_filter_path``, pure arithmetic: no GPU needed):
    "exact" (filtered brute force) when ``nprobe >= nlist`` or the allowed rows are few next to the rows the probes
    scan, else "probe".  Sharded callers apply it to the global counts."""
    out = C.c_int(0)
    N.check(N.load().mrag_ivf_choose_filter_path(int(nq), int(k), int(nprobe), int(nlist), int(total_rows), int(allowed_rows),
                                                 int(dim), C.byref(out)))
    return _IVF_FILTER_NAMES[out.value]


PRECISIONS = ("exact", "fp8")
_FP8_REGIMES = {N.FP8_BATCH: "batch", N.FP8_STREAM: "stream"}


def fp8_default_refine(k: int) -> int:
    """Candidate pool of an fp8 search when ``refine`` is not given (``mrag_index_fp8_default_refine``, no GPU
    needed): ``min(64, max(40, 4k))`` for ``1 <= k <= 64``; any other ``k`` raises :class:`MragError`."""
    out = C.c_int(0)
    N.check(N.load().mrag_index_fp8_default_refine(int(k), C.byref(out)))
    return out.value


def _check_precision(precision, refine, allow) -> Tuple[bool, int]:
    """The ``precision`` / ``refine`` arguments of a search, checked before any library call -> (fp8, refine for the ABI:
    0 = the default pool)."""
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
    if precision == "fp8" and allow is not None:
        raise ValueError("precision='fp8' does not combine with allow= (filtered search is exact only)")
    if refine is not None and precision != "fp8":
        raise ValueError("refine applies to precision='fp8' only")
    fp8 = precision == "fp8"
    r = 0 if refine is None else int(refine)
    if fp8 and r < 0:
        raise ValueError(f"refine must be positive, got {refine}")
    return fp8, r


def range_floor(min_score) -> np.float32:
    """The fp32 floor a range search compares against: the smallest float32 >= ``min_score`` (so that "score >= floor"
    on the fp32 scores means "score >= min_score").  NaN, +-inf and values beyond the float32 range raise ``ValueError``."""
    if isinstance(min_score, (bool, np.bool_)) or not isinstance(min_score, numbers.Real):
        raise ValueError(f"min_score must be a real number, got {min_score!r}")
    x = float(min_score)
    if not math.isfinite(x):
        raise ValueError(f"min_score must be finite, got {min_score!r}")
    with np.errstate(over="ignore"):
        f = np.float32(x)
    if not np.isfinite(f):
        raise ValueError(f"min_score {min_score!r} lies outside the float32 range")
    if float(f) < x:
        f = np.nextafter(f, np.float32(np.inf))
    return f


def _check_k(k, k_max: int) -> int:
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, numbers.Integral) or not 1 <= int(k) <= k_max:
        raise ValueError(f"k must be an integer in [1, {k_max}], got {k!r}")
    return int(k)


def _stream_ptr(stream) -> Optional[int]:
    if stream is None:
        return None
    return int(getattr(stream, "cuda_stream", stream))


def _run_search(call, queries, nq: int, k: int, is_dev: int, device: int, stream, device_work: bool, out=None):
    """What every search method shares: results [nq, k] where the queries live (CUDA tensors on their device, ``out``
    reused when given, or numpy arrays), ``stream`` defaulting to torch's current stream when the call works on device
    buffers (``device_work``), then ``call(scores_ptr, ids_ptr, out_is_device, stream_ptr)``.  The caller holds every
    buffer the call reads until it returns."""
    if device_work and stream is None:
        import torch
        stream = torch.cuda.current_stream(device)
    if is_dev:
        import torch
        if out is None:
            sc = torch.empty((nq, k), dtype=torch.float32, device=queries.device)
            ids = torch.empty((nq, k), dtype=torch.int64, device=queries.device)
        else:
            sc, ids = out
        N.check(call(sc.data_ptr(), ids.data_ptr(), 1, _stream_ptr(stream)))
        return sc, ids
    sc = np.empty((nq, k), dtype=np.float32)
    ids = np.empty((nq, k), dtype=np.int64)
    N.check(call(sc.ctypes.data, ids.ctypes.data, 0, _stream_ptr(stream)))
    return sc, ids


def _third_output(out, wanted: bool, name: str, shape, keep, is_dev):
    """The optional int32 third output (``which`` / ``keys``) of a search -> (array or None, its pointer or None): ``out[2]``
    when the caller passes three buffers, else a new array beside the queries when it is wanted."""
    if out is not None and wanted and len(out) < 3:
        raise ValueError(f"return_{name}=True needs out=(scores, ids, {name})")
    third = None
    if out is not None and len(out) > 2:
        third = out[2]
    elif wanted and is_dev:
        import torch
        third = torch.empty(shape, dtype=torch.int32, device=keep.device)
    elif wanted:
        third = np.empty(shape, dtype=np.int32)
    return third, None if third is None else (third.data_ptr() if is_dev else third.ctypes.data)


class DenseIndex:
    """Brute-force cosine (or inner-product) top-k index on one GPU."""

    def __init__(self, dim: int, metric: str = "cosine", dtype: str = "f16", device: int = 0, fp8_scan: bool = False):
        self._lib = N.load()
        self.dim, self.metric, self.dtype, self.device = int(dim), metric, dtype, int(device)
        h = C.c_uint64(0)
        N.check(self._lib.mrag_index_create(self.dim, N.METRIC_COSINE if metric == "cosine" else N.METRIC_IP,
                                            N.MRAG_F16 if dtype == "f16" else N.MRAG_BF16, self.device, C.byref(h)))
        self._h = h
        self.id_base = 0
        if fp8_scan:
            self.enable_fp8()

    def enable_fp8(self):
        """Keep an fp8 (e4m3fn) copy of the rows for ``search(precision="fp8")`` (``mrag_index_enable_fp8``): built
        from the rows already stored, then kept current by every add.  Cosine indexes only; idempotent."""
        N.check(self._lib.mrag_index_enable_fp8(self._h))

    # -- lifetime -------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.mrag_index_destroy(self._h)
            self._h = C.c_uint64(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        n = C.c_int64(0)
        N.check(self._lib.mrag_index_size(self._h, C.byref(n)))
        return n.value

    def _norm(self, normalize):
        return int(bool(self.metric == "cosine" if normalize is None else normalize))

    def _last_record(self, fn, *names) -> dict:
        """the three int64 figures of a ``mrag_index_last_*`` call under ``names``"""
        v = [C.c_int64(0) for _ in names]
        N.check(fn(self._h, *[C.byref(x) for x in v]))
        return {name: x.value for name, x in zip(names, v)}

    # -- build ----------------------------------------------------------------------------
    def reserve(self, n_rows: int):
        N.check(self._lib.mrag_index_reserve(self._h, int(n_rows)))

    def set_id_base(self, base: int):
        N.check(self._lib.mrag_index_set_id_base(self._h, int(base)))
        self.id_base = int(base)

    def add(self, rows, normalize: Optional[bool] = None, stream=None):
        """Append rows ([n, dim] numpy / torch, host or device).  ``normalize`` defaults to
        True for the cosine metric; pass False for rows that are already normalised and
        rounded (they are then stored bit-for-bit when their dtype is the storage dtype)."""
        norm = self._norm(normalize)
        keep, ptr, n, dt, is_dev = _as_buffer(rows, self.dim)
        if is_dev and stream is None:
            import torch
            stream = torch.cuda.current_stream(self.device)   # stream-ordered with the producer of `rows`
        N.check(self._lib.mrag_index_add(self._h, ptr, n, dt, norm, is_dev, _stream_ptr(stream)))
        del keep

    def rows(self, row0: int = 0, n: Optional[int] = None) -> np.ndarray:
        n = len(self) - row0 if n is None else n
        out = np.empty((n, self.dim), dtype=np.float32)
        N.check(self._lib.mrag_index_get_rows(self._h, int(row0), int(n), out.ctypes.data, 0, None))
        return out

    def rows_fp8(self, row0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """The fp8 copy of rows ``[row0, row0 + n)`` as its raw e4m3fn bytes ([n, dim] uint8)."""
        n = len(self) - row0 if n is None else n
        out = np.empty((n, self.dim), dtype=np.uint8)
        N.check(self._lib.mrag_index_get_rows_fp8(self._h, int(row0), int(n), out.ctypes.data, 0, None))
        return out

    # -- search ---------------------------------------------------------------------------
    def search(self, queries, k: int, normalize: Optional[bool] = None, stream=None, out=None, allow=None,
               filter_path: str = "auto", precision: str = "exact", refine: Optional[int] = None
               ) -> Tuple["np.ndarray", "np.ndarray"]:
        """-> (scores [nq,k] fp32 descending, ids [nq,k] int64; (-inf, -1) past the corpus).

        Host queries give numpy results (the call returns when they have landed); CUDA
        tensors give CUDA tensors, written asynchronously on ``stream`` (default: torch's
        current stream).  ``out=(scores, ids)`` reuses caller tensors.

        ``allow`` restricts the search to some rows (``mrag_index_search_filtered``): a bool / uint8 mask over the
        ``len(self)`` local rows (numpy, or a torch tensor on the host or on this index's device) or a host array of
        row positions.  Slots past the number of allowed rows are (-inf, -1).  ``filter_path``: "auto", "mask" (the
        search kernels drop disallowed rows) or "compact" (the allowed rows are gathered and searched alone); see
        :meth:`last_filter`.  ``allow=None`` is the plain search.

        ``precision="fp8"`` (index built with ``fp8_scan=True`` or :meth:`enable_fp8`; ``1 <= k <= 64``) picks the
        ``refine`` best rows per query (``k <= refine <= 64``; None: :func:`fp8_default_refine`) from the fp8 copy and
        re-scores them exactly against the 16-bit rows: the scores are exact, the row set is approximate (measured
        recall in DESIGN.md).  It does not combine with ``allow``."""
        fp8, r = _check_precision(precision, refine, allow)
        norm = self._norm(normalize)
        if allow is not None:
            return self._search_filtered(queries, k, norm, stream, out, allow, filter_path)
        keep, ptr, nq, dt, is_dev = _as_buffer(queries, self.dim)
        if fp8:
            def call(sc, ids, out_dev, st):
                return self._lib.mrag_index_search_fp8(self._h, ptr, nq, dt, norm, is_dev, int(k), r, sc, ids, out_dev, st)
        else:
            def call(sc, ids, out_dev, st):
                return self._lib.mrag_index_search(self._h, ptr, nq, dt, norm, is_dev, int(k), sc, ids, out_dev, st)
        return _run_search(call, keep, nq, k, is_dev, self.device, stream, bool(is_dev), out)

    def _search_filtered(self, queries, k, norm, stream, out, allow, filter_path):
        if filter_path not in FILTER_PATHS:
            raise ValueError(f"filter_path must be one of {sorted(FILTER_PATHS)}, got {filter_path!r}")
        n = len(self)
        akeep, aptr, afmt, adev = _allow_buffer(allow, n, self.device)
        keep, ptr, nq, dt, is_dev = _as_buffer(queries, self.dim)
        path = FILTER_PATHS[filter_path]

        def call(sc, ids, out_dev, st):
            return self._lib.mrag_index_search_filtered(self._h, ptr, nq, dt, norm, is_dev, int(k), aptr, n, afmt,
                                                        adev, path, sc, ids, out_dev, st)
        return _run_search(call, keep, nq, k, is_dev, self.device, stream, bool(is_dev or adev), out)

    def range_search(self, queries, min_score: float, k: int, normalize: Optional[bool] = None, allow=None,
                     filter_path: str = "auto", stream=None, out=None, precision: str = "exact"):
        """Rows scoring >= ``min_score`` (``mrag_index_search_range``) -> (scores [nq,k] fp32, ids [nq,k] int64, counts [nq]
        int64).

        Per query, with c = the number of rows scoring >= ``min_score`` (inclusive; the floor is the smallest float32 >=
        ``min_score``, see :func:`range_floor`): the best ``min(k, c)`` of them, (score desc, row asc), then (-inf, -1)
        slots; ``counts[q] = c`` exactly, so a query is truncated when ``counts[q] > k``.  Scores are the ones
        :meth:`search` computes, and the search is exact.  ``min_score`` must be finite and ``1 <= k <= 256``
        (``ValueError`` otherwise, before any GPU work).  Host queries give numpy arrays; CUDA tensors give CUDA tensors
        written on ``stream``; ``out=(scores, ids, counts)`` reuses buffers.  ``allow`` / ``filter_path`` as in
        :meth:`search`.  There is no fp8 range search: ``precision="fp8"`` raises ``ValueError``."""
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
        if precision == "fp8":
            raise ValueError("precision='fp8' does not combine with a score floor (range search is exact only)")
        floor = range_floor(min_score)
        k = _check_k(k, self.max_k())
        if filter_path not in FILTER_PATHS:
            raise ValueError(f"filter_path must be one of {sorted(FILTER_PATHS)}, got {filter_path!r}")
        norm = self._norm(normalize)
        n, akeep, aptr, afmt, adev = 0, None, None, N.ALLOW_BITS32, 0
        if allow is not None:
            n = len(self)
            akeep, aptr, afmt, adev = _allow_buffer(allow, n, self.device)
        keep, ptr, nq, dt, is_dev = _as_buffer(queries, self.dim)
        if out is not None:
            counts = out[2]
        elif is_dev:
            import torch
            counts = torch.empty(nq, dtype=torch.int64, device=keep.device)
        else:
            counts = np.empty(nq, dtype=np.int64)
        path = FILTER_PATHS[filter_path]

        def call(sc, ids, out_dev, st):
            cptr = counts.data_ptr() if out_dev else counts.ctypes.data
            return self._lib.mrag_index_search_range(self._h, ptr, nq, dt, norm, is_dev, k, float(floor), aptr, n, afmt, adev,
                                                     path, sc, ids, cptr, out_dev, st)
        sc, ids = _run_search(call, keep, nq, k, is_dev, self.device, stream, bool(is_dev or adev),
                              None if out is None else (out[0], out[1]))
        del akeep
        return sc, ids, counts

    def self_join(self, min_score: float, k: int = 64, batch: int = 16384):
        """Every stored row as a query against all the others: its epsilon-neighbour list -> CUDA tensors on this index's
        device (scores [n,k] fp32, ids [n,k] int64, counts [n] int64), as :meth:`range_search` returns them with the row
        itself removed (``1 <= k <= 255``).

        The stored 16-bit rows go to the search kernels device to device (unpacked to fp32 and rounded back: the same
        bits, no renormalisation).  Batches of ``batch`` rows run in order on torch's current stream; the result does not
        depend on ``batch``.  Each batch asks for k + 1 rows so that the row's own entry can be dropped exactly, also among
        duplicate rows that tie with it; ``counts`` excludes the row itself when it reached the floor (with
        ``metric="ip"`` it may not).  When more than k rows tie with or beat the row's own score its entry is not among
        the k + 1 listed, and whether it reached the floor is decided from its fp64 self dot product."""
        import torch
        floor = range_floor(min_score)
        k = _check_k(k, self.max_k() - 1)
        if isinstance(batch, (bool, np.bool_)) or not isinstance(batch, numbers.Integral) or int(batch) < 1:
            raise ValueError(f"batch must be a positive integer, got {batch!r}")
        n, dev = len(self), torch.device("cuda", self.device)
        scores = torch.empty((n, k), dtype=torch.float32, device=dev)
        ids = torch.empty((n, k), dtype=torch.int64, device=dev)
        counts = torch.empty(n, dtype=torch.int64, device=dev)
        if n == 0:
            return scores, ids, counts
        stream = torch.cuda.current_stream(dev)
        b = min(int(batch), n)
        rows = torch.empty((b, self.dim), dtype=torch.float32, device=dev)
        sc_b = torch.empty((b, k + 1), dtype=torch.float32, device=dev)
        id_b = torch.empty((b, k + 1), dtype=torch.int64, device=dev)
        cnt_b = torch.empty(b, dtype=torch.int64, device=dev)
        with torch.cuda.stream(stream):
            for r0 in range(0, n, b):
                m = min(b, n - r0)
                q = rows[:m]
                N.check(self._lib.mrag_index_get_rows(self._h, r0, m, q.data_ptr(), 1, _stream_ptr(stream)))
                s, i, c = self.range_search(q, float(floor), k + 1, normalize=False, stream=stream,
                                            out=(sc_b[:m], id_b[:m], cnt_b[:m]))
                own = torch.arange(r0, r0 + m, device=dev, dtype=torch.int64) + self.id_base
                is_self = i == own[:, None]
                found = is_self.any(dim=1)
                # the row's own entry moves behind the others (stable), the first k remain
                order = torch.argsort(is_self.to(torch.int8), dim=1, stable=True)[:, :k]
                scores[r0:r0 + m] = torch.gather(s, 1, order)
                ids[r0:r0 + m] = torch.gather(i, 1, order)
                # listed -> it reached the floor; not listed with every row >= floor listed (c <= k + 1) -> it did not;
                # otherwise more than k rows tie with or beat it: its fp64 self dot product decides
                qd = q.to(torch.float64)
                self_dot = (qd * qd).sum(dim=1)
                reached = found | ((c > k + 1) & (self_dot >= float(floor)))
                counts[r0:r0 + m] = c - reached.to(torch.int64)
        return scores, ids, counts

    def last_filter(self) -> dict:
        """Path and allowed-row count of the last filtered search on this index (``mrag_index_last_filter``):
        ``{"path": "mask" | "compact", "allowed": m}``."""
        p, m = C.c_int(0), C.c_int64(0)
        N.check(self._lib.mrag_index_last_filter(self._h, C.byref(p), C.byref(m)))
        return {"path": _FILTER_NAMES[p.value], "allowed": m.value}

    def search_sets(self, queries, k: int, sets, set_of=None, normalize: Optional[bool] = None) -> Tuple[np.ndarray, np.ndarray]:
        """:meth:`search` with ``allow=`` for a batch of questions that each have their own allow-set, in one call
        (``mrag_index_search_sets``) -> (scores [nq,k] fp32, ids [nq,k] int64), numpy.

        ``sets`` is a sequence of bool masks over the ``len(self)`` rows or of row-position arrays (:func:`pack_sets`), and
        question q searches ``sets[set_of[q]]``; ``set_of``
        defaults to one set per question when there are as many sets as questions.  Per question: the top-k of its
        set's rows, (score desc, row asc), (-inf, -1) past the set's size.  Sets of up to 8 192 rows are gathered and
        scored by one scan launch for the whole batch; a larger set is one filtered search over all of its questions
        (:meth:`last_sets`, :meth:`last_filter`).  Host queries only."""
        norm = self._norm(normalize)
        k = _check_k(k, 256)
        keep, ptr, nq, dt, is_dev = _as_buffer(queries, self.dim)
        if is_dev:
            raise ValueError("search_sets takes host queries")
        set_ptr, set_rows = pack_sets(sets, len(self))
        n_sets = set_ptr.shape[0] - 1
        if set_of is None:
            if n_sets != nq:
                raise ValueError(f"{n_sets} sets for {nq} questions: pass set_of")
            set_of = np.arange(nq, dtype=np.int32)
        so = np.asarray(set_of)
        if so.ndim != 1 or so.shape[0] != nq or not (np.issubdtype(so.dtype, np.integer) or so.size == 0):
            raise ValueError(f"set_of must hold one set index per question ({nq}), got shape {so.shape} dtype {so.dtype}")
        if so.size and (int(so.min()) < 0 or int(so.max()) >= n_sets):
            raise ValueError(f"set_of must lie in [0, {n_sets}), got [{int(so.min())}, {int(so.max())}]")
        so = np.ascontiguousarray(so, dtype=np.int32)
        sc = np.empty((nq, k), dtype=np.float32)
        ids = np.empty((nq, k), dtype=np.int64)
        N.check(self._lib.mrag_index_search_sets(self._h, ptr, nq, dt, norm, k, n_sets, set_ptr.ctypes.data,
                                                 set_rows.ctypes.data, so.ctypes.data, sc.ctypes.data, ids.ctypes.data, None))
        del keep
        return sc, ids

    def last_sets(self) -> dict:
        """What the last :meth:`search_sets` did (``mrag_index_last_sets``): ``{"scanned": questions served by the scan,
        "routed": questions served by filtered searches, "descriptors": scan descriptors launched}``."""
        return self._last_record(self._lib.mrag_index_last_sets, "scanned", "routed", "descriptors")

    def search_groups(self, queries, k: int, group_ptr=None, sizes=None, allow=None, normalize: Optional[bool] = None,
                      stream=None, out=None, return_which: bool = False):
        """:meth:`search` for questions that each come as several query vectors (the question and its expansions), merged
        per row with the maximum on the device (``mrag_index_search_groups``) -> (scores [n_groups,k] fp32, ids
        [n_groups,k] int64), with ``return_which=True`` also which [n_groups,k] int32.

        Question g owns the rows ``group_ptr[g] .. group_ptr[g+1]`` of ``queries`` (``group_ptr``: n_groups + 1
        non-decreasing integers from 0 to ``len(queries)``); ``sizes``, the number of queries of every question, is
        accepted instead (:func:`group_ptr_of`).  Per question: a row scores the largest of its scores under the
        question's queries, and the result is the top-k of those in (score desc, id asc) order -- bit for bit the merge
        of the per-query :meth:`search` results.  ``which`` is the position inside the question of the query that gave
        the kept score (the lowest among equals); slots past the distinct rows found are (-inf, -1, -1), and so is the
        row of a question without queries.  ``1 <= k <= 256`` and at most 4096 // k queries per question.

        Host queries give numpy results; CUDA tensors give CUDA tensors written on ``stream`` (default: torch's current
        stream); ``out=(scores, ids)`` or ``(scores, ids, which)`` reuses buffers.  ``allow`` is one allow-set for the
        whole call, as in :meth:`search` (packed on the host).  :meth:`last_groups` tells what the call did.  Exact
        precision only; the fp8 scan copy, the sharded indexes and ``IVFFlatIndex`` have no grouped search."""
        norm = self._norm(normalize)
        k = _check_k(k, 256)
        keep, ptr, nq, dt, is_dev = _as_buffer(queries, self.dim)
        gp = group_ptr_of(group_ptr, sizes, nq)
        n_groups = gp.shape[0] - 1
        n, abits, aptr = 0, None, None
        if allow is not None:
            n = len(self)
            abits = np.ascontiguousarray(allow_bits(allow, n))
            aptr = abits.ctypes.data
        which, wptr = _third_output(out, return_which, "which", (n_groups, k), keep, is_dev)

        def call(sc, ids, out_dev, st):
            return self._lib.mrag_index_search_groups(self._h, ptr, nq, dt, norm, is_dev, k, n_groups, gp.ctypes.data, aptr, n,
                                                      N.ALLOW_BITS32, sc, ids, wptr, out_dev, st)
        sc, ids = _run_search(call, keep, n_groups, k, is_dev, self.device, stream, bool(is_dev),
                              None if out is None else (out[0], out[1]))
        del abits
        return (sc, ids, which) if return_which else (sc, ids)

    def last_groups(self) -> dict:
        """What the last :meth:`search_groups` did (``mrag_index_last_groups``): ``{"queries": query vectors searched,
        "groups": questions merged, "max_entries": queries x k of the largest question}``."""
        return self._last_record(self._lib.mrag_index_last_groups, "queries", "groups", "max_entries")

    def set_row_keys(self, keys):
        """One int32 key per stored row, ``0 <= key < 2**31`` (``mrag_index_set_row_keys``): a 1-D integer array of
        ``len(self)`` entries, numpy or a CUDA int32 tensor; :func:`row_keys_of` makes one from any hashable per row.
        ``None`` clears the keys.  Rows added afterwards have no key: set the keys again before the next
        :meth:`search_collapsed`."""
        if keys is None:
            N.check(self._lib.mrag_index_set_row_keys(self._h, None, 0, 0))
            return
        if _is_torch(keys) and keys.is_cuda:
            import torch
            if keys.dim() != 1 or keys.dtype != torch.int32:
                raise ValueError(f"device keys must be a 1-D int32 tensor, got {tuple(keys.shape)} {keys.dtype}")
            t = keys.contiguous()
            torch.cuda.current_stream(t.device).synchronize()      # the call copies them back on its own
            N.check(self._lib.mrag_index_set_row_keys(self._h, t.data_ptr(), t.shape[0], 1))
            return
        a = np.asarray(keys.numpy() if _is_torch(keys) else keys)
        if a.ndim != 1 or a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) or a.size == 0):
            raise ValueError(f"keys must be 1-D integers, got shape {a.shape} dtype {a.dtype}")
        if a.size and (int(a.min()) < 0 or int(a.max()) > 2 ** 31 - 1):
            raise ValueError(f"keys must lie in [0, 2**31), got [{int(a.min())}, {int(a.max())}]")
        a = np.ascontiguousarray(a, dtype=np.int32)
        N.check(self._lib.mrag_index_set_row_keys(self._h, a.ctypes.data, a.shape[0], 0))

    def search_collapsed(self, queries, k: int, scan_k: Optional[int] = None, normalize: Optional[bool] = None, stream=None,
                         out=None, return_keys: bool = True):
        """:meth:`search` with one hit per row key (``mrag_index_search_collapsed``; :meth:`set_row_keys` first) ->
        (scores [nq,k] fp32, ids [nq,k] int64, keys [nq,k] int32), without the keys when ``return_keys=False``.

        A key scores what its best row scores and is represented by the first of its rows in (score desc, row asc) order;
        the result is the top-k keys in that order of their representatives, exactly: hits carry the representative's
        score and id and the key, slots past the distinct keys are (-inf, -1, -1).  With all keys distinct scores and
        ids are those of :meth:`search`.  ``1 <= k <= 256``.

        ``scan_k`` (``k .. 256``; None: :func:`collapse_scan_k`) is the depth of the one search that all queries share;
        a query that did not meet k keys in it is searched again alone, over the rows of the keys it has not found, until
        it has (:meth:`last_collapsed` counts those).  Host queries give numpy results; CUDA tensors give CUDA tensors
        written on ``stream`` (default: torch's current stream), and the call waits for that stream at least once either
        way; ``out=(scores, ids, keys)`` (or ``(scores, ids)`` with ``return_keys=False``) reuses buffers.  Exact
        precision only; the fp8 scan copy, the sharded indexes and ``IVFFlatIndex`` have no collapsed search."""
        norm = self._norm(normalize)
        k = _check_k(k, 256)
        if scan_k is None:
            scan = 0
        else:
            scan = _check_k(scan_k, 256)
            if scan < k:
                raise ValueError(f"scan_k must lie in [k, 256] = [{k}, 256], got {scan_k!r}")
        keep, ptr, nq, dt, is_dev = _as_buffer(queries, self.dim)
        keys, kptr = _third_output(out, return_keys, "keys", (nq, k), keep, is_dev)

        def call(sc, ids, out_dev, st):
            return self._lib.mrag_index_search_collapsed(self._h, ptr, nq, dt, norm, is_dev, k, scan, sc, ids, kptr, out_dev, st)
        sc, ids = _run_search(call, keep, nq, k, is_dev, self.device, stream, bool(is_dev),
                              None if out is None else (out[0], out[1]))
        return (sc, ids, keys) if return_keys else (sc, ids)

    def last_collapsed(self) -> dict:
        """What the last :meth:`search_collapsed` did (``mrag_index_last_collapsed``): ``{"scan_k": the depth it used,
        "redone_queries": queries incomplete after the shared search, "redo_rounds": filtered searches run for them in
        all, "max_rows_per_key", "distinct_keys": of the keys it searched under}``."""
        a = C.c_int(0)
        b, c, d, e = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        N.check(self._lib.mrag_index_last_collapsed(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e)))
        return {"scan_k": a.value, "redone_queries": b.value, "redo_rounds": c.value, "max_rows_per_key": d.value,
                "distinct_keys": e.value}

    def expand_neighbors(self, seeds, window: int, m: Optional[int] = None, decay=None, return_from: bool = False, stream=None,
                         out=None):
        """The rows around each question's seed rows inside the seeds' own documents (``mrag_index_expand_neighbors``;
        :meth:`set_row_keys` first) -> (scores [nq,m] fp32, ids [nq,m] int64), with ``return_from=True`` also
        (dist [nq,m] int32, seed [nq,m] int32).

        ``seeds`` is [nq, s] int64 global ids, numpy or a CUDA tensor -- for example the leading columns of a
        :meth:`search` result; an id of -1 or outside the index is skipped.  The *run* of a row is the maximal interval
        of consecutive rows with its key, and a seed row r reaches the rows of its run within ``window`` of r.  Every
        distinct reached row c gets ``dist`` = its smallest distance to a seed that reaches it, ``seed`` = the lowest
        seed position (column) at that distance, and the score ``decay[dist]``; the rows come ordered by (dist asc, seed
        position asc, row asc), the first ``m`` of them, then (-inf, -1, -1, -1).  ``decay`` (``window + 1`` finite,
        non-increasing values, a host array) defaults to :func:`reference_decay` as fp32; ``m`` defaults to
        ``s * (2 * window + 1)``, at most 4096.  ``window <= 16``, ``s <= 256``, ``s * (2 * window + 1) <= 4096``.

        Host seeds give numpy results after one synchronisation; CUDA seeds give CUDA tensors written by one launch on
        ``stream`` (default: torch's current stream) with no synchronisation; ``out=(scores, ids)`` or ``(scores, ids,
        dist, seed)`` reuses buffers.  The sharded indexes and ``IVFFlatIndex`` have no neighbour expansion."""
        if isinstance(window, (bool, np.bool_)) or not isinstance(window, numbers.Integral) or not 0 <= int(window) <= NEIGHBORS_MAX_WINDOW:
            raise ValueError(f"window must be an integer in [0, {NEIGHBORS_MAX_WINDOW}], got {window!r}")
        window = int(window)
        is_dev = int(_is_torch(seeds) and seeds.is_cuda)
        if is_dev:
            import torch
            if seeds.dim() != 2 or seeds.dtype != torch.int64:
                raise ValueError(f"device seeds must be a 2-D int64 tensor, got {tuple(seeds.shape)} {seeds.dtype}")
            if seeds.device.index != self.device:
                raise ValueError(f"seeds are on {seeds.device}, the index on cuda:{self.device}")
            keep = seeds.contiguous()
            sptr = keep.data_ptr()
        else:
            a = np.asarray(seeds.numpy() if _is_torch(seeds) else seeds)
            if a.ndim != 2 or a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) or a.size == 0):
                raise ValueError(f"seeds must be 2-D integers, got shape {a.shape} dtype {a.dtype}")
            keep = np.ascontiguousarray(a, dtype=np.int64)
            sptr = keep.ctypes.data
        nq, s = int(keep.shape[0]), int(keep.shape[1])
        if s > NEIGHBORS_MAX_SEEDS or s * (2 * window + 1) > NEIGHBORS_MAX_ENTRIES:
            raise ValueError(f"{s} seeds per question at window {window}: at most {NEIGHBORS_MAX_SEEDS} seeds and "
                             f"{NEIGHBORS_MAX_ENTRIES} entries = seeds * (2 * window + 1)")
        m = max(1, min(NEIGHBORS_MAX_ENTRIES, s * (2 * window + 1))) if m is None else _check_k(m, NEIGHBORS_MAX_ENTRIES)
        dk = reference_decay(window).astype(np.float32) if decay is None else np.ascontiguousarray(decay, dtype=np.float32).reshape(-1)
        if dk.shape[0] != window + 1:
            raise ValueError(f"decay must hold window + 1 = {window + 1} values, got {dk.shape[0]}")
        if not np.isfinite(dk).all() or (np.diff(dk) > 0).any():
            raise ValueError("decay must be finite and must not increase")
        if out is not None and len(out) not in (2, 4):
            raise ValueError("out must be (scores, ids) or (scores, ids, dist, seed)")
        if out is not None and return_from and len(out) != 4:
            raise ValueError("return_from=True needs out=(scores, ids, dist, seed)")
        extra = [None, None]
        if out is not None and len(out) == 4:
            extra = [out[2], out[3]]
        elif return_from and is_dev:
            import torch
            extra = [torch.empty((nq, m), dtype=torch.int32, device=keep.device) for _ in range(2)]
        elif return_from:
            extra = [np.empty((nq, m), dtype=np.int32) for _ in range(2)]
        eptr = [None if x is None else (x.data_ptr() if is_dev else x.ctypes.data) for x in extra]

        def call(sc, ids, out_dev, st):
            return self._lib.mrag_index_expand_neighbors(self._h, sptr if nq * s else None, nq, s, is_dev, window, dk.ctypes.data, m,
                                                         sc, ids, eptr[0], eptr[1], out_dev, st)
        sc, ids = _run_search(call, keep, nq, m, is_dev, self.device, stream, bool(is_dev),
                              None if out is None else (out[0], out[1]))
        return (sc, ids, extra[0], extra[1]) if return_from else (sc, ids)

    def last_neighbors(self) -> dict:
        """What the last :meth:`expand_neighbors` did (``mrag_index_last_neighbors``): ``{"questions", "max_entries": seeds
        per question x (2 x window + 1), "window"}``."""
        return self._last_record(self._lib.mrag_index_last_neighbors, "questions", "max_entries", "window")

    def last_fp8(self) -> dict:
        """Refine pool and regime of the last fp8 search on this index (``mrag_index_last_fp8``):
        ``{"refine": r, "regime": "batch" | "stream"}``."""
        r, g = C.c_int(0), C.c_int(0)
        N.check(self._lib.mrag_index_last_fp8(self._h, C.byref(r), C.byref(g)))
        return {"refine": r.value, "regime": _FP8_REGIMES[g.value]}

    def max_k(self, nq: int = 1) -> int:
        """Largest ``k`` :meth:`search` serves (``mrag_index_max_k``); above it the library raises
        MRAG_ERR_UNSUPPORTED, it never clamps."""
        out = C.c_int(0)
        N.check(self._lib.mrag_index_max_k(int(nq), C.byref(out)))
        return out.value

    def last_wide_redone(self) -> int:
        """Queries the last 64 < k <= 256 batch search redid through the streaming kernel (``mrag_index_last_wide_redone``)."""
        out = C.c_int64(0)
        N.check(self._lib.mrag_index_last_wide_redone(C.byref(out)))
        return out.value

    def score_rows(self, query, row_ids, normalize: Optional[bool] = None) -> np.ndarray:
        """<query, stored row i> for every listed row (``mrag_index_score_rows``): the re-ranker's
        candidate lookup by row id.  Ids outside the index score 0.0."""
        norm = self._norm(normalize)
        q = np.ascontiguousarray(np.asarray(query, dtype=np.float32).reshape(-1))
        if q.shape[0] != self.dim:
            raise ValueError(f"query has dim {q.shape[0]}, index has {self.dim}")
        ids = np.ascontiguousarray(row_ids, dtype=np.int64).reshape(-1)
        out = np.empty(ids.shape[0], dtype=np.float32)
        N.check(self._lib.mrag_index_score_rows(self._h, q.ctypes.data, N.MRAG_F32, norm, ids.ctypes.data,
                                                ids.shape[0], out.ctypes.data, None))
        return out

    def score_rows_batch(self, queries, row_ids, normalize: Optional[bool] = None):
        """:meth:`score_rows` for a batch of questions in one call (``mrag_index_score_rows_batch``): ``queries`` is
        ``[nq, dim]``, ``row_ids`` either a sequence of nq int arrays -- the result is then a list of nq float32 arrays --
        or a pair ``(row_ptr int64 [nq + 1], flat_ids)`` -- the result is then ``(row_ptr, flat_scores)``.  Question g's
        scores are bit for bit ``score_rows(queries[g], ids of g)``.  No library call for nq = 0 or no entries."""
        norm = self._norm(normalize)
        q = np.ascontiguousarray(np.asarray(queries, dtype=np.float32))
        if q.ndim == 1 and q.shape[0] == 0:
            q = q.reshape(0, self.dim)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError(f"queries have shape {q.shape}, index has dim {self.dim}")
        nq = q.shape[0]
        csr = isinstance(row_ids, tuple) and len(row_ids) == 2
        if csr:
            ptr = np.ascontiguousarray(row_ids[0], dtype=np.int64).reshape(-1)
            ids = np.ascontiguousarray(row_ids[1], dtype=np.int64).reshape(-1)
            if ptr.shape[0] != nq + 1:
                raise ValueError(f"row_ptr has {ptr.shape[0]} entries for {nq} queries (expected {nq + 1})")
            if ptr[0] != 0 or (np.diff(ptr) < 0).any() or ptr[-1] != ids.shape[0]:
                raise ValueError("row_ptr must start at 0, never decrease and end at the number of ids")
        else:
            lists = [np.asarray(r, dtype=np.int64).reshape(-1) for r in row_ids]
            if len(lists) != nq:
                raise ValueError(f"{len(lists)} id lists for {nq} queries")
            ptr = np.zeros(nq + 1, dtype=np.int64)
            np.cumsum([r.shape[0] for r in lists], out=ptr[1:])
            ids = np.ascontiguousarray(np.concatenate(lists)) if lists else np.zeros(0, dtype=np.int64)
        out = np.empty(ids.shape[0], dtype=np.float32)
        if nq and ids.shape[0]:
            N.check(self._lib.mrag_index_score_rows_batch(self._h, q.ctypes.data, N.MRAG_F32, norm, nq,
                                                          ptr.ctypes.data, ids.ctypes.data, out.ctypes.data, None))
        if csr:
            return ptr, out
        return [out[ptr[g]:ptr[g + 1]] for g in range(nq)]

    def stored_bits(self) -> np.ndarray:
        """The stored rows as their 16-bit patterns ([n, dim] uint16, fp16 or bf16 per ``dtype``):
        what the embedding cache keeps, so that a warm start re-adds the exact bits K1 produced."""
        r = self.rows()
        if self.dtype == "f16":
            return r.astype(np.float16).view(np.uint16)       # exact: every stored value is an fp16 value
        return (r.view(np.uint32) >> 16).astype(np.uint16)     # exact: low 16 bits of a widened bf16 are zero

    def add_stored_bits(self, bits: np.ndarray):
        """Append rows given as the storage dtype's bit patterns, verbatim (no normalise, no rounding)."""
        bits = np.ascontiguousarray(bits, dtype=np.uint16)
        if self.dtype == "f16":
            self.add(bits.view(np.float16), normalize=False)
        else:
            import torch
            self.add(torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16), normalize=False)

    def measure_clock(self, enable: bool = True):
        """Ask the batch kernel's workgroup 0 to stamp s_memtime / s_memrealtime (``mrag_index_measure_clock``)."""
        N.check(self._lib.mrag_index_measure_clock(self._h, int(bool(enable))))

    def last_clock_ghz(self) -> float:
        """Held shader clock during the last batch-kernel search (``mrag_index_last_clock``)."""
        g = C.c_float(0)
        N.check(self._lib.mrag_index_last_clock(self._h, C.byref(g)))
        return g.value

    def last_timing_ms(self) -> Tuple[float, float]:
        """(fused similarity+top-k kernel ms, whole search ms) of the last search, from
        hipEvents recorded on the launch stream."""
        g, t = C.c_float(0), C.c_float(0)
        N.check(self._lib.mrag_index_last_timing(self._h, C.byref(g), C.byref(t)))
        return g.value, t.value


def cosine_f64(query, cands, device: int = 0) -> np.ndarray:
    """One query against n candidates, fp64 on the GPU -- the arithmetic of
    ``DenseReranker._cosine`` (retrieval_backend.py:192-197) for every candidate at once."""
    q = np.ascontiguousarray(query, dtype=np.float64).reshape(-1)
    c = np.ascontiguousarray(cands, dtype=np.float64)
    if c.ndim != 2 or c.shape[1] != q.shape[0]:
        raise ValueError("dimension mismatch")
    out = np.empty(c.shape[0], dtype=np.float64)
    N.check(N.load().mrag_cosine_f64(device, q.ctypes.data, c.ctypes.data, c.shape[0], c.shape[1],
                                     out.ctypes.data, 0, None))
    return out


def topk_merge(scores: np.ndarray, ids: np.ndarray, nthreads: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """Host merge of per-shard partial top-k: scores/ids [nparts, nq, k] -> [nq, k]
    ordered by (score desc, id asc).  Runs on the CPU (C++ threads)."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    i = np.ascontiguousarray(ids, dtype=np.int64)
    if s.ndim != 3 or s.shape != i.shape:
        raise ValueError("expected matching [nparts, nq, k] arrays")
    nparts, nq, k = s.shape
    os_, oi = np.empty((nq, k), dtype=np.float32), np.empty((nq, k), dtype=np.int64)
    N.check(N.load().mrag_topk_merge(s.ctypes.data, i.ctypes.data, nparts, nq, k, os_.ctypes.data,
                                     oi.ctypes.data, int(nthreads)))
    return os_, oi


def topk_merge_device(scores, ids, out_scores=None, out_ids=None):
    """The same merge on the GPU (``mrag_topk_merge_device``) for gathered partial top-k that
    already sits in HBM: ``scores`` float32 / ``ids`` int64 CUDA tensors [nparts, nq, k] (each
    part sorted, empties last) -> CUDA tensors [nq, k].  Asynchronous on the current stream."""
    import torch
    if not (torch.is_tensor(scores) and scores.is_cuda and torch.is_tensor(ids) and ids.is_cuda):
        raise ValueError("topk_merge_device expects CUDA tensors (use topk_merge for host arrays)")
    if scores.dim() != 3 or scores.shape != ids.shape or scores.dtype != torch.float32 or ids.dtype != torch.int64:
        raise ValueError("expected matching [nparts, nq, k] float32 / int64 tensors")
    scores, ids = scores.contiguous(), ids.contiguous()
    nparts, nq, k = scores.shape
    dev = scores.device
    if out_scores is None:
        out_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
    if out_ids is None:
        out_ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    N.check(N.load().mrag_topk_merge_device(dev.index or 0, scores.data_ptr(), ids.data_ptr(), nparts, nq, k,
                                            out_scores.data_ptr(), out_ids.data_ptr(), stream))
    return out_scores, out_ids


def pack_partial_device(scores, ids, id_base: int, out_words=None, bad_flag=None):
    """[Q,k] fp32 scores + int64 global ids (CUDA) -> the exchange's packed int64 words in ONE kernel (``mrag_pack_partial_device``;
    the torch form in ``sharded.pack_partial`` is ~8 elementwise kernels).  ``bad_flag``: int32 CUDA tensor [1], OR'ed with 1 when
    an id does not fit 32 bits above ``id_base``.  Asynchronous on the current stream."""
    import torch
    scores, ids = scores.contiguous(), ids.contiguous()
    if out_words is None:
        out_words = torch.empty(scores.shape, dtype=torch.int64, device=scores.device)
    stream = torch.cuda.current_stream(scores.device).cuda_stream
    N.check(N.load().mrag_pack_partial_device(scores.device.index or 0, scores.data_ptr(), ids.data_ptr(), scores.numel(), int(id_base),
                                              out_words.data_ptr(), bad_flag.data_ptr() if bad_flag is not None else None, stream))
    return out_words


def topk_merge_packed_device(words, bases, out_scores=None, out_ids=None):
    """Merge of the GATHERED packed words [nparts, nq, k] (int64 CUDA) with the parts' first global rows ``bases`` (int64 CUDA
    [nparts]) -> CUDA tensors [nq, k] (``mrag_topk_merge_packed_device``): no unpack pass over the gathered buffer."""
    import torch
    words = words.contiguous()
    nparts, nq, k = words.shape
    dev = words.device
    if out_scores is None:
        out_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
    if out_ids is None:
        out_ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    N.check(N.load().mrag_topk_merge_packed_device(dev.index or 0, words.data_ptr(), bases.contiguous().data_ptr(), nparts, nq, k,
                                                   out_scores.data_ptr(), out_ids.data_ptr(), stream))
    return out_scores, out_ids


class IVFFlatIndex:
    """IVF-flat index on one GPU (BASELINE.json config 5): nlist spherical-k-means lists, every
    search probes the ``nprobe`` best lists and scans them exactly.  Same id / tie-break
    conventions as :class:`DenseIndex`."""

    def __init__(self, dim: int, nlist: int, metric: str = "cosine", dtype: str = "f16", device: int = 0,
                 fp8_scan: bool = False):
        self._lib = N.load()
        self.dim, self.nlist, self.metric, self.dtype, self.device = int(dim), int(nlist), metric, dtype, int(device)
        h = C.c_uint64(0)
        N.check(self._lib.mrag_ivf_create(self.dim, self.nlist, N.METRIC_COSINE if metric == "cosine" else N.METRIC_IP,
                                          N.MRAG_F16 if dtype == "f16" else N.MRAG_BF16, self.device, C.byref(h)))
        self._h = h
        self.id_base = 0
        if fp8_scan:
            self.enable_fp8()

    def enable_fp8(self):
        """Keep an fp8 (e4m3fn) copy of the regrouped rows for ``search(precision="fp8")`` (``mrag_ivf_enable_fp8``):
        built from the rows already stored, then rebuilt with every regroup (the first search after an add).  Costs
        ``round_up(dim, 128)`` bytes per stored position.  Cosine indexes only; idempotent."""
        N.check(self._lib.mrag_ivf_enable_fp8(self._h))

    def rows_fp8(self, row0: int = 0, n: Optional[int] = None) -> np.ndarray:
        """The fp8 copy of the original rows ``[row0, row0 + n)``, in insertion order, as raw e4m3fn bytes
        ([n, dim] uint8); regroups first when rows were added since the last search."""
        n = len(self) - row0 if n is None else n
        out = np.empty((n, self.dim), dtype=np.uint8)
        N.check(self._lib.mrag_ivf_get_rows_fp8(self._h, int(row0), int(n), out.ctypes.data, 0, None))
        return out

    def last_fp8(self) -> dict:
        """Refine pool of the last fp8 search on this index (``mrag_ivf_last_fp8``): ``{"refine": r}``."""
        r = C.c_int(0)
        N.check(self._lib.mrag_ivf_last_fp8(self._h, C.byref(r)))
        return {"refine": r.value}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.mrag_ivf_destroy(self._h)
            self._h = C.c_uint64(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        n = C.c_int64(0)
        N.check(self._lib.mrag_ivf_size(self._h, C.byref(n)))
        return n.value

    def _norm(self, normalize):
        return int(bool(self.metric == "cosine" if normalize is None else normalize))

    def train(self, rows, iters: int = 10, seed: int = 0, normalize: Optional[bool] = None):
        keep, ptr, n, dt, is_dev = _as_buffer(rows, self.dim)
        N.check(self._lib.mrag_ivf_train(self._h, ptr, n, dt, self._norm(normalize), is_dev, int(iters), int(seed), None))

    def set_centroids(self, centroids, normalize: Optional[bool] = None):
        keep, ptr, n, dt, is_dev = _as_buffer(centroids, self.dim)
        if n != self.nlist:
            raise ValueError(f"expected {self.nlist} centroids, got {n}")
        N.check(self._lib.mrag_ivf_set_centroids(self._h, ptr, dt, self._norm(normalize), is_dev, None))

    def centroids(self) -> np.ndarray:
        out = np.empty((self.nlist, self.dim), dtype=np.float32)
        N.check(self._lib.mrag_ivf_get_centroids(self._h, out.ctypes.data, 0, None))
        return out

    def add(self, rows, normalize: Optional[bool] = None):
        keep, ptr, n, dt, is_dev = _as_buffer(rows, self.dim)
        N.check(self._lib.mrag_ivf_add(self._h, ptr, n, dt, self._norm(normalize), is_dev, None))

    def set_id_base(self, base: int):
        N.check(self._lib.mrag_ivf_set_id_base(self._h, int(base)))
        self.id_base = int(base)

    def assignments(self) -> np.ndarray:
        out = np.empty(len(self), dtype=np.int32)
        N.check(self._lib.mrag_ivf_get_assignments(self._h, out.ctypes.data, 0, None))
        return out

    def last_timing(self) -> dict:
        """Device timing of the last search: list-scan kernel ms, whole-search ms, rows the scan streamed,
        workgroups (``mrag_ivf_last_timing``)."""
        g, t, rows, nwg = C.c_float(0), C.c_float(0), C.c_int64(0), C.c_int(0)
        N.check(self._lib.mrag_ivf_last_timing(self._h, C.byref(g), C.byref(t), C.byref(rows), C.byref(nwg)))
        return {"scan_ms": g.value, "total_ms": t.value, "scanned_rows": rows.value, "n_wg": nwg.value}

    def search(self, queries, k: int, nprobe: int, normalize: Optional[bool] = None, allow=None, filter_path: str = "auto",
               list_allowed=None, stream=None, precision: str = "exact", refine: Optional[int] = None, out=None):
        """-> (scores [nq,k], ids [nq,k]); host queries give numpy arrays (complete on return), CUDA tensors give CUDA
        tensors filled asynchronously on ``stream`` (default: the current torch stream), like any torch op;
        ``out=(scores, ids)`` reuses caller tensors of a plain or fp8 search.  ``nprobe``: 1..256, or ``nlist``
        (exhaustive).

        ``allow`` restricts the search to some rows (``mrag_ivf_search_filtered``), in the forms
        :meth:`DenseIndex.search` takes: a bool / uint8 mask over the ``len(self)`` local rows (numpy, or a torch tensor
        on the host or this index's device) or a host array of row positions.  ``filter_path``: "probe" (every query
        probes its ``nprobe`` best lists among those holding an allowed row), "exact" (filtered brute force) or "auto".
        ``list_allowed``: allowed rows per list (int32 [nlist], on the host for a host ``allow``, on the device for a
        device one) deciding which lists are live instead of this index's own counts (sharded search: the global
        counts).  See :meth:`last_filter`.

        ``precision="fp8"`` (index built with ``fp8_scan=True`` or :meth:`enable_fp8`; ``1 <= k <= 64``, at most 256
        probed lists): the same lists are probed, their rows are scanned in the fp8 copy, and the ``refine`` best rows per
        query (``k <= refine <= 64``; None: :func:`fp8_default_refine`) are re-scored exactly against the 16-bit rows.
        The scores are exact, the row set is approximate (measured recall in DESIGN.md); a query whose probed lists hold
        at most ``refine`` rows gets the exact search's answer.  It does not combine with ``allow``."""
        fp8, r = _check_precision(precision, refine, allow)
        if allow is not None:
            return self._search_filtered(queries, k, nprobe, normalize, allow, filter_path, list_allowed, stream)
        keep, ptr, nq, dt, is_dev = _as_buffer(queries, self.dim)
        norm = self._norm(normalize)
        if fp8:
            def call(sc, ids, out_dev, st):
                return self._lib.mrag_ivf_search_fp8(self._h, ptr, nq, dt, norm, is_dev, int(nprobe), int(k), r, sc, ids, out_dev, st)
        else:
            def call(sc, ids, out_dev, st):
                return self._lib.mrag_ivf_search(self._h, ptr, nq, dt, norm, is_dev, int(nprobe), int(k), sc, ids, out_dev, st)
        return _run_search(call, keep, nq, k, is_dev, self.device, stream, bool(is_dev), out)

    @staticmethod
    def _check_nprobe(nprobe) -> int:
        if isinstance(nprobe, (bool, np.bool_)) or not isinstance(nprobe, numbers.Integral) or int(nprobe) < 1:
            raise ValueError(f"nprobe must be a positive integer, got {nprobe!r}")
        return int(nprobe)

    def _exclude_buffer(self, exclude, nq: int):
        """-> (keepalive, pointer, is_device): one excluded local row per query (int64 [nq], -1 = none)."""
        if _is_torch(exclude) and exclude.is_cuda:
            import torch
            if exclude.dim() != 1 or exclude.shape[0] != nq:
                raise ValueError(f"exclude must be 1-D with one row per query ({nq}), got shape {tuple(exclude.shape)}")
            if exclude.dtype != torch.int64:
                raise ValueError(f"a device exclude must be int64, got {exclude.dtype}")
            if exclude.device.index != self.device:
                raise ValueError(f"exclude is on {exclude.device}, the index on cuda:{self.device}")
            t = exclude.contiguous()
            return t, t.data_ptr(), 1
        a = exclude.cpu().numpy() if _is_torch(exclude) else np.asarray(exclude)
        if a.ndim != 1 or a.shape[0] != nq:
            raise ValueError(f"exclude must be 1-D with one row per query ({nq}), got shape {a.shape}")
        if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"exclude must hold integer row positions (-1 = none), got dtype {a.dtype}")
        if a.size and int(a.min()) < -1:
            raise ValueError(f"exclude rows must be >= -1, got {int(a.min())}")
        a = np.ascontiguousarray(a, dtype=np.int64)
        return a, a.ctypes.data, 0

    def range_search(self, queries, min_score: float, k: int, nprobe: int, normalize: Optional[bool] = None, exclude=None,
                     stream=None, out=None):
        """Rows of the probed lists scoring >= ``min_score`` (``mrag_ivf_search_range``) -> (scores [nq,k] fp32, ids [nq,k]
        int64, counts [nq] int64).

        Per query, over the rows of its ``nprobe`` probed lists only (the lists :meth:`search` probes), with c = the number
        of those rows scoring >= ``min_score`` (inclusive; the floor is the smallest float32 >= ``min_score``, see
        :func:`range_floor`): the best ``min(k, c)`` of them, (score desc, row asc), then (-inf, -1) slots; ``counts[q] = c``
        exactly, so a query is truncated when ``counts[q] > k``.  ``counts`` is a lower bound of
        :meth:`DenseIndex.range_search`'s and equal to it when every list is probed.  Scores are the ones :meth:`search`
        returns.  ``min_score`` must be finite, ``1 <= k <= 256``, ``nprobe >= 1`` (``ValueError`` otherwise, before any
        GPU work).  ``exclude``: one local row (before ``id_base``) per query, int64 [nq], -1 for none, on the host or on
        this index's device; that row is neither listed nor counted, rows holding the same values stay.  Host queries give
        numpy arrays; CUDA tensors give CUDA tensors written on ``stream``; ``out=(scores, ids, counts)`` reuses buffers.

        The search runs in the score-segment regime only: ``nprobe = nlist > 256``, ``MRAG_IVF_SCORES_MB=0`` or segments
        beyond the score buffer raise :class:`MragError` (``MRAG_ERR_UNSUPPORTED``); no answer comes back without the
        floor applied.  There is no ``allow=`` parameter: a floor does not combine with an allow-set on this index."""
        floor = range_floor(min_score)
        k = _check_k(k, 256)
        nprobe = self._check_nprobe(nprobe)
        keep, ptr, nq, dt, is_dev = _as_buffer(queries, self.dim)
        xkeep, xptr, xdev = (None, None, 0) if exclude is None else self._exclude_buffer(exclude, nq)
        if out is not None:
            counts = out[2]
        elif is_dev:
            import torch
            counts = torch.empty(nq, dtype=torch.int64, device=keep.device)
        else:
            counts = np.empty(nq, dtype=np.int64)
        norm = self._norm(normalize)

        def call(sc, ids, out_dev, st):
            cptr = counts.data_ptr() if out_dev else counts.ctypes.data
            return self._lib.mrag_ivf_search_range(self._h, ptr, nq, dt, norm, is_dev, nprobe, k, float(floor), xptr, xdev,
                                                   sc, ids, cptr, out_dev, st)
        sc, ids = _run_search(call, keep, nq, k, is_dev, self.device, stream, bool(is_dev or xdev),
                              None if out is None else (out[0], out[1]))
        del xkeep
        return sc, ids, counts

    def self_join(self, min_score: float, nprobe: int, k: int = 64, batch: int = 65536):
        """Every stored row as a query against the rows of its ``nprobe`` probed lists, itself left out
        (``mrag_ivf_self_join``) -> CUDA tensors on this index's device (scores [n,k] fp32, ids [n,k] int64, counts [n]
        int64): row ``i``'s result is ``range_search(stored row i, min_score, k, nprobe, exclude=i)``.

        The stored 16-bit rows are the queries as they are (device to device, no renormalisation).  The row itself is
        excluded inside the selection kernel by its position, so duplicates of it stay, ``counts`` never includes it and
        ``1 <= k <= 256``.  Batches of ``batch`` rows run in order on torch's current stream; the result does not depend on
        ``batch``.  A pair of rows is found only from a side whose probed lists hold the other row."""
        import torch
        floor = range_floor(min_score)
        k = _check_k(k, 256)
        nprobe = self._check_nprobe(nprobe)
        if isinstance(batch, (bool, np.bool_)) or not isinstance(batch, numbers.Integral) or int(batch) < 1:
            raise ValueError(f"batch must be a positive integer, got {batch!r}")
        n, dev = len(self), torch.device("cuda", self.device)
        scores = torch.empty((n, k), dtype=torch.float32, device=dev)
        ids = torch.empty((n, k), dtype=torch.int64, device=dev)
        counts = torch.empty(n, dtype=torch.int64, device=dev)
        st = _stream_ptr(torch.cuda.current_stream(dev))
        b = int(batch)
        for r0 in range(0, n, b):
            m = min(b, n - r0)
            N.check(self._lib.mrag_ivf_self_join(self._h, r0, m, nprobe, k, float(floor), scores[r0:r0 + m].data_ptr(),
                                                 ids[r0:r0 + m].data_ptr(), counts[r0:r0 + m].data_ptr(), st))
        return scores, ids, counts

    def _list_allowed_buffer(self, list_allowed, adev: int):
        if list_allowed is None:
            return None, None
        if _is_torch(list_allowed) and list_allowed.is_cuda:
            import torch
            if not adev:
                raise ValueError("list_allowed is on the device, allow on the host: pass both in the same memory space")
            if list_allowed.dtype != torch.int32 or tuple(list_allowed.shape) != (self.nlist,):
                raise ValueError(f"list_allowed must be int32 [{self.nlist}], got {list_allowed.dtype} {tuple(list_allowed.shape)}")
            t = list_allowed.contiguous()
            return t, t.data_ptr()
        if adev:
            raise ValueError("list_allowed is on the host, allow on the device: pass both in the same memory space")
        a = list_allowed.cpu().numpy() if _is_torch(list_allowed) else np.asarray(list_allowed)
        if a.shape != (self.nlist,):
            raise ValueError(f"list_allowed must have {self.nlist} entries, got shape {a.shape}")
        if a.size and (int(a.min()) < 0 or int(a.max()) > np.iinfo(np.int32).max):
            raise ValueError("list_allowed counts must lie in [0, 2^31)")
        a = np.ascontiguousarray(a, dtype=np.int32)
        return a, a.ctypes.data

    def _search_filtered(self, queries, k, nprobe, normalize, allow, filter_path, list_allowed, stream):
        if filter_path not in IVF_FILTER_PATHS:
            raise ValueError(f"filter_path must be one of {sorted(IVF_FILTER_PATHS)}, got {filter_path!r}")
        n = len(self)
        akeep, aptr, afmt, adev = _allow_buffer(allow, n, self.device)
        lkeep, lptr = self._list_allowed_buffer(list_allowed, adev)
        keep, ptr, nq, dt, is_dev = _as_buffer(queries, self.dim)
        path = IVF_FILTER_PATHS[filter_path]
        norm = self._norm(normalize)

        def call(sc, ids, out_dev, st):
            return self._lib.mrag_ivf_search_filtered(self._h, ptr, nq, dt, norm, is_dev, int(nprobe), int(k), aptr, n, afmt, adev,
                                                      lptr, path, sc, ids, out_dev, st)
        return _run_search(call, keep, nq, k, is_dev, self.device, stream, bool(is_dev or adev))

    def allowed_per_list(self, allow, stream=None):
        """Allowed rows per list of an allow-set (``mrag_ivf_allowed_per_list``): int32 [nlist], a numpy array for a
        host ``allow``, a CUDA tensor (written on ``stream``) for a device one."""
        n = len(self)
        akeep, aptr, afmt, adev = _allow_buffer(allow, n, self.device)
        if adev:
            import torch
            if stream is None:
                stream = torch.cuda.current_stream(self.device)
            out = torch.empty(self.nlist, dtype=torch.int32, device=akeep.device)
            N.check(self._lib.mrag_ivf_allowed_per_list(self._h, aptr, n, afmt, 1, out.data_ptr(), 1, _stream_ptr(stream)))
            return out
        out = np.empty(self.nlist, dtype=np.int32)
        N.check(self._lib.mrag_ivf_allowed_per_list(self._h, aptr, n, afmt, 0, out.ctypes.data, 0, _stream_ptr(stream)))
        return out

    def last_filter(self) -> dict:
        """Path, allowed rows and live lists of the last filtered search on this index (``mrag_ivf_last_filter``):
        ``{"path": "probe" | "exact", "allowed": m, "live_lists": l}`` (``live_lists`` is None after path "exact")."""
        p, m, live = C.c_int(0), C.c_int64(0), C.c_int(0)
        N.check(self._lib.mrag_ivf_last_filter(self._h, C.byref(p), C.byref(m), C.byref(live)))
        return {"path": _IVF_FILTER_NAMES[p.value], "allowed": m.value, "live_lists": None if live.value < 0 else live.value}
