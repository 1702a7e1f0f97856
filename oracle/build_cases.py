"""CPU oracle and cases for the index build path: row preparation (K1) and IVF training.

TEST INFRASTRUCTURE (see ``oracle/__init__.py``).  numpy, and torch on the CPU for bf16 rounding.  The reference ships no
index, so there is nothing of the reference to pin here: PARITY UNPINNED by the reference.  What this module states is the
library's own contract, in fp64:

* ``prep_reference``: ``dense_search.l2_normalize`` (fp64 sum of squares, fp64 divide, one rounding to fp32) followed by
  one rounding to the storage type.
* ``train_picks``: the seeded choice of starting rows (splitmix64, Floyd's sampling, ascending).
* ``kmeans_step``: one Lloyd step.

Row values travel as 16-bit patterns (``uint16``) wherever bits are compared.  ``PREP_CASES`` and ``TRAIN_CASES`` are the
cases ``tests/test_gpu_build_paths.py`` runs on the device; ``tests/test_build_sensitivity.py`` shows on the CPU, with
the mutants below, what those comparisons can see.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import dense_search as ds

STORAGES = ("f16", "bf16")
SOURCES = ("f32", "f16", "bf16", "f64")
_MANT = {"f16": 10, "bf16": 7}                 # stored mantissa bits
_MIN_SUB_EXP = {"f16": -24, "bf16": -133}      # exponent of the smallest subnormal
_NP_SRC = {"f32": np.float32, "f16": np.float16, "f64": np.float64}

# the project's bar where the order of an fp64 / fp32 sum is the only legitimate difference (tests/test_gpu_bruteforce.py)
SHARE_BAR = 1e-5
MUTANT_FACTOR = 4.0

PREP_MUTANTS = ("ss_f32", "div_f32", "no_f32_step", "trunc", "flush_subnormal", "tail_out_of_norm")
TRAIN_MUTANTS = ("drop_row", "cols_ge_64", "ip_sum", "zero_empty", "ties_high")


def _torch():
    import torch
    return torch


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


# ------------------------------------------------------------------ number formats
def as_f64(x) -> np.ndarray:
    if _is_torch(x):
        return x.to(_torch().float64).numpy()
    return np.asarray(x, dtype=np.float64)


def to_source(values, src: str):
    """``values`` rounded to the source type: numpy for f32 / f16 / f64, a CPU torch tensor for bf16."""
    if src == "bf16":
        torch = _torch()
        return torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(torch.bfloat16)
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(np.asarray(values).astype(_NP_SRC[src]))


def round_bits(x32: np.ndarray, storage: str) -> np.ndarray:
    """fp32 -> storage type, round to nearest even, as bit patterns."""
    x32 = np.ascontiguousarray(x32, dtype=np.float32)
    if storage == "f16":
        with np.errstate(over="ignore"):
            return x32.astype(np.float16).view(np.uint16)
    torch = _torch()
    return torch.from_numpy(x32).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def bits_to_f64(bits: np.ndarray, storage: str) -> np.ndarray:
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if storage == "f16":
        return bits.view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def values_to_bits(vals: np.ndarray, storage: str) -> np.ndarray:
    """Storage values that were widened to fp32 (``rows()``, ``centroids()``) -> their bit patterns, exactly."""
    v = np.ascontiguousarray(vals, dtype=np.float32)
    if storage == "f16":
        return v.astype(np.float16).view(np.uint16)
    return (v.view(np.uint32) >> 16).astype(np.uint16)


def bits_to_source(bits: np.ndarray, storage: str):
    """Bit patterns as an array of the storage type (numpy fp16 / torch bf16), as ``add(normalize=False)`` takes them."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if storage == "f16":
        return bits.view(np.float16)
    torch = _torch()
    return torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16)


def _round_fmt(x64: np.ndarray, storage: str, rnd=np.rint) -> np.ndarray:
    """fp64 -> the storage format's value grid in ONE step (``rnd`` = np.rint: nearest even; np.trunc: toward zero)."""
    x64 = np.asarray(x64, dtype=np.float64)
    _, e = np.frexp(x64)
    ue = np.maximum(e - (_MANT[storage] + 1), _MIN_SUB_EXP[storage])
    return np.ldexp(rnd(np.ldexp(x64, -ue)), ue)


def ulp_diff(a_bits: np.ndarray, b_bits: np.ndarray) -> np.ndarray:
    """Signed distance in storage ulps (sign-magnitude patterns mapped to a monotone integer line)."""
    def key(b):
        b = np.asarray(b).astype(np.int32)
        return np.where(b & 0x8000, -(b & 0x7FFF), b)
    return key(a_bits) - key(b_bits)


def share_and_max(got_bits, want_bits) -> Tuple[float, int]:
    d = np.abs(ulp_diff(got_bits, want_bits))
    return float((d != 0).mean()), int(d.max())


def within_bar(got_bits, want_bits, bar: float = SHARE_BAR) -> bool:
    share, worst = share_and_max(got_bits, want_bits)
    return worst <= 1 and share <= bar


def exceeds_bar(got_bits, want_bits, bar: float = SHARE_BAR) -> bool:
    """A mutant is told apart by a clear margin: some element off by more than 1 ulp, or MUTANT_FACTOR x the share."""
    share, worst = share_and_max(got_bits, want_bits)
    return worst > 1 or share > MUTANT_FACTOR * bar


# ------------------------------------------------------------------ row preparation
def lane_order_ss(x, kernel: str, dtype=np.float64) -> np.ndarray:
    """Sum of squares per row in the order the device takes it: 64 per-lane partial sums (vector kernel: lane l owns the
    8-element chunks l, l + 64, ...; scalar kernel: elements l, l + 64, ...), then the xor butterfly 32, 16, ..., 1."""
    x = as_f64(x).astype(dtype)
    n, dim = x.shape
    part = np.zeros((n, 64), dtype=dtype)
    if kernel == "vec":
        nch = dim // 8
        for c0 in range(0, nch, 64):
            cs = np.arange(c0, min(c0 + 64, nch))
            for j in range(8):
                v = x[:, cs * 8 + j]
                part[:, :len(cs)] += v * v
    else:
        for i0 in range(0, dim, 64):
            v = x[:, i0:i0 + 64]
            part[:, :v.shape[1]] += v * v
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lanes ^ off]
    return part[:, 0].astype(np.float64)


def prep_kernel(src: str, dim: int) -> str:
    """Which device kernel a HOST source of this type and dim takes (staged copies are 16-byte aligned)."""
    ld = -(-dim // 64) * 64
    return "vec" if src == "f32" and dim % 8 == 0 and ld <= 4096 else "scalar"


def prep_reference(x, storage: str, normalize: bool, mutant: Optional[str] = None, ss: Optional[np.ndarray] = None
                   ) -> np.ndarray:
    """The stored bits of rows ``x`` ([n, dim], any source type).  ``normalize``: ``ds.l2_normalize`` then one rounding to
    the storage type; otherwise ``x`` rounded to fp32 and then to the storage type.  ``ss`` replaces the fp64 sum of
    squares (for ``lane_order_ss``); ``mutant`` is one of PREP_MUTANTS."""
    assert mutant is None or mutant in PREP_MUTANTS
    x64 = as_f64(x)
    if normalize:
        if ss is None and mutant is None:
            y32 = ds.l2_normalize(x64)
        else:
            if ss is None:
                if mutant == "ss_f32":
                    ss = lane_order_ss(x64, "scalar", np.float32)
                elif mutant == "tail_out_of_norm":
                    head = x64[:, :x64.shape[1] - x64.shape[1] % 64]
                    ss = np.einsum("ij,ij->i", head, head)
                else:
                    ss = np.einsum("ij,ij->i", x64, x64)
            nrm = np.sqrt(ss)
            nrm[~(ss > 0)] = 1.0
            if mutant == "div_f32":
                with np.errstate(over="ignore", under="ignore"):
                    y32 = x64.astype(np.float32) / nrm.astype(np.float32)[:, None]
            else:
                y64 = x64 / nrm[:, None]
                y32 = y64.astype(np.float32)
    else:
        y64 = x64
        with np.errstate(over="ignore"):
            y32 = x64.astype(np.float32)
    if mutant == "no_f32_step":
        bits = round_bits(_round_fmt(y64, storage).astype(np.float32), storage)
    elif mutant == "trunc":
        bits = round_bits(_round_fmt(y32.astype(np.float64), storage, np.trunc).astype(np.float32), storage)
    else:
        bits = round_bits(y32, storage)
    if mutant == "flush_subnormal":
        expo = 0x7C00 if storage == "f16" else 0x7F80
        bits = np.where((bits & expo) == 0, bits & 0x8000, bits).astype(np.uint16)
    return bits


# input generators ---------------------------------------------------------------------------------
def gen_gauss(n: int, dim: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal((n, dim))


def gen_edge_norms(dim: int = 100) -> np.ndarray:
    """normalize=True edges (fp32 source): a zero row, one-hot rows (first column, last column of the dimension tail),
    rows of norm 1e-20, 1e+18 and 1e+30 (their squares leave fp32's range, not fp64's), and a row whose weight sits in
    the dimension tail."""
    rng = np.random.default_rng(77)
    g = ds.l2_normalize(rng.standard_normal((4, dim))).astype(np.float64)
    rows = np.zeros((9, dim))
    rows[1, 0] = 3.5
    rows[2, dim - 1] = -0.25
    rows[3, 7] = 1e-30
    rows[4] = g[0] * 1e-20
    rows[5] = g[1] * 1e18
    rows[6] = g[2] * 1e30
    rows[7] = g[3]
    rows[7, dim - (dim % 64 or 64):] *= 8.0
    rows[8] = -rows[4]
    return rows.astype(np.float32).astype(np.float64)


def gen_subnormals(dim: int = 100) -> np.ndarray:
    """normalize=False values around fp16's subnormal range: every k x 2^-24 grid point near zero, the halfway points
    between them (ties go to even), values below half the smallest subnormal, the last subnormal and the first normal."""
    k = np.arange(0, 40, dtype=np.float64)
    v = np.concatenate([k * 2.0 ** -24, (k + 0.5) * 2.0 ** -24, (k + 0.25) * 2.0 ** -24, (k + 0.75) * 2.0 ** -24,
                        [2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 2.0 ** -26, 2.0 ** -30, 1e-12,
                         1023 * 2.0 ** -24, 1023.5 * 2.0 ** -24, 1024 * 2.0 ** -24, 1024.5 * 2.0 ** -24, 1025.5 * 2.0 ** -24]])
    v = np.concatenate([v, -v])
    n = -(-len(v) // dim)
    out = np.zeros(n * dim)
    out[:len(v)] = v
    return out.reshape(n, dim)


def _halfway_points(storage: str) -> Tuple[np.ndarray, np.ndarray]:
    """(h, m): values exactly halfway between the storage values with mantissa m and m + 1, over many binades."""
    p = _MANT[storage]
    ms = np.array([0, 1, 2, 3, 4, 5, 2 ** (p - 1) - 1, 2 ** (p - 1), 2 ** p - 3, 2 ** p - 2, 2 ** p - 1], dtype=np.float64)
    es = np.arange(-12, 15, dtype=np.float64)
    m, e = [a.reshape(-1) for a in np.meshgrid(ms, es)]
    return (2.0 ** p + m + 0.5) * 2.0 ** (e - p), m


def _pad_rows(v: np.ndarray, dim: int) -> np.ndarray:
    n = -(-len(v) // dim)
    out = np.zeros(n * dim)
    out[:len(v)] = v
    return out.reshape(n, dim)


def gen_halfway(storage: str, dim: int = 100) -> np.ndarray:
    """normalize=False fp32 values exactly halfway between two storage values, even and odd neighbours, both signs."""
    h, _ = _halfway_points(storage)
    return _pad_rows(np.concatenate([h, -h]), dim)


def gen_double_rounding(storage: str, dim: int = 100) -> np.ndarray:
    """normalize=False fp64 values a hair (2^-30 relative, below fp32's half ulp) off a halfway point: rounding through
    fp32 lands ON the halfway point and goes to the even neighbour, rounding directly goes to the nearer one.  Half of
    them differ between the two rules."""
    h, _ = _halfway_points(storage)
    v = np.concatenate([h * (1 + 2.0 ** -30), h * (1 - 2.0 ** -30)])
    return _pad_rows(np.concatenate([v, -v]), dim)


@functools.lru_cache(maxsize=None)
def gen_sensitive(storage: str, mutant: str, dim: int = 16) -> np.ndarray:
    """Gaussian fp32 rows picked, out of 200 000, because ``mutant`` changes a stored bit of them: what the share
    comparison cannot tell apart at an affordable size (a flip rate of a few 1e-5) a bit comparison of these rows does."""
    x = np.random.default_rng(99).standard_normal((200000, dim), dtype=np.float32)
    hit = (prep_reference(x, storage, True) != prep_reference(x, storage, True, mutant=mutant)).any(axis=1)
    assert hit.sum() >= 3, (storage, mutant, int(hit.sum()))
    return x[hit][:40].astype(np.float64)


@dataclass(frozen=True)
class PrepCase:
    name: str
    src: str
    storage: str
    normalize: bool
    gen: tuple                       # (generator name, *args)
    mode: str = "bits"               # "bits": bit for bit; "share": +-1 ulp on at most SHARE_BAR of the elements
    targets: tuple = ()              # mutants this case must tell apart
    ivf: bool = False                # also through IVFFlatIndex.set_centroids / centroids()

    def values(self) -> np.ndarray:
        return _GEN[self.gen[0]](*self.gen[1:])

    def source(self):
        return to_source(self.values(), self.src)

    def expected(self) -> np.ndarray:
        return _prep_expected(self)


_GEN = {"gauss": gen_gauss, "edge_norms": gen_edge_norms, "subnormals": gen_subnormals, "halfway": gen_halfway,
        "double_rounding": gen_double_rounding, "sensitive": gen_sensitive}


@functools.lru_cache(maxsize=None)
def _prep_expected(case: PrepCase) -> np.ndarray:
    bits = prep_reference(case.source(), case.storage, case.normalize)
    bits.setflags(write=False)
    return bits


def _rounds(src: str, storage: str) -> bool:
    """normalize=False: does the conversion round at all (gaussian values, far from either format's range limits)?"""
    return src in ("f32", "f64") or (src, storage) == ("f16", "bf16")


def _prep_cases():
    cases = []
    # every source x storage x normalize at 257 x 100: scalar kernel, ld 128 (28 pad columns), rows not a multiple of 4
    for src in SOURCES:
        for st in STORAGES:
            cases.append(PrepCase(f"types-{src}-{st}-norm", src, st, True, ("gauss", 257, 100, 3),
                                  targets=("trunc", "tail_out_of_norm"), ivf=True))
            cases.append(PrepCase(f"types-{src}-{st}-raw", src, st, False, ("gauss", 257, 100, 3),
                                  targets=("trunc",) if _rounds(src, st) else ()))
    # vector kernel at dim 8 .. 4096, scalar kernel above (ld > 4096): the same expectation on both sides of the boundary
    for dim in (8, 64, 384, 4096, 4104, 8192):
        for st in STORAGES:
            tg = ("trunc",) + (("tail_out_of_norm",) if dim % 64 else ())
            cases.append(PrepCase(f"dim-{dim}-{st}", "f32", st, True, ("gauss", 5, dim, dim), targets=tg))
    for st in STORAGES:
        cases.append(PrepCase(f"edge-norms-{st}", "f32", st, True, ("edge_norms", 100),
                              targets=("ss_f32", "trunc", "tail_out_of_norm"), ivf=True))
        cases.append(PrepCase(f"halfway-{st}", "f32", st, False, ("halfway", st, 100), targets=("trunc",)))
        cases.append(PrepCase(f"double-rounding-{st}", "f64", st, False, ("double_rounding", st, 100),
                              targets=("no_f32_step", "trunc")))
        for m in ("ss_f32", "div_f32"):
            cases.append(PrepCase(f"sensitive-{m}-{st}", "f32", st, True, ("sensitive", st, m), targets=(m,)))
    cases.append(PrepCase("subnormals-f16", "f32", "f16", False, ("subnormals", 100), targets=("flush_subnormal", "trunc")))
    cases.append(PrepCase("subnormals-f64-f16", "f64", "f16", False, ("subnormals", 100), targets=("flush_subnormal", "trunc")))
    # the share cases: ~1.15 M elements, so that a flip rate of 2^-13 shows
    for src in ("f32", "f64"):
        for st in STORAGES:
            cases.append(PrepCase(f"share-{src}-{st}", src, st, True, ("gauss", 3001, 384, 21), mode="share",
                                  targets=SHARE_TARGETS[st]))
    return tuple(cases)


# what the share comparison tells apart at 3001 x 384 (measured shares of the others: DESIGN.md, "Build-path tests")
SHARE_TARGETS = {"f16": ("trunc",), "bf16": ("trunc",)}
PREP_CASES = _prep_cases()


# ------------------------------------------------------------------ IVF training
_M64 = (1 << 64) - 1


def _splitmix64(s: int) -> Tuple[int, int]:
    s = (s + 0x9E3779B97F4A7C15) & _M64
    z = s
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return s, z ^ (z >> 31)


def train_picks(seed: int, n: int, nlist: int) -> np.ndarray:
    """The rows ``IVFFlatIndex.train`` starts from: Floyd's sampling of ``nlist`` distinct rows out of ``n`` driven by
    splitmix64(seed), in ascending row order.  Depends on (seed, n, nlist) only."""
    s = seed & _M64
    chosen = set()
    for j in range(n - nlist, n):
        s, z = _splitmix64(s)
        t = z % (j + 1)
        chosen.add(j if t in chosen else t)
    assert len(chosen) == nlist
    return np.array(sorted(chosen), dtype=np.int64)


def _finish(sums: np.ndarray, cnt: np.ndarray, metric: str, storage: str, mutant: Optional[str]) -> np.ndarray:
    if metric == "cosine":
        return prep_reference(sums, storage, True)
    if mutant != "ip_sum":
        sums = sums / np.maximum(cnt, 1)[:, None]
    return prep_reference(sums, storage, False)


def _assign(x_vals: np.ndarray, cen_bits: np.ndarray, storage: str, high: bool = False):
    """argmax over the DISTINCT centroids (identical centroids tie exactly, whatever the summation order), ties to the
    lowest list (``high``: the highest); margin = best minus second-best distinct centroid's score."""
    uniq, inv = np.unique(cen_bits, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    s = x_vals @ bits_to_f64(uniq, storage).T
    full = s[:, inv]                                               # per list; identical centroids hold copies of one column
    if high:
        a = full.shape[1] - 1 - np.argmax(full[:, ::-1], axis=1)
    else:
        a = np.argmax(full, axis=1)
    if s.shape[1] > 1:
        top = np.partition(s, -2, axis=1)[:, -2:]
        margin = top[:, 1] - top[:, 0]
    else:
        margin = np.full(len(s), np.inf)
    return a.astype(np.int64), margin


def kmeans_step(x_vals: np.ndarray, cen_bits: np.ndarray, metric: str, storage: str, mutant: Optional[str] = None):
    """One Lloyd step in fp64 over stored rows ``x_vals`` (fp64 values of the stored bits) and centroid bits.
    -> (new centroid bits, assignment, margin per row, rows per list).  Cosine: the per-list sum re-normalised and
    rounded; ip: the sum divided by the count and rounded; an empty list keeps its bits."""
    assert mutant is None or mutant in TRAIN_MUTANTS
    nlist = cen_bits.shape[0]
    a, margin = _assign(x_vals, cen_bits, storage, high=(mutant == "ties_high"))
    keep = np.ones(len(a), dtype=bool)
    if mutant == "drop_row":
        last = np.full(nlist, -1)
        last[a] = np.arange(len(a))                                # the last row of every list
        keep[last[last >= 0]] = False
    xs = x_vals
    if mutant == "cols_ge_64":
        xs = x_vals.copy()
        xs[:, 64:] = 0.0
    sums = np.zeros((nlist, x_vals.shape[1]))
    np.add.at(sums, a[keep], xs[keep])
    cnt = np.bincount(a[keep], minlength=nlist)
    new = _finish(sums, cnt, metric, storage, mutant).copy()
    empty = cnt == 0
    new[empty] = 0 if mutant == "zero_empty" else cen_bits[empty]
    return new, a, margin, cnt


def device_step(x_vals: np.ndarray, a: np.ndarray, cen_bits: np.ndarray, metric: str, storage: str, rng) -> np.ndarray:
    """The device's arithmetic for one update on a given assignment: fp32 sums of the rows in a shuffled order (the
    atomics' order is not defined), then cosine: K1's normalisation of the fp32 sums; ip: (float)((double)sum / count)."""
    nlist = cen_bits.shape[0]
    perm = rng.permutation(len(a))
    sums = np.zeros((nlist, x_vals.shape[1]), dtype=np.float32)
    np.add.at(sums, a[perm], x_vals[perm].astype(np.float32))
    cnt = np.bincount(a, minlength=nlist)
    if metric == "cosine":
        new = prep_reference(sums, storage, True).copy()
    else:
        new = prep_reference((sums.astype(np.float64) / np.maximum(cnt, 1)[:, None]).astype(np.float32), storage, False).copy()
    new[cnt == 0] = cen_bits[cnt == 0]
    return new


@dataclass(frozen=True)
class TrainCase:
    name: str
    metric: str
    storage: str
    dim: int
    n: int
    nlist: int
    iters: int
    seed: int
    kind: str = "clusters"           # "clusters", "empty" (two identical starting rows), "ints" (rows in -2..2)

    @property
    def mutants(self) -> tuple:
        if self.iters == 0:
            return ()
        m = ["drop_row"]
        if self.dim > 64:
            m.append("cols_ge_64")
        if self.metric == "ip":
            m.append("ip_sum")
        if self.kind == "empty":
            m.append("zero_empty")
        if self.kind == "ints":
            m.append("ties_high")
        return tuple(m)


EMPTY_LISTS = (2, 5)                 # kind "empty": the starting rows of these two lists are identical


def train_rows(case: TrainCase):
    """-> (stored bits of the training rows [n, dim], the picked rows).  Tight clusters, one per list, with the row at
    the j-th picked position in cluster j; cosine rows are unit rows, ip rows are the raw cluster points."""
    picks = train_picks(case.seed, case.n, case.nlist)
    rng = np.random.default_rng(1000 + case.seed)
    if case.kind == "ints":
        vals = rng.integers(-2, 3, size=(case.n, case.dim)).astype(np.float64)
        return prep_reference(vals, case.storage, False), picks
    centres = ds.l2_normalize(rng.standard_normal((case.nlist, case.dim))).astype(np.float64)
    cl = rng.integers(0, case.nlist, size=case.n)
    cl[picks] = np.arange(case.nlist)
    raw = centres[cl] + (0.3 / np.sqrt(case.dim)) * rng.standard_normal((case.n, case.dim))
    if case.kind == "empty":
        lo, hi = EMPTY_LISTS
        raw[(cl == lo) | (cl == hi)] = raw[picks[lo]]              # one point, many copies: the cluster's mean is the point
    return prep_reference(raw, case.storage, case.metric == "cosine"), picks


@functools.lru_cache(maxsize=None)
def train_expected(case: TrainCase) -> dict:
    """Iterated ``kmeans_step`` from the picked rows, plus the device emulation of the last update in several orders.
    ``emu_diff``: the most elements any emulated order moved (each by at most ``emu_ulp`` ulp) against the fp64 result."""
    bits, picks = train_rows(case)
    x = bits_to_f64(bits, case.storage)
    cen = bits[picks].copy()
    out = {"rows": bits, "picks": picks, "start": cen.copy(), "min_margin": np.inf, "emu_diff": 0, "emu_ulp": 0, "counts": None}
    prev = cen
    for _ in range(case.iters):
        prev = cen
        cen, a, margin, cnt = kmeans_step(x, cen, case.metric, case.storage)
        out["min_margin"] = min(out["min_margin"], float(margin.min()))
        out["assign"], out["counts"] = a, cnt
    out["centroids"] = cen
    if case.iters:
        rng = np.random.default_rng(5)
        for _ in range(4):
            emu = device_step(x, out["assign"], prev, case.metric, case.storage, rng)
            d = np.abs(ulp_diff(emu, cen))
            out["emu_diff"] = max(out["emu_diff"], int((d != 0).sum()))
            out["emu_ulp"] = max(out["emu_ulp"], int(d.max()))
    out["allowed_diff"] = max(1, int(MUTANT_FACTOR * out["emu_diff"]))
    return out


def train_mutant(case: TrainCase, mutant: str) -> np.ndarray:
    bits, picks = train_rows(case)
    x = bits_to_f64(bits, case.storage)
    cen = bits[picks].copy()
    for _ in range(case.iters):
        cen = kmeans_step(x, cen, case.metric, case.storage, mutant)[0]
    return cen


def train_matches(got_bits: np.ndarray, exp: dict) -> Tuple[bool, int, int]:
    """The GPU comparison: every element within 1 storage ulp, at most ``allowed_diff`` elements off at all."""
    d = np.abs(ulp_diff(got_bits, exp["centroids"]))
    ndiff, worst = int((d != 0).sum()), int(d.max())
    return (worst <= 1 and ndiff <= exp["allowed_diff"]), ndiff, worst


def _train_cases():
    cases = [TrainCase("start-8-of-1000", "cosine", "f16", 64, 1000, 8, 0, 11),
             TrainCase("start-300-of-777", "cosine", "f16", 100, 777, 300, 0, 12),     # centroid matrix spans two 256-row tiles
             TrainCase("start-300-of-777-bf16", "ip", "bf16", 100, 777, 300, 0, 13),
             TrainCase("start-n-equals-nlist", "cosine", "f16", 64, 40, 40, 0, 14)]
    seed = 20
    for metric in ("cosine", "ip"):
        for st in STORAGES:
            for dim in (64, 100):
                for n, nlist in ((2003, 8), (4999, 37)):
                    for iters in (1, 3):
                        seed += 1
                        cases.append(TrainCase(f"{metric}-{st}-d{dim}-n{n}-it{iters}", metric, st, dim, n, nlist, iters, seed))
    for st in STORAGES:
        cases.append(TrainCase(f"ints-ip-{st}", "ip", st, 64, 2000, 8, 1, 60, kind="ints"))
        for metric in ("cosine", "ip"):
            cases.append(TrainCase(f"empty-{metric}-{st}", metric, st, 100, 600, 8, 2, 61, kind="empty"))
    return tuple(cases)


TRAIN_CASES = _train_cases()
