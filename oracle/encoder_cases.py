"""Shared case definitions of the encoder tests.  TEST INFRASTRUCTURE (oracle/__init__.py).

Three things live here, used by the CPU test of the suite's discriminating power (tests/test_encoder_sensitivity.py) and by
the GPU parity tests (tests/test_gpu_encoder_paths.py, tests/test_gpu_encoder.py):

* inputs that make attention matter: ``sharp_weights`` (query / key matrices scaled so that the softmax is neither uniform nor
  saturated) and mask generators (trailing padding, left padding, holes, values other than 0 / 1, an empty row, a row whose
  few valid keys sit on the kernels' tile boundaries);
* the noise model ``forward_rounded``: the oracle's fp64 forward with the roundings a 16-bit pipeline cannot avoid (layer
  matrices, every stored activation tensor, the softmax probabilities).  The tolerance of a GPU comparison is
  ``TOL_FACTOR x`` the largest deviation this emulation shows on the same inputs -- derived from the number format, never
  from what the kernels return;
* structural mutants of the forward pass (a dropped key, an attended padding key, a wrong pooling divisor, ...): the CPU
  test asserts that every one of them moves a compared output by at least ``MUTANT_MARGIN x`` its tolerance.

``_run`` is a private copy of ``oracle.encoder.forward`` with the rounding points and mutation hooks; with neither it equals
the oracle to the last bits (asserted by the CPU test).
"""
from __future__ import annotations

import functools
import math
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import encoder as oe

TOL_FACTOR = 4.0        # tolerance = 4 x emulated rounding noise (fp32 accumulation order and hardware exp are not modelled)
MUTANT_MARGIN = 2.0     # a structural mutant must move a compared output by at least 2 x its tolerance
PROB_BAND = (0.3, 0.7)  # mean of each query's largest attention probability, every layer of every case
POOLS = ("mean", "cls")

# geometries: (oracle spec name, overrides).  max_position 512 everywhere: S runs up to 512.
GEOMETRIES = {
    "dh32": dict(oe.SPECS["tiny"], max_position=512),                                   # 2 heads x 32
    "dh64": dict(oe.SPECS["small"], max_position=512),                                  # 2 heads x 64
    "minilm": dict(oe.SPECS["minilm-l6"], vocab_size=3000, layers=2),                   # 12 heads x 32, K = 384 / 1536 (skinny GEMM)
    "bge": dict(oe.SPECS["bge-base"], vocab_size=3000, layers=2),                       # 12 heads x 64, K = 768 / 3072
}


_GAINS = {   # geometry -> ((largest S, gain), ...): chosen on the CPU so that every case's attention lies inside PROB_BAND
    "dh32": ((32, 4.0), (128, 5.0), (300, 5.5), (512, 6.0)),
    "dh64": ((32, 2.5), (128, 3.25), (300, 3.5), (512, 3.75)),
    "minilm": ((16, 1.6), (32, 1.8), (64, 2.0), (512, 2.4)),
    "bge": ((128, 1.5), (512, 2.0)),
}


def qk_gain(geometry: str, S: int) -> float:
    """Factor on every layer's query and key matrices.  Logits grow with the square of it; a softmax over more keys needs
    larger logits for the same largest probability, so the gain of an architecture rises slowly with S."""
    return next(g for top, g in _GAINS[geometry] if S <= top)


def sharp_weights(spec, seed: int, gain: float) -> Dict[str, np.ndarray]:
    """``oracle.encoder.seeded_weights`` with every layer's query and key weight matrices scaled by ``gain``."""
    w = oe.seeded_weights(spec, seed)
    for i in range(spec["layers"]):
        for n in ("query", "key"):
            k = f"encoder.layer.{i}.attention.self.{n}.weight"
            w[k] = (w[k] * np.float32(gain)).astype(np.float32)
    return w


# ---------------------------------------------------------------------------------------------- masks
BOUNDARY_KEYS = (64, 128, 256)      # first key of a new tile: of the SP 128 / 256 kernels' padding, of the general kernel's key blocks


def mask_row(kind: str, S: int, arg: int = 0, rng: Optional[np.random.Generator] = None) -> np.ndarray:
    """One int32 mask row.  ``trailing`` / ``left``: ``arg`` valid tokens at the start / end; ``holes``: about 60 % valid at
    random, first and last slot valid; ``values``: ``arg`` leading valid tokens marked by integers other than 1 (they count
    as valid: oracle and kernels read ``!= 0``); ``pair``: slot 0 and slot ``arg`` only (a tile-boundary key that carries
    half of the row); ``empty``: no valid token."""
    m = np.zeros(S, dtype=np.int32)
    if kind == "trailing":
        m[:arg] = 1
    elif kind == "left":
        m[S - arg:] = 1
    elif kind == "holes":
        m[:] = (rng.random(S) < 0.6).astype(np.int32)
        m[0] = m[S - 1] = 1
    elif kind == "values":
        m[:arg] = rng.choice(np.array([2, -1, 7, 1 << 20, -(1 << 31)], dtype=np.int64), size=arg).astype(np.int32)
    elif kind == "pair":
        m[[0, arg]] = 1
    elif kind != "empty":
        raise ValueError(kind)
    return m


def mixed_rows(S: int) -> List[Tuple[str, int]]:
    """The batch of the attention cases: every mask family in one batch, lengths 1, 2, S - 1 and S among them."""
    rows = [("trailing", S), ("trailing", 1), ("trailing", 2), ("trailing", S - 1),
            ("left", max(1, S - 130) if S > 256 else max(1, S // 3)),       # S > 256: >= 128 leading zeros, two masked key blocks
            ("left", 1), ("holes", 0), ("values", max(2, (2 * S) // 3))]
    return rows + [("pair", k) for k in BOUNDARY_KEYS if k < S]


class Case(NamedTuple):
    name: str
    geometry: str
    S: int
    rows: Tuple[Tuple[str, int], ...]
    dtypes: Tuple[str, ...] = ("f16", "bf16")
    seed: int = 5
    note: str = ""             # what the case is for (kernel / path)
    B: int = 0                 # > 0: a ``large_batch`` of B rows instead of ``rows``; the oracle sees ``sample()`` only

    @property
    def spec(self):
        return GEOMETRIES[self.geometry]

    def weights(self):
        return _weights(self.geometry, self.seed, qk_gain(self.geometry, self.S))

    def batch(self):
        """ids / mask int32 [B, S]; ids are random everywhere, masked slots included (they must not matter)."""
        if self.B:
            return large_batch(self.geometry, self.B, self.S, self.seed)[:2]
        rng = np.random.default_rng(1000 + self.seed * 7919 + self.S)
        mask = np.stack([mask_row(k, self.S, a, rng) for k, a in self.rows])
        ids = rng.integers(3, self.spec["vocab_size"], size=mask.shape).astype(np.int32)
        return ids, mask

    def sample(self) -> np.ndarray:
        """Rows that are compared against the oracle (all of them, but for the large batches)."""
        return large_batch(self.geometry, self.B, self.S, self.seed)[2] if self.B else np.arange(len(self.rows))

    def oracle_batch(self):
        ids, mask = self.batch()
        sub = self.sample()
        return ids[sub], mask[sub]


@functools.lru_cache(maxsize=8)
def _weights(geometry, seed, gain):
    return sharp_weights(GEOMETRIES[geometry], seed, gain)


ATTENTION_S = (16, 64, 65, 128, 129, 256, 257, 300, 511, 512)


def attention_instance(dh: int, S: int) -> str:
    """Kernel that ``launch_attention`` launches for this head dim and sequence length (read off its dispatch in
    csrc/enc_attention.hip)."""
    if S > 256:
        return f"enc_attention_kernel<DT, {dh}, 8>"
    sp = 64 if S <= 64 else 128 if S <= 128 else 256
    return f"enc_attention_s128_kernel<DT, {dh}, {sp}, {8 if sp == 256 else 4}>"


ATTENTION_CASES = tuple(Case(f"{g}-S{S}", g, S, tuple(mixed_rows(S)), note=attention_instance(int(g[2:]), S))
                        for g in ("dh32", "dh64") for S in ATTENTION_S)

# MiniLM widths (K = 384 / 1536: the only ones the skinny GEMM takes), M = B x S tokens
GEMM_CASES = (
    Case("skinny-1x16", "minilm", 16, (("trailing", 13),), note="skinny NFR 1, M = 16"),
    Case("skinny-1x9", "minilm", 9, (("trailing", 9),), note="skinny NFR 1, M = 9"),
    Case("skinny-2x16", "minilm", 16, (("trailing", 16), ("trailing", 5)), note="skinny NFR 2, M = 32"),
    Case("skinny-4x16", "minilm", 16, (("trailing", 16), ("trailing", 1), ("left", 7), ("values", 12)),
         note="skinny NFR 4, M = 64 (last skinny size)"),
    Case("tiled-5x13", "minilm", 13, (("trailing", 13), ("trailing", 1), ("left", 7), ("values", 9), ("holes", 0)),
         note="128 x 128 GEMM, M = 65 (first size past the skinny path)"),
    Case("tiled-8x64", "minilm", 64, (("trailing", 64), ("trailing", 1), ("trailing", 2), ("trailing", 63), ("left", 20),
                                           ("holes", 0), ("values", 40), ("trailing", 33)),
         note="128 x 128 GEMM, M = 512: a multiple of 256 too small to fill the chip"),
)

# batches large enough for the 256 x 256 GEMMs and the fused-LayerNorm flow; compared on a sample of the rows
LARGE_CASES = (
    Case("large-minilm-512x32", "minilm", 32, (), B=512, seed=17, note="fused-LayerNorm flow and plain 256 x 256 flow, M = 16384"),
    Case("large-bge-130x96", "bge", 96, (), B=130, seed=19,
         note="fused-LayerNorm flow and plain 256 x 256 flow, ragged: M = 12480 < M_pad = 12544"),
    Case("large-dh64-342x96", "dh64", 96, (), B=342, seed=23,
         note="fused-LayerNorm flow with hidden 128: Linears narrower than one 256-row weight tile; M = 32832 < M_pad = 33024"),
)

CASES = ATTENTION_CASES + GEMM_CASES + LARGE_CASES


def large_batch(geometry: str, B: int, S: int, seed: int):
    """Large ragged batch for the 256 x 256 / fused-LayerNorm flows: trailing lengths 1 .. S (both ends present), a left-padded, a
    holed and the tile-boundary ``pair`` rows.  -> (ids, mask, sample): ``sample`` = rows to compare against the oracle -- first, last, shortest, longest
    and an even spread."""
    spec = GEOMETRIES[geometry]
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, S + 1, size=B)
    lens[1], lens[2] = 1, S
    mask = np.stack([mask_row("trailing", S, int(L)) for L in lens])
    mask[3] = mask_row("left", S, S // 3)
    mask[4] = mask_row("holes", S, 0, rng)
    for i, k in enumerate(k for k in BOUNDARY_KEYS if k < S):
        mask[5 + i] = mask_row("pair", S, k)
    ids = rng.integers(3, spec["vocab_size"], size=mask.shape).astype(np.int32)
    cnt = (mask != 0).sum(1)
    sample = sorted({0, B - 1, int(cnt.argmin()), int(cnt.argmax()), 3, 4, 5, 6, 7, *range(8, B, max(1, B // 10))})
    return ids, mask, np.array(sample)


# ---------------------------------------------------------------------------------------------- forward with hooks
def _rounder(dtype: Optional[str]):
    if dtype is None:
        return lambda a: a
    if dtype == "f16":
        return lambda a: a.astype(np.float16).astype(np.float64)
    if dtype == "bf16":
        return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()
    raise ValueError(dtype)


MUTANTS = ("drop_last_valid", "attend_first_masked", "drop_key_64", "drop_key_128", "drop_key_256", "leading_block",
           "pool_div_S", "pos_shift", "swap_v_heads")
REPORTED_MUTANTS = ("scale_dh_plus_1", "tanh_gelu")
# The scale mutant is asserted where the CPU measurement put it at MUTANT_MARGIN x tol or more: one (case, dtype) pair.
# Everywhere else it stays below that (0.1 - 1.9 x tol in fp16, below 0.3 x tol in bf16) and is printed only.
SCALE_MUTANT_ASSERTED = (("skinny-1x16", "f16"),)


def mutated_keys(mask: np.ndarray, mut: Optional[str]) -> Optional[np.ndarray]:
    """Boolean [B, S] "key is attended" under the mutant, or None where the mutant does not apply to this batch (it would
    change nothing).  Rows the mutant would leave without any key, and rows without a valid key, stay as they are."""
    valid = mask != 0
    keys = valid.copy()
    B, S = mask.shape
    n = valid.sum(1)
    if mut == "drop_last_valid":
        for b in np.nonzero(n >= 2)[0]:
            keys[b, np.nonzero(valid[b])[0][-1]] = False
    elif mut == "attend_first_masked":
        for b in np.nonzero((n >= 1) & (n < S))[0]:
            keys[b, np.nonzero(~valid[b])[0][0]] = True
    elif mut in ("drop_key_64", "drop_key_128", "drop_key_256"):
        k = int(mut.rsplit("_", 1)[1])
        if k < S:
            keys[(n >= 2) & valid[:, k], k] = False
    elif mut == "leading_block":
        if S > 64:
            keys[(n >= 1) & ~valid[:, :64].any(1), :64] = True
    else:
        return keys
    return None if np.array_equal(keys, valid) else keys


def _run(spec, w, ids, mask, dtype: Optional[str] = None, mut: Optional[str] = None, probs: Optional[list] = None):
    """fp64 forward up to the last LayerNorm -> hidden states [B, S, H].  ``dtype``: round what a 16-bit pipeline stores
    (see forward_rounded).  ``mut``: one structural mutant.  ``probs``: list that receives, per layer, the mean over valid
    queries and heads of the largest attention probability."""
    rnd = _rounder(dtype)
    W = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    if dtype is not None:
        for k in W:
            if k.startswith("encoder.layer.") and k.endswith(".weight") and "LayerNorm" not in k:
                W[k] = rnd(W[k])
    B, S = ids.shape
    H, nh, eps = spec["hidden"], spec["heads"], spec["layer_norm_eps"]
    dh = H // nh
    pos = W["embeddings.position_embeddings.weight"]
    pos = np.roll(pos, -1, axis=0)[:S] if mut == "pos_shift" else pos[:S]
    x = W["embeddings.word_embeddings.weight"][ids] + pos[None] + W["embeddings.token_type_embeddings.weight"][0][None, None]
    x = rnd(oe._ln(x, W["embeddings.LayerNorm.weight"], W["embeddings.LayerNorm.bias"], eps))
    keys = mutated_keys(mask, mut)
    if keys is None:
        return None
    bias = np.where(keys[:, None, None, :], 0.0, -1e30)
    scale = 1.0 / math.sqrt(dh + 1 if mut == "scale_dh_plus_1" else dh)
    valid_q = (mask != 0)
    for i in range(spec["layers"]):
        p = f"encoder.layer.{i}."
        lin = lambda t, n: t @ W[p + n + ".weight"].T + W[p + n + ".bias"]     # noqa: E731
        q = rnd(lin(x, "attention.self.query")).reshape(B, S, nh, dh).transpose(0, 2, 1, 3)
        k = rnd(lin(x, "attention.self.key")).reshape(B, S, nh, dh).transpose(0, 2, 1, 3)
        v = rnd(lin(x, "attention.self.value")).reshape(B, S, nh, dh).transpose(0, 2, 1, 3)
        if mut == "swap_v_heads":
            v = v.copy()
            v[:, [0, 1]] = v[:, [1, 0]]
        sc = q @ k.transpose(0, 1, 3, 2) * scale + bias
        sc = sc - sc.max(-1, keepdims=True)
        pr = np.exp(sc)
        den = pr.sum(-1, keepdims=True)
        if probs is not None:
            pm = (pr / den).max(-1)                                             # [B, nh, S]
            probs.append(float(pm.transpose(0, 2, 1)[valid_q].mean()))
        # the kernels round exp(score - max) and divide the P V product by the fp32 sum of the unrounded terms
        ctx = rnd(((rnd(pr) @ v) / den).transpose(0, 2, 1, 3).reshape(B, S, H))
        y = rnd(lin(ctx, "attention.output.dense") + x)
        x = rnd(oe._ln(y, W[p + "attention.output.LayerNorm.weight"], W[p + "attention.output.LayerNorm.bias"], eps))
        h = lin(x, "intermediate.dense")
        if mut == "tanh_gelu":
            h = 0.5 * h * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (h + 0.044715 * h ** 3)))
        else:
            h = 0.5 * h * (1.0 + oe._erf(h / math.sqrt(2.0)))
        y = rnd(lin(rnd(h), "output.dense") + x)
        x = rnd(oe._ln(y, W[p + "output.LayerNorm.weight"], W[p + "output.LayerNorm.bias"], eps))
    return x


def pooled(x: np.ndarray, mask: np.ndarray, pool: str, normalize: bool, mut: Optional[str] = None) -> np.ndarray:
    if pool == "cls":
        e = x[:, 0]
    else:
        m = (mask != 0).astype(np.float64)[:, :, None]
        div = np.full((x.shape[0], 1), float(x.shape[1])) if mut == "pool_div_S" else np.maximum(m.sum(1), 1e-9)
        e = (x * m).sum(1) / div
    if normalize:
        e = e / np.maximum(np.linalg.norm(e, axis=1, keepdims=True), 1e-12)
    return e


def forward_rounded(spec, w, ids, mask, pool: str, normalize: bool, dtype: str) -> np.ndarray:
    """The oracle's forward in fp64 with the roundings of a 16-bit pipeline -- the noise model:

    * the layer matrices (Q / K / V / attention output / FFN weights) are rounded to ``dtype`` ("f16", or "bf16" through a
      ``torch.bfloat16`` round trip); embeddings, biases and LayerNorm parameters stay fp32, as the encoder keeps them;
    * every tensor the HIP encoder stores in 16 bits is rounded: embedding-LayerNorm output, q / k / v, the attention context,
      each GEMM + residual output, each LayerNorm output and the GELU output;
    * the softmax numerators are rounded before P V.
    Pooling and normalisation stay fp64 (the kernel pools in fp32)."""
    return pooled(_run(spec, w, ids, mask, dtype=dtype), mask, pool, normalize)


QUANTITIES = tuple((pool, norm) for pool in POOLS for norm in (True, False))       # what a GPU case compares


def quantities(x, mask, mut=None):
    return {(pool, norm): pooled(x, mask, pool, norm, mut) for pool, norm in QUANTITIES}


class Expected(NamedTuple):
    want: Dict[Tuple[str, bool], np.ndarray]     # the oracle's fp64 forward
    noise: Dict[Tuple[str, bool], float]         # max |forward_rounded - forward|
    tol: Dict[Tuple[str, bool], float]           # TOL_FACTOR x noise


def expected(spec, w, ids, mask, dtype: str, want=None) -> Expected:
    """Reference outputs and tolerances of one batch in one dtype, for all four compared quantities.  ``want``: the fp64
    outputs where the caller has them already (they do not depend on the dtype)."""
    if want is None:
        want = quantities(_run(spec, w, ids, mask), mask)      # == oracle.encoder.forward (tests/test_encoder_sensitivity.py)
    xr = _run(spec, w, ids, mask, dtype=dtype)
    noise = {q: float(np.abs(pooled(xr, mask, *q) - want[q]).max()) for q in QUANTITIES}
    return Expected(want, noise, {q: TOL_FACTOR * n for q, n in noise.items()})


CASE_BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def case_want(name: str):
    c = CASE_BY_NAME[name]
    ids, mask = c.oracle_batch()
    return quantities(_run(c.spec, c.weights(), ids, mask), mask)


@functools.lru_cache(maxsize=None)
def case_expected(name: str, dtype: str) -> Expected:
    """Expected outputs (rows ``case.sample()``) and tolerances of a listed case."""
    c = CASE_BY_NAME[name]
    ids, mask = c.oracle_batch()
    return expected(c.spec, c.weights(), ids, mask, dtype, want=case_want(name))
