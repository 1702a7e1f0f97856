"""Row-sharded corpus search: one process per GPU, each rank owns a
contiguous block of corpus rows, runs the fused similarity + top-k locally, then ONE
all-gather of the per-shard (score, global id) partial top-k (RCCL over xGMI when the
process group is ``nccl``; ``gloo`` in the CPU tests) followed by the merge: on the host
(``mrag_topk_merge``, C++ threads) for host tensors, and by default on the device
(``mrag_topk_merge_packed_device``) when the gathered buffers are in HBM -- the merged [Q,k] result is
then the only thing that crosses PCIe (C4 at 8 GPUs: 1.2 MB instead of 9.6 MB + 0.5 ms of host
merge per step).  Result = the single-GPU result: ids are global, tie-break (score desc, id asc).

The exchange is ONE collective of 8-byte (fp32 score bits, int32 shard-local row) words -- Q*k*8 bytes per
rank (C4: 10 000 x 10 -> 800 KB, 6.4 MB gathered at 8 GPUs) -- latency-bound, so a direct all-gather on the
fully connected xGMI mesh, no ring tuning, no all-reduce; global ids are rebuilt from the rank's row base,
which every rank knows (``shard_bounds``).  The whole sequence -- pack, all-gather, merge, pinned D2H, the call's
one stream sync, the range-flag check -- and every buffer it uses belong to :class:`_Exchange`.

``ShardedIVFIndex`` is the same for IVF-flat (BASELINE config 5): rows sharded, centroids trained once and
replicated, so every GPU holds 1/N of every list and does equal work for any probe set.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import numpy as np

from .index import _check_precision, pack_partial_device, topk_merge, topk_merge_packed_device


def shard_bounds(n_total: int, world: int, rank: int) -> Tuple[int, int]:
    """Contiguous row block of ``rank``: [lo, hi)."""
    return (n_total * rank) // world, (n_total * (rank + 1)) // world


def local_allow_mask(allow, n_total: int, lo: int, hi: int) -> np.ndarray:
    """Global allow-set (bool / uint8 mask over the ``n_total`` rows, or global row positions) -> the local mask over
    rows ``[lo, hi)`` of one shard (numpy bool), as the single-GPU indexes take it."""
    from .index import allow_bits
    words = allow_bits(allow, n_total)        # validates length / range / shape like the single index
    mask = np.unpackbits(words.view(np.uint8), bitorder="little")[:n_total].astype(np.bool_)
    return mask[lo:hi]


class _Phases:
    """Per-phase milliseconds of one exchange.  CUDA inputs: events on the current stream, read after the call's
    final stream sync (no extra sync); host inputs: ``time.perf_counter``."""

    def __init__(self, cuda: bool, device=None):
        self.cuda, self.device, self.marks = cuda, device, []

    def mark(self, name: str):
        if self.cuda:
            import torch
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream(self.device))
            self.marks.append((name, e))
        else:
            import time
            self.marks.append((name, time.perf_counter()))

    def result(self) -> dict:
        out = {}
        for (_, a), (name, b) in zip(self.marks, self.marks[1:]):
            ms = a.elapsed_time(b) if self.cuda else (b - a) * 1e3
            out[name] = out.get(name, 0.0) + float(ms)
        return out


def _device_merge_applies(merge: str, world: int, k: int) -> bool:
    return merge == "device" or (merge == "auto" and world <= 64 and world * k <= 2048)


def _raise_if_bad(bad_host) -> None:
    if int(bad_host) != 0:
        raise ValueError("gather_and_merge: a local id lies outside [id_base, id_base + 2^32 - 1) -- the packed exchange "
                         "carries shard-local rows in 32 bits (is the index's id_base set to the shard's first row?)")


def pack_partial(scores, ids, id_base: int, return_bad: bool = False):
    """[Q,k] fp32 scores + int64 GLOBAL ids (-1 = empty) -> int64 words: score bits in the high half, the
    shard-local row (id - id_base, 32 bits) in the low half.  ``return_bad``: also a 1-element int32 tensor (the
    dtype of the pack kernel's flag), non-zero when some non-empty id is outside [id_base, id_base + 0xFFFFFFFF).
    The caller raises AFTER the collective (a rank that raised before it would leave the others waiting in it); on
    CUDA the flag rides along with the result copy and is checked after the call's one sync instead of forcing a
    sync inside the exchange."""
    import torch
    local = ids - id_base
    empty = ids < 0
    words = (scores.contiguous().view(torch.int32).to(torch.int64) << 32) | \
        (torch.where(empty, torch.full_like(ids, 0xFFFFFFFF), local) & 0xFFFFFFFF)
    if not return_bad:
        return words
    bad = (((local < 0) | (local >= 0xFFFFFFFF)) & ~empty).any().to(torch.int32).view(1)
    return words, bad


def unpack_partial(words, bases):
    """Inverse of :func:`pack_partial` for gathered words [world,Q,k]; ``bases`` [world,1,1] int64."""
    import torch
    scores = (words >> 32).to(torch.int32).view(torch.float32)
    low = words & 0xFFFFFFFF
    ids = torch.where(low == 0xFFFFFFFF, torch.full_like(low, -1), low + bases)
    return scores, ids


def _bases_key(id_bases):
    """First global row of every rank, as a tuple of ints (compared by VALUE), or None."""
    return None if id_bases is None else tuple(int(b) for b in id_bases)


class _Exchange:
    """The exchange of one sharded index, and the owner of every buffer it uses.  One call is
    ``begin`` -> ``post`` once per part of the batch -> ``collect``:

    * ``post`` packs a part's local [q,k] (score, global id) into 8-byte words and starts its all-gather;
    * ``collect`` waits for each part, merges its [world,q,k] into its rows of the [nq,k] result, copies the result
      to pinned host memory, does the call's ONE stream sync and then checks the out-of-range flag.

    The one-shot exchange is the one-part case (a blocking collective); with two parts the collectives are
    ``async_op`` and the first is in flight while the caller computes the second part.  Alone (a world of one, not
    forced through the collective) the same three calls are the pinned D2H of the local result and the one sync.

    Buffers fit the current call -- world, nq, k, the cuts, the device -- and are replaced when that changes; nothing
    is kept per batch size.  With CUDA inputs the returned arrays are views of pinned buffers, two sets used
    alternately, which stay valid until the call AFTER the next one (no per-call allocation or copy)."""

    def __init__(self, group=None, id_bases=None):
        self.group = group
        self.id_bases = _bases_key(id_bases)
        self.world, self.rank = 1, 0
        self._fit = None                 # what the buffers below were made for
        self.bases = None                # [world] int64 on the exchange's device
        self.flag = None                 # [1] int32 on the exchange's device: some posted id did not fit 32 bits
        self.gather: List = []           # per part: [world, q, k] int64
        self.words = self.merged = None  # device merge: [nq,k] packed words; ([nq,k] f32, [nq,k] i64)
        self.stage: List = []            # CUDA + host merge: per part, pinned ([world,q,k] f32, [world,q,k] i64)
        self.host_flag = None            # pinned copy of ``flag``
        self._ring, self._ring_fit, self._turn = None, None, 0
        self._phases: Optional[_Phases] = None

    def mark(self, name: str) -> None:
        if self._phases is not None:
            self._phases.mark(name)

    def phases(self) -> dict:
        return self._phases.result() if self._phases is not None else {}

    def _host_pair(self):
        import torch
        if self._ring_fit != (self.nq, self.k):
            self._ring_fit = (self.nq, self.k)
            self._ring = [(torch.empty((self.nq, self.k), dtype=torch.float32, pin_memory=True),
                           torch.empty((self.nq, self.k), dtype=torch.int64, pin_memory=True)) for _ in range(2)]
        self._turn ^= 1
        return self._ring[self._turn]

    def begin(self, nq: int, k: int, device, merge: str = "auto", force_collective: bool = False,
              pipeline: bool = False, timed: bool = False) -> List[Tuple[int, int]]:
        """Start a call for ``nq`` queries whose local results live on ``device``; returns the row ranges the
        caller posts, in order (two with ``pipeline``, when the batch can be cut and there is a collective to hide)."""
        import torch.distributed as dist
        self.nq, self.k, self.device, self.cuda = int(nq), int(k), device, device.type == "cuda"
        self.world, self.rank = (dist.get_world_size(self.group), dist.get_rank(self.group)) if dist.is_initialized() else (1, 0)
        self.alone = self.world == 1 and not force_collective   # (force_collective: all-gather + merge even alone -- tests)
        self.cuts = [(0, self.nq)]
        self._posted: List = []
        self._phases = _Phases(self.cuda, device) if timed else None
        if not self.alone:
            self._prepare(merge, pipeline)
        self.mark("start")
        return self.cuts

    def _prepare(self, merge: str, pipeline: bool) -> None:
        import torch
        device = self.device
        if merge == "device" and not self.cuda:
            raise ValueError("merge='device' needs CUDA tensors")
        if pipeline and self.nq >= 2:
            h = self.nq // 2
            if h > 256:
                h = (h + 255) // 256 * 256          # cut on a query-tile boundary of the batch kernel
            self.cuts = [(0, h), (h, self.nq)]
        # CUDA + device merge: one pack kernel, the collective, one merge kernel that unpacks the gathered words on its way
        # into LDS (the torch forms are ~8 + ~6 elementwise kernels per step: 0.1-0.15 ms at C4's 10 000 x 10)
        self.on_device = self.cuda and _device_merge_applies(merge, self.world, self.k)
        fit = (self.world, self.nq, self.k, tuple(self.cuts), str(device))
        if self._fit != fit:
            if self.id_bases is None:
                raise ValueError("gather_and_merge needs id_bases (first global row of every rank) for N > 1")
            if len(self.id_bases) != self.world:
                raise ValueError(f"id_bases has {len(self.id_bases)} entries for a world of {self.world}")
            self._fit = fit
            self.bases = torch.as_tensor(list(self.id_bases), dtype=torch.int64, device=device)
            self.flag = torch.zeros(1, dtype=torch.int32, device=device)
            self.gather = [torch.empty((self.world, b - a, self.k), dtype=torch.int64, device=device) for a, b in self.cuts]
            self.words = self.merged = None
            self.stage = []
            if self.cuda and self.host_flag is None:
                self.host_flag = torch.zeros(1, dtype=torch.int32, pin_memory=True)
        if self.on_device and self.words is None:
            self.words = torch.empty((self.nq, self.k), dtype=torch.int64, device=device)
            self.merged = (torch.empty((self.nq, self.k), dtype=torch.float32, device=device),
                           torch.empty((self.nq, self.k), dtype=torch.int64, device=device))
        if self.cuda and not self.on_device and not self.stage:
            self.stage = [(torch.empty(g.shape, dtype=torch.float32, pin_memory=True),
                           torch.empty(g.shape, dtype=torch.int64, pin_memory=True)) for g in self.gather]
        self.flag.zero_()

    def post(self, scores, ids, part: int = 0) -> None:
        """Hand over the local result of ``cuts[part]``: [q,k] float32 scores and int64 global ids, torch tensors on
        the call's device or numpy arrays (host)."""
        import torch
        import torch.distributed as dist
        if not torch.is_tensor(scores):
            scores, ids = torch.from_numpy(np.ascontiguousarray(scores)), torch.from_numpy(np.ascontiguousarray(ids))
        if self.alone:
            self._posted.append((scores, ids))
            return
        a, b = self.cuts[part]
        # this rank's base comes from the HOST list (reading bases[rank] back from the device would be a blocking
        # sync inside the exchange)
        if self.on_device:
            words = pack_partial_device(scores, ids, self.id_bases[self.rank], out_words=self.words[a:b], bad_flag=self.flag)
        else:
            words, bad = pack_partial(scores, ids, self.id_bases[self.rank], return_bad=True)
            self.flag |= bad
        self.mark("pack_ms")
        # ONE collective per part: (score bits << 32) | shard-local row (0xFFFFFFFF = empty slot); output = the inputs
        # concatenated along dim 0 (the layout both nccl and gloo accept)
        work = dist.all_gather_into_tensor(self.gather[part].view(self.world * (b - a), self.k), words, group=self.group,
                                           async_op=len(self.cuts) > 1)
        self._posted.append((work, words))          # (words stays referenced until the collective is done)

    def collect(self, nthreads: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """Every rank returns the full merged (scores [nq,k] float32, ids [nq,k] int64) as numpy arrays."""
        import torch
        stream = torch.cuda.current_stream(self.device) if self.cuda else None
        if self.alone:
            (scores, ids), = self._posted
            if not self.cuda:
                return (scores.detach().numpy().astype(np.float32, copy=False),
                        ids.detach().numpy().astype(np.int64, copy=False))
            # one pinned D2H per array + one stream sync (pageable .cpu() costs two blocking staged copies)
            hs, hi = self._host_pair()
            hs.copy_(scores, non_blocking=True)
            hi.copy_(ids, non_blocking=True)
            self.mark("d2h_ms")
            stream.synchronize()
            return hs.numpy(), hi.numpy()
        parts = []
        for part, ((a, b), (work, _)) in enumerate(zip(self.cuts, self._posted)):
            if work is not None:
                work.wait()                          # nccl: the current stream waits for the collective; gloo: the host does
            self.mark("gather_ms")
            if self.on_device:
                topk_merge_packed_device(self.gather[part], self.bases, self.merged[0][a:b], self.merged[1][a:b])
                self.mark("merge_ms")
                continue
            gs, gi = unpack_partial(self.gather[part], self.bases.view(self.world, 1, 1))
            if self.cuda:                            # everything crosses PCIe; merged on the host after the sync
                hs, hi = self.stage[part]
                hs.copy_(gs, non_blocking=True)
                hi.copy_(gi, non_blocking=True)
                parts.append((hs.numpy(), hi.numpy()))
                self.mark("d2h_ms")
            else:
                parts.append(topk_merge(gs.numpy(), gi.numpy(), nthreads))
                self.mark("merge_ms")
        self._posted = []
        # the flag is raised after the last collective, never before it (a rank that raised earlier would leave the
        # others waiting); on CUDA it rides along with the result copy and is read after the call's one sync
        if not self.cuda:
            _raise_if_bad(self.flag.item())
        else:
            if self.on_device:
                hs, hi = self._host_pair()
                hs.copy_(self.merged[0], non_blocking=True)
                hi.copy_(self.merged[1], non_blocking=True)
            self.host_flag.copy_(self.flag, non_blocking=True)
            self.mark("d2h_ms")
            stream.synchronize()
            _raise_if_bad(self.host_flag.item())
            if self.on_device:
                return hs.numpy(), hi.numpy()
            parts = [topk_merge(s_, i_, nthreads) for s_, i_ in parts]
        if len(parts) == 1:
            return parts[0]
        return np.concatenate([p_[0] for p_ in parts]), np.concatenate([p_[1] for p_ in parts])


def gather_and_merge(local_scores, local_ids, group=None, nthreads: int = 0, bufs: Optional[dict] = None,
                     merge: str = "auto", force_collective: bool = False, id_bases=None,
                     phases: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray]:
    """All-gather the per-shard partial top-k and merge.  ``merge``: "host" (mrag_topk_merge),
    "device" (mrag_topk_merge_packed_device, CUDA tensors only) or "auto" (device when it applies).

    ``local_scores`` [Q,k] float32 and ``local_ids`` [Q,k] int64 are torch tensors on the
    backend's device (CUDA for nccl, CPU for gloo).  Every rank returns the full merged
    (scores [Q,k] float32, ids [Q,k] int64) as numpy arrays.  ``bufs`` (a dict the caller
    keeps; its content is the exchange's business) keeps the gather / pinned staging buffers across calls; with CUDA
    inputs the returned arrays are views of pinned buffers that stay valid until the call after the next one.
    ``id_bases``: first global row of every rank's shard (needed when more than one rank takes part);
    ids must lie in [id_base, id_base + 2^32 - 1) of their rank -- anything else raises, it never wraps.
    ``phases`` (a dict) receives pack_ms / gather_ms / merge_ms / d2h_ms of this call."""
    bufs = bufs if bufs is not None else {}
    ex = bufs.get("exchange")
    # another group or other bases (another ``n_total`` or shard layout, even with the same world / q / k) never
    # reuse the previous exchange's device copy of the bases
    if ex is None or ex.group is not group or ex.id_bases != _bases_key(id_bases):
        ex = bufs["exchange"] = _Exchange(group, id_bases)
    q, k = local_scores.shape
    ex.begin(q, k, local_scores.device, merge=merge, force_collective=force_collective, timed=phases is not None)
    ex.post(local_scores, local_ids)
    out = ex.collect(nthreads)
    if phases is not None:
        phases.update(ex.phases())
    return out


class _Sharded:
    """What the two sharded indexes share: this rank's row block, the exchange, adding rows."""

    def __init__(self, n_total: int, rank: int, world: int, group):
        self.n_total, self.rank, self.world, self.group = n_total, rank, world, group
        self.lo, self.hi = shard_bounds(n_total, world, rank)
        self._exchange = _Exchange(group, [shard_bounds(n_total, world, r)[0] for r in range(world)])
        self.index = None

    def add_local(self, rows, normalize=None):
        """Append rows of THIS shard (global rows lo + len(index) ...)."""
        self.index.add(rows, normalize=normalize)
        if len(self.index) > self.hi - self.lo:
            raise ValueError("more rows than this shard owns")

    def local_allow(self, allow):
        """Global allow-set (bool / uint8 mask over the ``n_total`` rows, or global row positions) -> this rank's
        local mask over rows ``[lo, hi)`` (numpy bool), as the single-GPU index's ``search`` takes it."""
        return local_allow_mask(allow, self.n_total, self.lo, self.hi)


def _device_of(queries):
    import torch
    return queries.device if torch.is_tensor(queries) else torch.device("cpu")


class ShardedDenseIndex(_Sharded):
    """One rank's view of a row-sharded corpus.

    ``local_search(queries, k) -> (scores, ids)`` defaults to a :class:`DenseIndex` on this
    rank's GPU with ``id_base`` = the shard's first global row; tests inject a CPU searcher
    to exercise the exchange + merge on ``gloo``.  ``fp8_scan=True`` gives that index its fp8 copy, so that
    ``search(..., precision="fp8", refine=...)`` (passed through to the local search) runs the fp8 scan per shard."""

    def __init__(self, dim: int, n_total: int, rank: int, world: int, device: int = 0, group=None,
                 dtype: str = "f16", metric: str = "cosine",
                 local_search: Optional[Callable] = None, fp8_scan: bool = False):
        super().__init__(n_total, rank, world, group)
        self.dim = dim
        self.last_phases: dict = {}
        self._out, self._out_fit = None, None     # device result tensors of the local search, reused across calls
        if local_search is None:
            from .index import DenseIndex
            self.index = DenseIndex(dim, metric=metric, dtype=dtype, device=device, fp8_scan=fp8_scan)
            self.index.set_id_base(self.lo)
            self.index.reserve(self.hi - self.lo)
            local_search = self.index.search
        self._local_search = local_search

    def search(self, queries, k: int, nthreads: int = 0, merge: str = "auto", force_collective: bool = False,
               pipeline: bool = False, allow=None, **kw) -> Tuple[np.ndarray, np.ndarray]:
        """Local search over this rank's rows, then the exchange + merge; every rank returns the full result.
        ``pipeline=True`` cuts the batch in two halves: the all-gather of half A is in flight (``async_op``, on the
        process group's own stream) while the local search of half B runs -- same result, bit for bit (every query's
        answer depends on its own rows of the batch only).  ``self.last_phases`` holds the call's per-phase
        milliseconds: local_ms, pack_ms, gather_ms (in pipeline mode: the part of the collective the local search
        did NOT cover), merge_ms, d2h_ms.
        ``allow`` (global rows: a mask over ``n_total`` or global row positions) restricts the search to those rows:
        every rank searches the allowed rows of its own shard; a rank with none contributes (-inf, -1) slots."""
        import torch
        device = _device_of(queries)
        nq = int(queries.shape[0])
        if allow is not None:
            kw = dict(kw, allow=self.local_allow(allow))
        out = kw.pop("out", None)
        if out is None and self.index is not None and device.type == "cuda":
            if self._out_fit != (nq, int(k), device):       # (they are consumed by the exchange below)
                self._out_fit = (nq, int(k), device)
                self._out = (torch.empty((nq, k), dtype=torch.float32, device=device),
                             torch.empty((nq, k), dtype=torch.int64, device=device))
            out = self._out
        ex = self._exchange
        cuts = ex.begin(nq, k, device, merge=merge, force_collective=force_collective, pipeline=pipeline, timed=True)
        for part, (a, b) in enumerate(cuts):
            kwp = kw if out is None else dict(kw, out=(out[0][a:b], out[1][a:b]))
            sc, ids = self._local_search(queries[a:b] if len(cuts) > 1 else queries, k, **kwp)
            ex.mark("local_ms")
            ex.post(sc, ids, part)
        res = ex.collect(nthreads)
        self.last_phases = ex.phases()
        return res


class ShardedIVFIndex(_Sharded):
    """One rank's view of a row-sharded IVF-flat index (BASELINE config 5): rank r holds rows
    ``shard_bounds(n_total, world, r)`` of EVERY list; the centroids are trained once (rank 0) and broadcast,
    so all ranks probe the same lists and scan equal shares of them; the per-shard top-k meets in the same
    one-collective exchange + merge as the brute-force index.  Result = the single-GPU IVF result for the
    same centroids.

    ``local_search(queries, k, nprobe) -> (scores, ids)`` defaults to an :class:`IVFFlatIndex` on this rank's
    GPU; tests inject a CPU searcher to exercise the exchange on ``gloo``.  A filtered search also calls it with
    ``allow=`` (local mask), ``filter_path=`` ("probe" / "exact") and ``list_allowed=`` (global per-list counts), and
    ``local_list_counts(local_mask) -> int [nlist]`` (default: :meth:`IVFFlatIndex.allowed_per_list`) is injectable the
    same way.  ``fp8_scan=True`` gives the local index its fp8 copy, so that ``search(..., precision="fp8", refine=...)``
    (passed through to the local search as ``precision=`` / ``refine=``) runs the fp8 scan per shard."""

    def __init__(self, dim: int, nlist: int, n_total: int, rank: int, world: int, device: int = 0, group=None,
                 dtype: str = "f16", metric: str = "cosine", local_search: Optional[Callable] = None,
                 local_list_counts: Optional[Callable] = None, fp8_scan: bool = False):
        super().__init__(n_total, rank, world, group)
        self.dim, self.nlist = dim, nlist
        if local_search is None:
            from .index import IVFFlatIndex
            self.index = IVFFlatIndex(dim, nlist, metric=metric, dtype=dtype, device=device, fp8_scan=fp8_scan)
            self.index.set_id_base(self.lo)
            local_search = self.index.search
            if local_list_counts is None:
                local_list_counts = self.index.allowed_per_list
        self._local_search = local_search
        self._local_list_counts = local_list_counts

    def train(self, sample_rows, iters: int = 10, seed: int = 0, normalize=None):
        """k-means on rank 0 (``sample_rows`` is ignored elsewhere), centroids broadcast to every rank."""
        import torch
        import torch.distributed as dist
        cen = None
        if self.rank == 0:
            self.index.train(sample_rows, iters=iters, seed=seed, normalize=normalize)
            cen = self.index.centroids()
        if self.world > 1:
            dev = torch.device("cuda", self.index.device) if dist.get_backend(self.group) == "nccl" else torch.device("cpu")
            t = torch.from_numpy(cen).to(dev) if self.rank == 0 else torch.empty((self.nlist, self.dim), dtype=torch.float32, device=dev)
            dist.broadcast(t, src=0, group=self.group)
            if self.rank != 0:
                self.index.set_centroids(t.cpu().numpy(), normalize=False)     # already normalised + rounded
        return self

    def set_centroids(self, centroids, normalize=None):
        self.index.set_centroids(centroids, normalize=normalize)

    def global_list_counts(self, local_mask) -> np.ndarray:
        """Allowed rows per list summed over the ranks (int32 [nlist], host): this rank's counts, all-reduced."""
        import torch
        import torch.distributed as dist
        c = self._local_list_counts(local_mask)
        c = c.cpu().numpy() if torch.is_tensor(c) else np.asarray(c)
        t = torch.from_numpy(np.ascontiguousarray(c, dtype=np.int64))
        if dist.is_initialized() and dist.get_world_size(self.group) > 1:
            if dist.get_backend(self.group) == "nccl":
                t = t.to(torch.device("cuda", self.index.device if self.index is not None else torch.cuda.current_device()))
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t.cpu().numpy().astype(np.int32)

    def search(self, queries, k: int, nprobe: int, nthreads: int = 0, merge: str = "auto",
               force_collective: bool = False, allow=None, filter_path: str = "auto", precision: str = "exact",
               refine: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """Local search over this rank's rows, then the exchange + merge; every rank returns the full result.
        ``allow`` (global rows: a mask over ``n_total`` or global row positions) restricts the search to those rows,
        with the semantics of :meth:`IVFFlatIndex.search`: every rank takes its slice, the per-list allowed counts are
        summed over the ranks so that all ranks agree on the live lists, and the path ("auto": decided once, from the
        global counts) is passed explicitly to every rank.  Result = the single-index filtered result.
        ``precision="fp8"`` / ``refine`` (see :meth:`IVFFlatIndex.search`; not with ``allow``) go to the local search
        unchanged: every rank picks and re-ranks the ``refine`` candidates of its OWN rows, and the exchange merges the
        exact-scored results.  The ranks together re-rank up to ``world x refine`` candidates per query, so a multi-rank
        answer can only contain more true neighbours than the one-index fp8 answer; it is not identical to it."""
        fp8, _ = _check_precision(precision, refine, allow)
        kw = dict(precision=precision, refine=refine) if fp8 else {}
        if allow is not None:
            from .index import IVF_FILTER_PATHS, ivf_choose_filter_path
            if filter_path not in IVF_FILTER_PATHS:
                raise ValueError(f"filter_path must be one of {sorted(IVF_FILTER_PATHS)}, got {filter_path!r}")
            local = self.local_allow(allow)
            counts = self.global_list_counts(local)
            if filter_path == "auto":
                filter_path = ivf_choose_filter_path(int(queries.shape[0]), k, nprobe, self.nlist, self.n_total,
                                                     int(counts.sum(dtype=np.int64)), self.dim)
            kw = dict(allow=local, filter_path=filter_path, list_allowed=counts)
        ex = self._exchange
        ex.begin(int(queries.shape[0]), k, _device_of(queries), merge=merge, force_collective=force_collective)
        ex.post(*self._local_search(queries, k, nprobe, **kw))
        return ex.collect(nthreads)
