"""Shared case builders of the batched dense re-rank tests (``mrag_index_score_rows_batch``): the index cases, the
batch structures and the two numpy restatements of a row's fp64 sum.  No kernel runs here; tests/test_rerank_batch_host.py
checks on the CPU that the cases can see what they are built to see, tests/test_gpu_rerank_batch.py runs them.
"""
import numpy as np

R = 64                    # rows per descriptor (RERANK_ROWS of csrc/bf_kernels.h): list lengths straddle it
N_ROWS = 700              # stored rows of every index case
REG_LD = 1024             # widest row whose query columns the kernel keeps in registers
DIMS = (64, 200, 768, 1100)            # one tile; not a multiple of 64; the reference's dim; above the register-held width
DTYPES = ("f16", "bf16")
KINDS = ("cosine", "wide")             # rows through K1 | un-normalised rows with a 2^22 spread of column scales
INDEX_CASES = [(dim, dtype, kind) for dim in DIMS for dtype in DTYPES for kind in KINDS]
LENGTHS = (0, 1, R - 1, R, R + 1, 200, 4 * R + 1)


def case_id(case):
    return "d%d-%s-%s" % case


def wide_scale(dim):
    """column j scaled by 2**((7 j) % 23 - 11): partial sums of very different magnitude, so that the order of an fp64
    accumulation shows in the float32 result"""
    return np.exp2(((np.arange(dim) * 7) % 23 - 11).astype(np.float64)).astype(np.float32)


N_CANCEL = 100            # the last rows of a wide case: cancelling rows (below)


def anchor_query(dim, kind, seed=23):
    """the query the cancelling rows are built against; every structure asks it once (``structure_queries``)"""
    q = np.random.default_rng(seed + dim).standard_normal(dim).astype(np.float32)
    return q * wide_scale(dim) if kind == "wide" else q


def cancelling_rows(dim, dtype, n=N_CANCEL, seed=31):
    """Rows whose score against the anchor query depends on the ORDER of the fp64 sum.  Random rows do not: the products
    of two 16-bit values have at most 22 significant bits, an fp64 sum of a few hundred of them is off by some 1e-16 of
    its largest term in any order, and the float32 rounding of the result hides that.  So each of these rows holds three
    column pairs (j, k) with x_j = s q_k, x_k = -s q_j (s a power of two: exact in the storage type) -- two products of
    some 2^24 that cancel EXACTLY -- and two columns of some 2^-10 that carry the result.  Whether a small term is added
    before, between or after a pair decides which of its bits survive, and that is visible in float32."""
    rng = np.random.default_rng(seed + dim)
    q = round_storage(anchor_query(dim, "wide"), dtype)
    exp = (np.arange(dim) * 7) % 23 - 11
    big, small = np.flatnonzero((exp >= 0) & (q != 0)), np.flatnonzero(exp <= -8)
    x = np.zeros((n, dim), dtype=np.float64)
    for r in range(n):
        cols = rng.choice(big, size=6, replace=False)
        for j, k in cols.reshape(3, 2):
            s = np.exp2(12 - np.ceil(np.log2(max(abs(q[j]), abs(q[k])))))
            x[r, j], x[r, k] = s * q[k], -s * q[j]
        m = rng.choice(small, size=2, replace=False)
        x[r, m] = round_storage(rng.standard_normal(2) * np.exp2(exp[m]), dtype)
    return x.astype(np.float32)


def make_rows(dim, kind, dtype="f16", n=N_ROWS, seed=11):
    x = np.random.default_rng(seed + dim).standard_normal((n, dim)).astype(np.float32)
    if kind != "wide":
        return x
    x *= wide_scale(dim)[None, :]
    x[n - N_CANCEL:] = cancelling_rows(dim, dtype)
    return x


def make_queries(dim, kind, nq, seed=23):
    q = np.random.default_rng(seed + dim + nq).standard_normal((nq, dim)).astype(np.float32)
    return q * wide_scale(dim)[None, :] if kind == "wide" else q


def normalize_flag(kind):
    """``normalize`` of add and of the score calls: K1's cosine preparation, or the values as they are"""
    return kind == "cosine"


def structures(n=N_ROWS, seed=5):
    """name -> list of int64 id arrays, one per question"""
    rng = np.random.default_rng(seed)

    def ids(k):
        return rng.integers(0, n, size=k).astype(np.int64)

    out = {}
    out["one question, the reference's pool"] = [ids(200)]
    out["two questions around a descriptor"] = [ids(R - 1), ids(R + 1)]
    out["five questions, empty first and last"] = [ids(0), ids(1), ids(R), ids(4 * R + 1), ids(0)]
    out["all questions empty"] = [ids(0) for _ in range(5)]
    # every length, ids outside the index, an id repeated inside a question and across questions
    q33 = [ids(LENGTHS[g % len(LENGTHS)]) for g in range(33)]
    q33[1] = np.asarray([-1], dtype=np.int64)
    q33[2][[0, 5, R - 2]] = (n, 17, 17)
    q33[3][[1, 2, R - 1]] = (17, -1, 17)
    q33[5][[0, 64, 128, 199]] = (n, 17, -1, n + 5)
    q33[6][[0, 4 * R]] = (17, 2 ** 40)
    out["thirty-three questions of every length"] = q33
    skew = [ids(3) for _ in range(33)]
    skew[20] = ids(5000)
    out["one list of 5000 among lists of 3"] = skew
    big = [ids(int(k)) for k in rng.integers(0, 41, size=1000)]
    big[0] = ids(R + 7)
    out["a thousand questions"] = big
    # the anchor question of every structure (the first with 8 ids or more) asks for cancelling rows too
    for lists in out.values():
        g = anchor_question(lists)
        if g is not None:
            k = min(len(lists[g]) // 2, 40)
            lists[g][:k] = rng.integers(n - N_CANCEL, n, size=k)
    big[500], big[999] = big[0].copy(), big[0].copy()          # the same (query, ids) first, in the middle and last
    return out


SAME_AT = (0, 500, 999)                # of "a thousand questions": queries and ids are equal at these positions


def anchor_question(lists):
    return next((g for g, x in enumerate(lists) if len(x) >= 8), None)


def structure_queries(dim, kind, name, lists):
    q = make_queries(dim, kind, len(lists))
    g = anchor_question(lists)
    if g is not None:
        q[g] = anchor_query(dim, kind)
    if name == "a thousand questions":
        q[SAME_AT[1]] = q[SAME_AT[2]] = q[SAME_AT[0]]
    return q


def to_csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    flat = np.concatenate(lists).astype(np.int64) if lists else np.zeros(0, dtype=np.int64)
    return ptr, flat


# ---- the storage rounding and the two orders of the fp64 sum ---------------------------------------------------------
def round_storage(x, dtype):
    """float32 -> the storage type and back (round to nearest even), as float64"""
    x = np.asarray(x, dtype=np.float32)
    if dtype == "f16":
        return x.astype(np.float16).astype(np.float64)
    b = x.view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def products(rows16, q16):
    """the exact fp64 products of each row with the query, zero padded to the row pitch (a multiple of 64)"""
    p = rows16 * q16[None, :]
    ld = (p.shape[1] + 63) // 64 * 64
    return np.concatenate([p, np.zeros((p.shape[0], ld - p.shape[1]))], axis=1)


def sum_kernel_order(p):
    """the single kernel's order: lane l takes columns l, l + 64, ... one after the other; then the xor butterfly at 32 .. 1"""
    acc = np.zeros((p.shape[0], 64))
    for i in range(p.shape[1] // 64):
        acc = acc + p[:, 64 * i:64 * i + 64]
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ off]
    return acc[:, 0].astype(np.float32)


def sum_left_to_right(p):
    s = np.zeros(p.shape[0])
    for c in range(p.shape[1]):
        s = s + p[:, c]
    return s.astype(np.float32)
