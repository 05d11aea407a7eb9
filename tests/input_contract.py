"""The input contract of include/rs_simplify.h as test material (no GPU needed):

  permutations   the rows of chosen blocks with their (col, val) pairs permuted together -- "within a
                 row the columns must be distinct; order is free";
  validator      a plain-Python restatement of what the header requires of an rs_input;
  defects        one function per class of malformed input, each applied to one block of a valid holder;
  uncertain rows the certificate of how many linear rows k_lin_keyframes cannot settle from keys alone,
                 and a gadget that builds exactly n of them (the keys-first boundary unc_cap of run.hpp);
  edge values    per prime, coefficients on the carry and limb edges of field.hpp, and a rewrite of a
                 gen_system result that draws every coefficient from them.

tests/test_input_contract.py proves these on the CPU; tests/test_gpu_input_contract.py runs them through
the library's entry points against the oracle on the canonical form (same rows, keys ascending)."""
from __future__ import annotations

import ctypes as C
import random
import struct
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

import dispatch_shapes as ds
import rsio

R = rsio.R
BLOCKS = ("cons_eq", "eq", "linear", "nl_a", "nl_b", "nl_c")
CE, EQ, LIN, NLA, NLB, NLC = range(6)
KINDS = ("reversed", "random", "rotate1", "swap_last_pair", "le_bytes")
F257, F97 = 257, 97
_ID_PRIME = {v: k for k, v in rsio.PRIME_IDS.items()}


# ============================================================================ holders
def _relink(h: "rsio.InputHolder") -> None:
    """Points h.inp at h's arrays (after they were replaced)."""
    for b in h.blocks:
        b.lc.ptr = b.ptr.ctypes.data_as(C.POINTER(C.c_uint64))
        b.lc.col = b.col.ctypes.data_as(C.POINTER(C.c_uint32))
        b.lc.val = b.val.ctypes.data_as(C.POINTER(C.c_uint64))
    h.inp.forbidden = h.forb.ctypes.data_as(C.POINTER(C.c_uint32))
    h.inp.cons_eq, h.inp.eq, h.inp.linear, h.inp.nl_a, h.inp.nl_b, h.inp.nl_c = [b.lc for b in h.blocks]


def copy_holder(h: "rsio.InputHolder") -> "rsio.InputHolder":
    """A deep copy: its own arrays, its own rs_input."""
    g = object.__new__(rsio.InputHolder)
    g.blocks = []
    for b in h.blocks:
        nb = object.__new__(rsio._Block)
        nb.ptr, nb.col, nb.val = b.ptr.copy(), b.col.copy(), b.val.copy()
        nb.lc = rsio.RsLc(b.lc.n_rows, b.lc.nnz, None, None, None)
        g.blocks.append(nb)
    g.forb = h.forb.copy()
    g.inp = rsio.RsInput.from_buffer_copy(h.inp)
    _relink(g)
    return g


def prime_of(h: "rsio.InputHolder") -> int:
    if h.inp.prime_id == 255:
        return sum(int(h.inp.prime[i]) << (64 * i) for i in range(4))
    return R.PRIMES[_ID_PRIME[int(h.inp.prime_id)]]


def rows_of(b, r: int) -> Tuple[int, int]:
    return int(b.ptr[r]), int(b.ptr[r + 1])


def not_ascending(b) -> int:
    """Rows of the block whose keys are not strictly ascending."""
    n = 0
    for r in range(int(b.lc.n_rows)):
        s, e = rows_of(b, r)
        k = b.col[s:e].astype(np.int64)
        n += bool((np.diff(k) <= 0).any())
    return n


# ============================================================================ permutations
def _le_key(k: int) -> bytes:
    return struct.pack("<I", int(k))


def _order(kind: str, keys: np.ndarray, rng: random.Random) -> List[int]:
    """Positions of the row's entries in their new order; `keys` are the row's keys as given."""
    asc = sorted(range(len(keys)), key=lambda i: int(keys[i]))
    m = len(asc)
    if kind == "reversed":
        return asc[::-1]
    if kind == "random":
        o = list(asc)
        rng.shuffle(o)
        return o
    if kind == "rotate1":          # the smallest key last
        return asc[1:] + asc[:1]
    if kind == "swap_last_pair":
        return asc[:-2] + [asc[-1], asc[-2]] if m >= 2 else asc
    if kind == "le_bytes":         # the order of an .r1cs file: by the key's little-endian byte string
        return sorted(range(m), key=lambda i: _le_key(keys[i]))
    if kind == "sorted":
        return asc
    raise ValueError(kind)


def permute(h: "rsio.InputHolder", kind: str, blocks: Sequence[int], seed: int = 0):
    """-> (a copy of h whose `blocks` have every row's (col, val) pairs reordered by `kind`,
    {block: rows that ended up not ascending})."""
    g = copy_holder(h)
    rng = random.Random(seed)
    count = {}
    for q in blocks:
        b = g.blocks[q]
        v = b.val.reshape(-1, 4)
        for r in range(int(b.lc.n_rows)):
            s, e = rows_of(b, r)
            if e - s < 2:
                continue
            o = [s + i for i in _order(kind, b.col[s:e], rng)]
            b.col[s:e] = b.col[o]
            v[s:e] = v[o]
        count[q] = not_ascending(b)
    return g, count


def canonical(h: "rsio.InputHolder") -> "rsio.InputHolder":
    """The canonical form: the same rows, keys ascending."""
    return permute(h, "sorted", range(6))[0]


def same_arrays(x: "rsio.InputHolder", y: "rsio.InputHolder") -> bool:
    return all(np.array_equal(getattr(a, f), getattr(b, f)) and a.lc.nnz == b.lc.nnz and a.lc.n_rows == b.lc.n_rows
               for a, b in zip(x.blocks, y.blocks) for f in ("ptr", "col", "val")) and np.array_equal(x.forb, y.forb)


# ============================================================================ the validator model
def invalid(h: "rsio.InputHolder") -> Optional[str]:
    """None when the holder's rs_input keeps the header's contract, else the first reason it does not."""
    inp = h.inp
    S = int(inp.max_signal)
    p = prime_of(h)
    if not 0 < S <= 0x7FFFFFFF:
        return "max_signal"
    forb = [int(f) for f in h.forb[: int(inp.n_forbidden)]]
    if any(f >= S for f in forb):
        return "forbidden id out of range"
    if 0 not in forb:
        return "signal 0 must be forbidden"
    if not (h.blocks[NLA].lc.n_rows == h.blocks[NLB].lc.n_rows == h.blocks[NLC].lc.n_rows):
        return "non-linear blocks differ in row count"
    for nm, b in zip(BLOCKS, h.blocks):
        n, nnz = int(b.lc.n_rows), int(b.lc.nnz)
        if n == 0:
            continue
        ptr = [int(x) for x in b.ptr[: n + 1]]
        if ptr[0] != 0:
            return f"{nm}: ptr[0] != 0"
        if any(ptr[r + 1] < ptr[r] for r in range(n)):
            return f"{nm}: decreasing row pointer"
        if ptr[n] != nnz:
            return f"{nm}: ptr[n] != nnz"
        for r in range(n):
            keys = [int(k) for k in b.col[ptr[r]:ptr[r + 1]]]
            if any(k >= S for k in keys):
                return f"{nm}: key >= max_signal in row {r}"
            if len(set(keys)) != len(keys):
                return f"{nm}: duplicate key in row {r}"
            for e in range(ptr[r], ptr[r + 1]):
                v = sum(int(b.val[4 * e + i]) << (64 * i) for i in range(4))
                if v == 0:
                    return f"{nm}: zero value in row {r}"
                if v >= p:
                    return f"{nm}: value >= p in row {r}"
    return None


# ============================================================================ defects
def _set_val(b, e: int, v: int) -> None:
    for i in range(4):
        b.val[4 * e + i] = (v >> (64 * i)) & rsio.U64_MAX


def _row_with(b, lo: int, hi: int = 1 << 62, last=False) -> Optional[int]:
    """A row of the block with lo <= entries <= hi (the first, or the last)."""
    rows = range(int(b.lc.n_rows))
    for r in (reversed(rows) if last else rows):
        s, e = rows_of(b, r)
        if lo <= e - s <= hi:
            return r
    return None


def _value_defect(value_of: Callable[[int], Optional[int]]):
    def apply(h, q) -> bool:
        b = h.blocks[q]
        v = value_of(prime_of(h))
        r = _row_with(b, 1, last=True)      # the last row that holds an entry: its last entry
        if v is None or r is None:
            return False
        _set_val(b, rows_of(b, r)[1] - 1, v)
        return True
    return apply


def _key_defect(key_of: Callable[["rsio.InputHolder"], int]):
    def apply(h, q) -> bool:
        b = h.blocks[q]
        r = _row_with(b, 1, last=True)
        if r is None:
            return False
        b.col[rows_of(b, r)[1] - 1] = key_of(h)
        return True
    return apply


def _dup_adjacent(h, q) -> bool:
    b = h.blocks[q]
    r = _row_with(b, 2)
    if r is None:
        return False
    s, _ = rows_of(b, r)
    b.col[s + 1] = b.col[s]                 # the row stays non-decreasing
    return True


def _dup_apart(lo: int, hi: int):
    def apply(h, q) -> bool:
        b = h.blocks[q]
        r = _row_with(b, lo, hi)
        if r is None:
            return False
        s, e = rows_of(b, r)
        v = b.val.reshape(-1, 4)
        b.col[s:e] = b.col[s:e][::-1].copy()     # unsorted: descending
        v[s:e] = v[s:e][::-1].copy()
        b.col[e - 1] = b.col[s]                  # the largest key again at the other end of the row
        return True
    return apply


def _ptr0(h, q) -> bool:
    b = h.blocks[q]
    if int(b.lc.n_rows) < 1:
        return False
    b.ptr[0] = 1
    return True


def _ptr_decreasing(h, q) -> bool:
    b = h.blocks[q]
    if int(b.lc.n_rows) < 3:
        return False
    b.ptr[1] = b.ptr[2] + 1                       # ptr[2] < ptr[1]: a wrapped row length without the check
    return True


def _ptr_end(h, q) -> bool:
    b = h.blocks[q]
    if int(b.lc.n_rows) < 1:
        return False
    b.ptr[int(b.lc.n_rows)] += 1                  # ptr[n] != nnz
    return True


def sort_insert_max() -> int:
    return ds.constant("kSortInsertMax")


# name -> apply(holder, block) -> bool (False: the block has no place for this defect).  A defect is
# applied in place to a copy the caller made.
DEFECTS: Dict[str, Callable] = {
    "zero_value": _value_defect(lambda p: 0),
    "value_eq_p": _value_defect(lambda p: p),
    "value_all_ones": _value_defect(lambda p: (1 << 256) - 1),
    # only limb 1 set: 2^64, not canonical for the primes under 2^64 (a one-word product reads limb 0 alone)
    "value_limb1": _value_defect(lambda p: (1 << 64) if p < (1 << 64) else None),
    "key_eq_max_signal": _key_defect(lambda h: int(h.inp.max_signal)),
    "key_ffffffff": _key_defect(lambda h: 0xFFFFFFFF),
    "dup_adjacent_sorted": _dup_adjacent,
    "dup_apart_short": lambda h, q: _dup_apart(3, sort_insert_max())(h, q),
    "dup_apart_long": lambda h, q: _dup_apart(sort_insert_max() + 1, 1 << 62)(h, q),
    "ptr0_nonzero": _ptr0,
    "ptr_decreasing": _ptr_decreasing,
    "ptr_end_ne_nnz": _ptr_end,
}
VALUE_DEFECTS = ("zero_value", "value_eq_p", "value_all_ones", "value_limb1")


def defect(h: "rsio.InputHolder", name: str, q: int) -> Optional["rsio.InputHolder"]:
    """A copy of h with defect `name` in block q, or None when the block has no place for it."""
    g = copy_holder(h)
    return g if DEFECTS[name](g, q) else None


def defect_blocks(name: str, p: int) -> Tuple[int, ...]:
    """The blocks of lengths_system(p) that have a place for defect `name`: all six, but the unsorted
    duplicates need a row of three entries or more (cons_eq and eq have none), and 2^64 is a canonical
    value for a prime above it."""
    if name == "value_limb1" and p >= (1 << 64):
        return ()
    if name.startswith("dup_apart"):
        return (LIN, NLA, NLB, NLC)
    return tuple(range(6))


# ============================================================================ a system of given row lengths
def row_lengths() -> List[int]:
    k = sort_insert_max()
    return [1, 2, 3, k - 1, k, k + 1, 64, 65, 200]


def lengths_system(p: int, seed: int = 5) -> "R.System":
    """Rows of every length of row_lengths() in `linear` (from 2 on: a one-entry row is a constant
    equality) and in each of nl_a, nl_b, nl_c (some nl_c rows empty), over 700 signals, so that ids pass
    255 and the little-endian byte order of an .r1cs file differs from the ascending one.  Also constant
    equalities, equalities that rename, and equalities with both ends forbidden that form a cluster of
    their own (the rows rs_engine_simplify keeps with values from the host input)."""
    rng = random.Random(seed)
    S = 700
    forb = {0, 1, 2, 3} | set(range(600, 640))
    free = [s for s in range(9, S) if s not in forb]

    def coef():
        return rng.choice((1, p - 1, 2 % p or 1, rng.randrange(1, p)))

    def lc(n, const=False):
        m = {s: coef() for s in rng.sample(free, n - (1 if const else 0))}
        if const:
            m[0] = coef()
        return m

    rows: List["R.Con"] = []
    lens = row_lengths()
    for rep in range(2):
        for n in lens:
            if n >= 3:
                rows.append(R.Con({}, {}, lc(n, const=bool(rep))))
            elif n == 2:
                x, y = rng.sample(free, 2)
                rows.append(R.Con({}, {}, {x: 2 % p or 1, y: 1} if p > 3 else {x: 1, y: 1}))
    for i, n in enumerate(lens):          # each length in A, in B and in C, against short other parts
        for part in range(3):
            a, b, c = lc(2), lc(2, const=True), (lc(2) if i % 2 else {})
            big = lc(n, const=(n > 2 and i % 2 == 1))
            if part == 0:
                a = big
            elif part == 1:
                b = big
            else:
                c = big
            rows.append(R.Con(a, b, c))
    for i in range(12):                   # constant equalities x = c, with and without a constant
        m = {rng.choice(free): coef()}
        if i % 2:
            m[0] = coef()
        rows.append(R.Con({}, {}, m))
    for i in range(20):                   # renaming equalities
        x, y = rng.sample(free, 2)
        k = coef()
        rows.append(R.Con({}, {}, {x: k, y: (p - k) % p}))
    for i in range(6):                    # both ends forbidden, each a cluster of its own
        k = coef()
        rows.append(R.Con({}, {}, {600 + 2 * i: k, 601 + 2 * i: (p - k) % p}))
    rows.append(R.Con({}, {}, {620: 1, rng.choice(free): p - 1}))  # one forbidden end: renames the other
    rng.shuffle(rows)
    return R.System(p, S, 1, 2, 5, forb, rows)


# ============================================================================ keys-first: uncertain rows
def unc_cap(n_linear: int) -> int:
    """run.hpp's unc_cap for a linear block of n_linear rows."""
    return max(ds.constant("kUncMin"), n_linear // ds.constant("kUncDiv"))


def uncertain_rows(sys_: "R.System") -> int:
    """How many linear rows k_lin_keyframes flags: after the eq renaming and without the keys the
    constant equalities define, two keys of the row are the same signal (their coefficients may
    cancel), or no non-constant key is left (whether the row is empty depends on its constant)."""
    _, _, single, const_subs = ds.linear_after_frames(sys_)
    _, _, lin, _ = R.classify(sys_)
    n = 0
    for c in lin:
        seen, dup = set(), False
        for k in c.c:
            e = single.get(k)
            if e is not None:
                assert e.kind == "Signal"
                k = e.symbol
            if k == 0 or k in const_subs:
                continue
            dup |= k in seen
            seen.add(k)
        n += bool(dup or not seen)
    return n


def uncertain_gadget(n_dup: int, n_const: int, p: int, seed: int = 1, chain_rows: int = 40) -> "R.System":
    """Exactly n_dup linear rows whose keys a and b an equality k a - k b renames to one signal (next to
    a forbidden one; in every third row the coefficients of a and b cancel), exactly n_const rows over
    x and y with x = 3, y = 5 (+ a constant; in every second row the constant term sums to zero), and
    a chain of ordinary rows with probes."""
    b = ds.Builder(seed, p)
    for i in range(n_dup):
        x, y = b.take(2)
        f = b.forbid(1)[0]
        k = b.coef()
        b.rows.append(R.Con({}, {}, {x: k, y: (p - k) % p}))
        cx = b.coef()
        cy = (p - cx) % p if i % 3 == 0 else (cx + 1) % p or 1
        b.rows.append(R.Con({}, {}, {x: cx, y: cy, f: b.coef()}))
        b.n_lin += 1
    for i in range(n_const):
        x, y = b.take(2)
        b.rows.append(R.Con({}, {}, {x: 1, 0: (p - 3) % p}))
        b.rows.append(R.Con({}, {}, {y: 1, 0: (p - 5) % p}))
        cx, cy = b.coef(), b.coef()
        s = (3 * cx + 5 * cy) % p
        c0 = (p - s) % p if i % 2 == 0 else (p - s + 1) % p
        if c0 == 0:                          # (tiny primes) a row without a constant is not linear here
            c0 = 1
        b.rows.append(R.Con({}, {}, {0: c0, x: cx, y: cy}))
        b.n_lin += 1
    cl = ds.chain(b, chain_rows)
    b.probes(cl["probe"])
    return b.system()


def plain_system(p: int, seed: int = 2) -> "R.System":
    """No uncertain row: chains with probes."""
    b = ds.Builder(seed, p)
    for n in (40, 12):
        b.probes(ds.chain(b, n)["probe"])
    return b.system()


# ============================================================================ edge coefficients
EDGE_K = (29, 58, 63, 64, 116, 128, 192, 232, 255)


def edge_coefficients(p: int) -> List[int]:
    """Values on the carry and limb edges of the field arithmetic, in (0, p), ascending."""
    vals = {1, 2, p - 1, p - 2, (p + 1) // 2, (p - 1) // 2}
    for k in EDGE_K:
        for d in (-1, 0, 1):
            v = (1 << k) + d
            vals |= {v, p - v}
    ones = (1 << 64) - 1
    for mask in range(1, 16):
        vals.add(sum(ones << (64 * i) for i in range(4) if mask >> i & 1) % p)
    return sorted(v for v in vals if 0 < v < p)


def edge_system(seed: int, p: int, **kw) -> "R.System":
    """rsio.gen_system(seed, p, **kw) with every coefficient redrawn from edge_coefficients(p);
    equalities stay equalities (k, -k)."""
    sys_ = rsio.gen_system(seed, p, **kw)
    rng = random.Random(seed * 7919 + 13)
    E = edge_coefficients(p)
    rows = []
    for c in sys_.rows:
        if R.is_equality(c, p):
            x, y = list(c.c)
            k = rng.choice(E)
            rows.append(R.Con({}, {}, {x: k, y: p - k}))
        else:
            rows.append(R.Con(*({s: rng.choice(E) for s in m} for m in (c.a, c.b, c.c))))
    return R.System(p, sys_.max_signal, sys_.n_pub_out, sys_.n_pub_in, sys_.n_priv_in, set(sys_.forbidden), rows)


# ============================================================================ the order-is-free cases
def order_cases(le_bytes: bool) -> List[Tuple[str, Tuple[int, ...]]]:
    """(kind, blocks) pairs: every kind on each block alone and on all six together.  Rows of cons_eq and
    eq have at most two entries, which know one other order: `reversed` alone there.  le_bytes only for
    systems whose ids pass 255 (below, the little-endian order is the ascending one), and never on
    cons_eq: key 0 sorts first in both orders."""
    out = []
    for kind in KINDS:
        if kind == "le_bytes" and not le_bytes:
            continue
        for q in range(6):
            if q in (CE, EQ) and kind != "reversed":
                continue
            out.append((kind, (q,)))
        out.append((kind, (EQ, LIN, NLA, NLB, NLC) if kind == "le_bytes" else tuple(range(6))))
    return out
