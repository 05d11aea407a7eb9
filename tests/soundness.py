"""Oracle-free soundness check of a simplification result, and a generator of satisfiable systems.

A simplifier that only substitutes linearly must hand back output rows and a substitution log that
together say exactly what the input said.  `check` proves that for one result with Python big ints
and none of the oracle's algebra (oracle/pyref.py's apply_substitution, fix_constraint, ... are never
called here: only its Con / Sub / System containers are read), so a misreading of the reference that
pyref, refcpu and the kernels share still shows.  The same check runs on the engine's own output.

The six checks, each raising Unsound with its own name:

  log          the first entry per signal defines it, no forbidden signal is defined, the
               definitions resolve through each other without a cycle; a later entry for a signal
               that is already defined is kept as the extra equation `from - to = 0`
  forward      every input row, with the resolved definitions substituted and A*B - C expanded to a
               sparse polynomial over the monomials (i, j), i <= j, 0 the constant, reduces to zero
               against the row echelon form over F_p of the output rows; so do the extra equations
  reverse      every output row reduces to zero against the echelon form of the substituted input
               rows.  forward + reverse: the two spans are equal, which is exact equivalence for a
               simplifier whose only move is a linear substitution
  no leak      no defined signal occurs in an output row
  witness map  signal_map's keys are the forbidden signals plus the signals of the output rows, its
               values their ranks (rebuild_witness, constraint_simplification.rs:101-124: a stable
               compaction, 0 -> 0); no_private_inputs_witness counts the private inputs with a wire
  witnesses    (when given) every output row and every log entry holds on each witness: the cheap
               check where the echelon forms cost too much.  Over F_257 a wrong row passes one
               witness with probability 1/257, hence at least 4 of them

The witness-map check is stricter than the reference in one corner: the reference keeps the wire of
a signal that sat in a non-linear row after round 1 and left every row in a later round (its
non_linear_map is never pruned, constraint_simplification.rs:603-609, :637, read at :113).  No
gen_circuit case of the suites does that; test_soundness.py's census pins the two gen_system runs
that do.

What this does not prove: the reference's choice of WHICH signal a row eliminates and the order of
the output rows.  Those stay pinned by oracle parity only.
"""
from __future__ import annotations

import random
import re
from typing import Dict, Iterable, List, Sequence, Tuple

import rsio

R = rsio.R
Poly = Dict[Tuple[int, int], int]
CHECKS = ("log", "forward", "reverse", "no leak", "witness map", "witnesses")


class Unsound(AssertionError):
    def __init__(self, check: str, msg: str):
        super().__init__(f"[{check}] {msg}")
        self.check = check


# --------------------------------------------------------------------------- the result's form
def as_result(res):
    """(constraints, signal_map, no_private_inputs_witness, log as [(from, {signal: value})]) of a
    pyref Result or of such a tuple (log entries may be pyref Subs)."""
    if hasattr(res, "constraints"):
        res = (res.constraints, res.signal_map, res.no_private_inputs_witness, res.log)
    cons, sm, npiw, log = res
    log = [(s.frm, dict(s.to)) if hasattr(s, "frm") else (int(s[0]), dict(s[1])) for s in log]
    return list(cons), dict(sm), int(npiw), log


# --------------------------------------------------------------------------- sparse algebra over F_p
def _nz(m: Dict[int, int], p: int) -> Dict[int, int]:
    out = {}
    for k, v in m.items():
        v %= p
        if v:
            out[k] = v
    return out


def _subst_lc(m: Dict[int, int], defs: Dict[int, Dict[int, int]], p: int) -> Dict[int, int]:
    """The linear combination m with every defined signal replaced by its resolved definition."""
    out: Dict[int, int] = {}
    for k, v in m.items():
        d = defs.get(k)
        if d is None:
            out[k] = (out.get(k, 0) + v) % p
        else:
            for k2, v2 in d.items():
                out[k2] = (out.get(k2, 0) + v * v2) % p
    return {k: v for k, v in out.items() if v}


def _poly(a: Dict[int, int], b: Dict[int, int], c: Dict[int, int], p: int) -> Poly:
    """A*B - C as {(i, j): coefficient}, i <= j; a linear term x is (0, x), the constant (0, 0)."""
    out: Poly = {}
    for ka, va in a.items():
        for kb, vb in b.items():
            mono = (ka, kb) if ka <= kb else (kb, ka)
            out[mono] = (out.get(mono, 0) + va * vb) % p
    for k, v in c.items():
        out[(0, k)] = (out.get((0, k), 0) - v) % p
    return {k: v for k, v in out.items() if v}


def row_poly(con, defs: Dict[int, Dict[int, int]], p: int) -> Poly:
    return _poly(_subst_lc(con.a, defs, p), _subst_lc(con.b, defs, p), _subst_lc(con.c, defs, p), p)


class Echelon:
    """Row echelon form over F_p of sparse polynomials; the leading monomial of a row is its largest."""

    def __init__(self, p: int):
        self.p = p
        self.rows: Dict[Tuple[int, int], Poly] = {}   # leading monomial -> row, leading coefficient 1

    def reduce(self, poly: Poly) -> Poly:
        """The remainder of poly: empty iff poly lies in the span of the rows."""
        p = self.p
        poly = dict(poly)
        rest: Poly = {}
        while poly:
            lead = max(poly)
            c = poly.pop(lead)
            row = self.rows.get(lead)
            if row is None:
                rest[lead] = c
                continue
            for k, v in row.items():
                if k != lead:
                    nv = (poly.get(k, 0) - c * v) % p
                    if nv:
                        poly[k] = nv
                    else:
                        poly.pop(k, None)
        return rest

    def add(self, poly: Poly) -> bool:
        """Adds poly to the span; False if it was already inside."""
        rest = self.reduce(poly)
        if not rest:
            return False
        lead = max(rest)
        inv = pow(rest[lead], -1, self.p)
        self.rows[lead] = {k: v * inv % self.p for k, v in rest.items()}
        return True


def echelon(polys: Iterable[Poly], p: int) -> Echelon:
    e = Echelon(p)
    for q in polys:
        e.add(q)
    return e


def rank(polys: Iterable[Poly], p: int) -> int:
    return len(echelon(polys, p).rows)


# --------------------------------------------------------------------------- check 1: the log
def resolve_log(sys_, log) -> Tuple[Dict[int, Dict[int, int]], List[Tuple[int, Dict[int, int]]]]:
    """-> (resolved definitions {signal: linear map over undefined signals}, extra equations)."""
    p = sys_.p
    first: Dict[int, Dict[int, int]] = {}
    extras = []
    for frm, to in log:
        if frm in sys_.forbidden:
            raise Unsound("log", f"the forbidden signal {frm} is defined")
        if not 0 < frm < sys_.max_signal:
            raise Unsound("log", f"the defined signal {frm} is no signal of the system")
        to = _nz(to, p)
        if any(not 0 <= k < sys_.max_signal for k in to):
            raise Unsound("log", f"the definition of {frm} names a signal outside the system")
        if frm in first:
            extras.append((frm, to))
        else:
            first[frm] = to
    done: Dict[int, Dict[int, int]] = {}
    for root in first:
        if root in done:
            continue
        stack = [root]
        open_ = {root}
        while stack:
            s = stack[-1]
            pend = [k for k in first[s] if k in first and k not in done]
            if pend:
                for k in pend:
                    if k in open_:
                        raise Unsound("log", f"the definitions of {s} and {k} form a cycle")
                k = pend[0]
                open_.add(k)
                stack.append(k)
                continue
            done[s] = _subst_lc(first[s], done, p)
            open_.discard(s)
            stack.pop()
    return done, extras


def _extra_polys(defs, extras, p) -> List[Poly]:
    out = []
    for frm, to in extras:
        m = {k: -v % p for k, v in to.items()}
        m[frm] = (m.get(frm, 0) + 1) % p
        out.append(_poly({}, {}, _subst_lc(m, defs, p), p))
    return out


# --------------------------------------------------------------------------- checks 2-6
def check_forward(sys_, cons, defs, extras):
    p = sys_.p
    ech = echelon((row_poly(c, {}, p) for c in cons), p)
    for i, row in enumerate(sys_.rows):
        rest = ech.reduce(row_poly(row, defs, p))
        if rest:
            raise Unsound("forward", f"input row {i} is not implied by the output: remainder {_show(rest)}")
    for (frm, _), q in zip(extras, _extra_polys(defs, extras, p)):
        rest = ech.reduce(q)
        if rest:
            raise Unsound("forward", f"a repeated definition of {frm} is not implied by the output: {_show(rest)}")


def check_reverse(sys_, cons, defs):
    p = sys_.p
    ech = echelon((row_poly(r, defs, p) for r in sys_.rows), p)
    for i, c in enumerate(cons):
        rest = ech.reduce(row_poly(c, {}, p))
        if rest:
            raise Unsound("reverse", f"output row {i} is not implied by the input: remainder {_show(rest)}")


def _signals(con, p) -> set:
    return {k for m in (con.a, con.b, con.c) for k, v in m.items() if k and v % p}


def check_no_leak(sys_, cons, defs):
    for i, c in enumerate(cons):
        leak = _signals(c, sys_.p) & defs.keys()
        if leak:
            raise Unsound("no leak", f"output row {i} still holds the defined signals {sorted(leak)}")


def check_witness_map(sys_, cons, sm, npiw):
    keys = {s for s in sys_.forbidden if s < sys_.max_signal}
    for c in cons:
        keys |= _signals(c, sys_.p)
    if set(sm) != keys:
        raise Unsound("witness map", f"signals with a wire: {sorted(set(sm) - keys)} too many, "
                                     f"{sorted(keys - set(sm))} missing")
    for w, s in enumerate(sorted(keys)):
        if sm[s] != w:
            raise Unsound("witness map", f"signal {s} has wire {sm[s]}, its rank is {w}")
    lo = sys_.n_pub_out + sys_.n_pub_in
    want = sum(1 for s in range(lo + 1, lo + sys_.n_priv_in + 1) if s in sm)
    if npiw != want:
        raise Unsound("witness map", f"no_private_inputs_witness is {npiw}, {want} private inputs have a wire")


def _dot(m, w, p):
    return sum(v * w[k] for k, v in m.items()) % p


def holds(con, w: Sequence[int], p: int) -> bool:
    return (_dot(con.a, w, p) * _dot(con.b, w, p) - _dot(con.c, w, p)) % p == 0


def check_witnesses(sys_, cons, log, witnesses):
    p = sys_.p
    for n, w in enumerate(witnesses):
        for i, c in enumerate(cons):
            if not holds(c, w, p):
                raise Unsound("witnesses", f"output row {i} fails on witness {n}")
        for i, (frm, to) in enumerate(log):
            if (w[frm] - _dot(to, w, p)) % p:
                raise Unsound("witnesses", f"log entry {i} (signal {frm}) fails on witness {n}")


def _show(poly: Poly, n=4) -> str:
    items = sorted(poly.items())
    return "{" + ", ".join(f"{k}: {v}" for k, v in items[:n]) + (", ..." if len(items) > n else "") + "}"


def failing_checks(sys_, result, witnesses=None, algebra=True) -> Dict[str, str]:
    """Runs every check on its own: {check name: message} of those that fail.  algebra=False leaves
    out forward and reverse (the echelon forms), for sizes where only the witnesses are affordable."""
    cons, sm, npiw, log = as_result(result)
    bad: Dict[str, str] = {}
    try:
        defs, extras = resolve_log(sys_, log)
    except Unsound as e:
        return {e.check: str(e)}
    steps = [lambda: check_no_leak(sys_, cons, defs), lambda: check_witness_map(sys_, cons, sm, npiw)]
    if algebra:
        steps += [lambda: check_forward(sys_, cons, defs, extras), lambda: check_reverse(sys_, cons, defs)]
    if witnesses is not None:
        steps.append(lambda: check_witnesses(sys_, cons, log, witnesses))
    for f in steps:
        try:
            f()
        except Unsound as e:
            bad[e.check] = str(e)
    return bad


def check(sys_, result, witnesses=None, algebra=True) -> None:
    """Raises Unsound for the first check (in the order of CHECKS) the result fails."""
    bad = failing_checks(sys_, result, witnesses, algebra)
    for name in CHECKS:
        if name in bad:
            raise Unsound(name, bad[name].split("] ", 1)[1])


def consistent_log(sys_, log) -> bool:
    """False if the log defines a signal twice with different right-hand sides."""
    seen: Dict[int, Dict[int, int]] = {}
    for s in log:
        frm, to = (s.frm, s.to) if hasattr(s, "frm") else s
        to = _nz(to, sys_.p)
        if seen.setdefault(frm, to) != to:
            return False
    return True


# --------------------------------------------------------------------------- thresholds
def p4_threshold() -> int:
    """The cluster size from which the engine takes process_4 (full_simplification,
    simplification_utils.rs:548-553), read from d_is_p4 in csrc/kernels.hpp."""
    import dispatch_shapes as ds
    m = re.search(r"\bbool\s+d_is_p4\s*\([^)]*\)\s*\{\s*return\s+n\s*>=\s*(\d+)", ds._text("kernels.hpp"))
    if not m:
        raise KeyError("d_is_p4 not found in kernels.hpp")
    return int(m.group(1))


# --------------------------------------------------------------------------- satisfiable systems
def gen_circuit(seed: int, p: int, n_int: int = 60, n_out: int = 2, n_pub: int = 2, n_priv: int = 4,
                redundant: float = 0.25, big_cluster: int = 0, k_wit: int = 4):
    """A seeded satisfiable --O0 system with k_wit witnesses, laid out as circom lays signals out:
    outputs, public inputs, private inputs, intermediates.  The inputs are free; every other signal is
    defined by exactly one row from signals defined before it, in a seeded order with the outputs
    last: a scaled equality, a constant (0 included), a linear combination of 1-5 terms, or a product
    of two linear combinations minus a third (some with a bare constant as A: linear after round 1's
    constant-A reduction, so they feed round 2).  Coefficients are rsio.gen_system's mix (1, p-1,
    small powers of two, uniform), so cancellations happen over 256-bit primes too.  A share
    `redundant` of further rows are seeded linear combinations of linear rows (rank-deficient
    clusters, rows that reduce to 0 = 0) and exact or scaled duplicates of linear and non-linear
    rows; then the rows are shuffled.  big_cluster: that many more intermediates, each defined by a
    linear row over one signal of a sliding window of the 24 before it plus public inputs (the
    windowed shape of gen_system's big_cluster), which grows one linear cluster past the process_4
    threshold.  The cluster's rows form a tree over its signals, and the other rows see only 16 of
    them: process_4 eliminates by occurrence count, not in definition order, and on a consistent
    system whose rows each hold several window signals that order fills the rows in (a 340-row
    cluster of that shape took the C++ oracle 18 s); on a tree every merge keeps a row short.

    Returns (System, witnesses): witness[s] is the value of signal s, witness[0] = 1.  Every witness
    satisfies every row (asserted here)."""
    rng = random.Random(seed)
    n_in = n_pub + n_priv
    inputs = list(range(n_out + 1, n_out + n_in + 1))
    first_int = n_out + n_in + 1
    big = list(range(first_int, first_int + big_cluster))
    inter = list(range(first_int + big_cluster, first_int + big_cluster + n_int))
    S = first_int + big_cluster + n_int
    rng.shuffle(inter)

    def coef():
        r = rng.random()
        if r < 0.35:
            return 1
        if r < 0.55:
            return p - 1
        if r < 0.7:
            return pow(2, rng.randrange(1, 8), p)
        return rng.randrange(1, p)

    def lc(pool, nmin, nmax, const_prob):
        m = {s: coef() for s in rng.sample(pool, min(len(pool), rng.randint(nmin, nmax)))}
        if rng.random() < const_prob:
            m[0] = coef()
        return m

    defs: List[Tuple[int, "R.Con"]] = []   # (signal, its row: C holds the signal, A and B do not)
    avail = list(inputs)
    pub = inputs[:n_pub] or inputs[:1]
    for i, s in enumerate(big):   # one signal of the window before it + public inputs: see the docstring
        m = {rng.choice(big[max(0, i - 24):i] or inputs): coef(), s: coef()}
        for t in rng.sample(pub, rng.randint(1, len(pub))):
            m.setdefault(t, coef())
        if rng.random() < 0.3:
            m[0] = coef()
        defs.append((s, R.Con({}, {}, m)))
    avail += big[-8:] + rng.sample(big[:-8], min(8, max(0, len(big) - 8)))
    for s in inter + list(range(1, n_out + 1)):
        r = rng.random()
        k = coef()
        if r < 0.15:
            row = R.Con({}, {}, {s: k, rng.choice(avail): (p - k) % p})
        elif r < 0.25:
            row = R.Con({}, {}, {s: k, 0: coef()} if rng.random() < 0.7 else {s: k})
        elif r < 0.60:
            m = lc(avail, 1, 5, 0.4)
            m[s] = k
            row = R.Con({}, {}, m)
        else:
            a = {0: coef()} if rng.random() < 0.15 else lc(avail, 1, 2, 0.15)
            b = lc(avail, 1, 3, 0.2)
            c = lc(avail, 0, 2, 0.2)
            c[s] = k
            row = R.Con(a, b, c)
        defs.append((s, row))
        avail.append(s)

    rows = [row for _, row in defs]
    linear = [row for row in rows if not row.a and not row.b]
    for _ in range(int(redundant * len(rows))):
        r = rng.random()
        if r < 0.4:
            m: Dict[int, int] = {}
            for row in rng.sample(linear, min(len(linear), rng.randint(2, 3))):
                k = coef()
                for s, v in row.c.items():
                    m[s] = (m.get(s, 0) + k * v) % p
            m = {s: v for s, v in m.items() if v}
            if m:
                rows.append(R.Con({}, {}, m))
        else:
            row = rng.choice(rows)
            k = 1 if rng.random() < 0.5 else coef()
            rows.append(R.Con({s: v * k % p for s, v in row.a.items()}, dict(row.b),
                              {s: v * k % p for s, v in row.c.items()}))
    rng.shuffle(rows)

    witnesses = []
    for _ in range(max(4, k_wit)):
        w = [0] * S
        w[0] = 1
        for s in inputs:
            w[s] = rng.randrange(p)
        for s, row in defs:
            k = row.c[s]
            rest = sum(v * w[t] for t, v in row.c.items() if t != s)
            w[s] = (_dot(row.a, w, p) * _dot(row.b, w, p) - rest) * pow(k, -1, p) % p
        assert all(holds(row, w, p) for row in rows)
        witnesses.append(w)
    forb = {0} | set(range(1, n_out + n_pub + 1))
    return R.System(p, S, n_out, n_pub, n_priv, forb, rows), witnesses


# --------------------------------------------------------------------------- the suites' cases
PRIMES = {**R.PRIMES, "f257": 257, "f97": 97}           # the eight --prime choices, F_257 and F_97
FLAG_SETS = {"O1": ("O1", None, False), "O2": ("O2", None, False), "O2round1": ("O2", 1, False),
             "O2round2": ("O2", 2, False), "old": ("O2", None, True)}   # (level, rounds, old heuristics)
ROUND2 = ("bn128", 0)   # a small case whose round 2 substitutes (certified in test_soundness.py)


def small_circuit(prime: str, seed: int):
    """The small case `seed` (0..29) of a prime: 40-98 intermediates."""
    return gen_circuit(1000 * sorted(PRIMES).index(prime) + seed, PRIMES[prime], n_int=40 + 2 * seed)


def large_circuit(prime: str, i: int):
    """The large-cluster case i (0, 1) of a prime: one linear cluster past the process_4 threshold."""
    return gen_circuit(900 + i, PRIMES[prime], n_int=60, big_cluster=p4_threshold() + 40 + 25 * i)
