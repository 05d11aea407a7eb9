"""Inputs of known shape for the kernel dispatch boundaries, and the CPU proof of that shape.

The library routes every linear cluster, substitution and non-linear row by comparing a size with
a constant of csrc/.  This module has three parts, none of which needs a GPU:

  constants     a parser that reads those constants from the sources (a retuned constant moves the
                tests with it, a renamed one raises);
  gadgets       seeded builders of pyref.System whose shapes are fixed with forbidden signals (any
                id placed in System.forbidden): forbidden signals glue rows into one cluster in
                build_clusters and are never taken, so a row with one takeable signal and a
                constant plus L - 1 forbidden ones yields a substitution of exactly L terms;
  certificates  pure-Python functions over oracle/pyref.py that return, for a System, the numbers
                the device branches on.

CASES lists every boundary case once; tests/test_dispatch_shapes.py proves each case's shape on the
CPU and tests/test_gpu_dispatch.py runs the same cases against the oracle on the GPU.
"""
from __future__ import annotations

import copy
import os
import random
import re
from collections import defaultdict
from typing import Callable, Dict, List, Optional

import rsio

R = rsio.R
CSRC = os.path.join(rsio.ROOT, "circom_cvm_amd", "csrc")

# the reference's own rule (simplification_utils.rs:548-553, d_is_p4): process_4 for clusters of
# 350 <= rows < 1,000,000 unless --use_old_heuristics.  Not a constant of this library.
P4_MIN, P4_END = 350, 1000000


# ============================================================================ constants
_TEXT: Dict[str, str] = {}


def _text(name: str) -> str:
    if name not in _TEXT:
        with open(os.path.join(CSRC, name)) as f:
            # comments never define anything
            t = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
            _TEXT[name] = re.sub(r"//[^\n]*", "", t)
    return _TEXT[name]


def _files() -> List[str]:
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hpp") or f == "engine.hip")


_DEFS: Optional[Dict[str, str]] = None
_AMBIGUOUS = "<defined more than once>"


def _definitions() -> Dict[str, str]:
    """name -> defining expression, for `constexpr <type> a = x, b = y;` and `#define NAME x`."""
    global _DEFS
    if _DEFS is None:
        d: Dict[str, str] = {}
        for fn in _files():
            t = _text(fn)
            for m in re.finditer(r"\bconstexpr\s+(?:static\s+)?(?:const\s+)?[\w:]+\s+(k\w+\s*=[^;(){}]*);", t):
                for part in m.group(1).split(","):
                    nm, _, ex = part.partition("=")
                    nm, ex = nm.strip(), ex.strip()
                    if not re.fullmatch(r"\w+", nm) or not ex:
                        raise ValueError(f"{fn}: cannot read the definition {part!r}")
                    if nm in d and d[nm] != ex:
                        ex = _AMBIGUOUS   # (a local alias such as `kClChunk = CHUNK`): asking for it raises
                    d[nm] = ex
            for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S+)[ \t]*$", t, flags=re.M):
                d.setdefault(m.group(1), m.group(2))
        _DEFS = d
    return _DEFS


def _resolve(expr: str, depth: int = 0) -> int:
    expr = expr.strip()
    m = re.fullmatch(r"(0[xX][0-9a-fA-F]+|\d+)[uUlL]*", expr)
    if m:
        return int(m.group(1), 0)
    if re.fullmatch(r"\w+", expr) and depth < 8 and expr in _definitions():
        return _resolve(_definitions()[expr], depth + 1)
    raise KeyError(f"cannot resolve {expr!r} to an integer")


def constant(name: str) -> int:
    """The integer value of a named constant of csrc/; raises when it is gone or not an integer."""
    d = _definitions()
    if name not in d:
        raise KeyError(f"no constant named {name} in {CSRC}")
    return _resolve(d[name])


def template_arg(filename: str, callee: str) -> int:
    """The integer template argument `callee<N>` is launched / called with in `filename` (one value)."""
    vals = set()
    for m in re.finditer(r"\b" + re.escape(callee) + r"\s*<\s*(\w+)\s*>", _text(filename)):
        vals.add(_resolve(m.group(1)))
    if len(vals) != 1:
        raise KeyError(f"{callee}<N> in {filename}: expected one value, found {sorted(vals)}")
    return vals.pop()


class K:
    """Every threshold the cases use, read from the sources on first use."""
    _names = ("kWaveMin", "kClSmall", "kHeavyNnz", "kSpecK", "kComposeCap", "kFinWaveBelow", "kFwT", "kFwE",
              "kTailSplit", "kClMid", "kWideMin", "kSpecTabMax", "kGiantRows", "kClLds", "kHeadLimit",
              "kGhRowMax", "kGhRhsMax", "kMergeK", "kMergeO", "kMergeD", "kFwRunsRank")

    def __getattr__(self, nm):
        if nm in K._names:
            v = constant(nm)
        elif nm == "tail_cap":      # the tail's ordered loop: k_big_main<CAP> in engine.hip
            v = template_arg("engine.hip", "k_big_main")
        elif nm == "spec_cap":      # the speculative head's one-wave fallback in spec_loop.hpp
            v = template_arg("spec_loop.hpp", "d_big_main_cluster")
        else:
            raise AttributeError(nm)
        setattr(self, nm, v)
        return v


k = K()


# ============================================================================ gadgets
class Builder:
    """Accumulates rows over fresh signal ids.  Signals 1..3 are the public ones (forbidden), 4..8 the
    private inputs (unused); everything a gadget needs is allocated from 9 on."""

    def __init__(self, seed: int, p: int):
        self.rng = random.Random(seed)
        self.p = p
        self.forb = {0, 1, 2, 3}
        self.nxt = 9
        self.rows: List["R.Con"] = []
        self.n_lin = 0
        self.n_nl = 0

    def take(self, n: int) -> List[int]:
        s = list(range(self.nxt, self.nxt + n))
        self.nxt += n
        return s

    def forbid(self, n: int) -> List[int]:
        s = self.take(n)
        self.forb.update(s)
        return s

    def coef(self) -> int:
        r, p = self.rng.random(), self.p
        if r < 0.35:
            return 1
        if r < 0.55:
            return p - 1
        if r < 0.7:
            return pow(2, self.rng.randrange(1, 8), p)
        return self.rng.randrange(1, p)

    def lin(self, keys, const=False) -> int:
        """A linear row over `keys` (+ a constant term); never an equality or a constant equality."""
        keys = list(keys)
        assert len(set(keys)) == len(keys) and 0 not in keys
        assert len(keys) >= 3 or (len(keys) == 2 and const), "would classify as an (constant) equality"
        m = {}
        if const:
            m[0] = self.coef()
        for s in keys:
            m[s] = self.coef()
        self.rows.append(R.Con({}, {}, m))
        self.n_lin += 1
        return self.n_lin - 1

    def nonlin(self, a, b, c) -> int:
        self.rows.append(R.Con(dict(a), dict(b), dict(c)))
        self.n_nl += 1
        return self.n_nl - 1

    def probes(self, sigs, n=None):
        """Quadratic rows over cluster signals, so the cluster's substitutions reach the output: n
        random ones, or by default one row per six signals that together hold every signal once.
        Their A and B keep a signal after any substitution of these gadgets, so no row turns linear."""
        sigs = list(sigs)
        if n is not None:
            for _ in range(n):
                a, b, c = (self.rng.choice(sigs) for _ in range(3))
                self.nonlin({a: self.coef()}, {b: self.coef()}, {c: self.coef(), 0: self.coef()})
            return
        for i in range(0, len(sigs), 6):
            ch = sigs[i:i + 6]
            while len(ch) < 3:
                ch.append(self.rng.choice(sigs))
            c = {s: self.coef() for s in ch[2:]}
            c[0] = self.coef()
            self.nonlin({ch[0]: self.coef()}, {ch[1]: self.coef()}, c)

    def system(self) -> "R.System":
        return R.System(self.p, self.nxt, 1, 2, 5, set(self.forb), self.rows)


def chain(b: Builder, n: int, n_w: Optional[int] = None, unique=False, no_unique_rows=(), glue=None,
          extra_shared: int = 0, const_rows: int = 0) -> dict:
    """An n-row cluster x_i + c x_{i+1} + d w_{i mod n_w} = 0 (the style of test_gpu_edge.long_chain):
    ordered -- every row but the two ends has no signal of its own -- and with shared process_3
    pivots (the w ids lie above the x ids), so neither the uniques phase nor k_p3_fast takes it.
    unique: every row but `no_unique_rows` also gets a signal of its own, which makes a process_4
    cluster order-free (d_cl_order_free).  glue: a forbidden id added to the middle row.
    extra_shared: that many more takeable signals, each in two rows.  const_rows: that many rows get
    a constant term (one more entry each)."""
    assert n >= 4
    if n_w is None:
        n_w = max(1, min(50, n // 4))
    x = b.take(n + 1)
    u = b.take(n) if unique else None
    y = b.take(extra_shared)
    w = b.take(n_w)
    assert 2 * extra_shared <= n
    first = b.n_lin
    for i in range(n):
        keys = [x[i], x[i + 1], w[i % n_w]]
        if unique and i not in no_unique_rows:
            keys.append(u[i])
        if i // 2 < extra_shared:
            keys.append(y[i // 2])
        if glue is not None and i == n // 2:
            keys.append(glue)
        b.lin(keys, const=i < const_rows)
    return dict(x=x, w=w, first=first, n=n, probe=x + w)


def fillers(b: Builder, sizes) -> List[dict]:
    """Disjoint chains of the given sizes: workgroup-class clusters that occupy the first places of
    the size order, pushing a smaller cluster under test past kHeadLimit into the tail."""
    return [chain(b, n) for n in sizes]


def blob(b: Builder, n_rows: int, nnz: int) -> dict:
    """A cluster of n_rows (< kWaveMin) rows holding exactly nnz entries."""
    assert nnz >= 3 * n_rows
    g = b.forbid(1)[0]
    y = b.take(n_rows + 1)
    extra, per = nnz - 3 * n_rows, (nnz - 3 * n_rows) // n_rows
    first = b.n_lin
    for r in range(n_rows):
        e = per + (1 if r < extra - per * n_rows else 0)
        b.lin([g, y[r], y[r + 1]] + b.take(e))
    return dict(first=first, n=n_rows, probe=y)


def wide_row(b: Builder, cl: dict, length: int, fresh_ok=False, contiguous=False) -> int:
    """One row of exactly `length` entries, all takeable keys of the cluster `cl` (a chain's x); with
    fresh_ok the keys the cluster cannot supply are new takeable signals with smaller ids (process_3
    clusters only: process_4 would consume such a row in its uniques phase).  contiguous: a run of
    neighbouring chain signals instead of a random sample (its merges shorten the row: cheaper on
    the one-wave loops)."""
    have = cl["x"]
    if contiguous and length <= len(have):
        at = b.rng.randrange(len(have) - length + 1)
        keys = have[at:at + length]
    else:
        keys = b.rng.sample(have, min(length, len(have)))
    if len(keys) < length:
        assert fresh_ok
        lo = cl.get("low")
        assert lo is not None and len(lo) >= length - len(keys)
        keys += lo[: length - len(keys)]
    return b.lin(keys)


def merge_pair(b: Builder, glue: int, len_a: int, len_b: int):
    """Two rows of len_a and len_b entries that share their only takeable signal z: whichever is
    popped first becomes z's holder with a right-hand side as long as the row (the constant slot
    replaces z), and the other conflicts with it at its full length.  Both hold the forbidden
    `glue`, which puts them into the cluster that holds it."""
    z = b.take(1)[0]
    b.lin([z, glue] + b.forbid(len_a - 2))
    b.lin([z, glue] + b.forbid(len_b - 2))


def cancel_pair(b: Builder, glue: int, length: int, kind: str) -> dict:
    """Two rows of length + 1 entries -- the forbidden `glue`, length - 2 fresh forbidden signals, a
    constant and their only takeable signal z, which they share -- the second the first times a
    non-unit coefficient.  Whichever is popped first becomes z's holder with `length` right-hand-side
    terms; the other conflicts with it and every term of the merge cancels:
      "empty"    the merged row is 0 = 0 and is dropped;
      "const"    the second row's constant is changed: the merge leaves 0 = c, c != 0, a leftover row;
      "partial"  one fresh forbidden coefficient of the second row is changed: the other length - 1
                 terms cancel and that key survives alone, a leftover row without a takeable signal."""
    assert length >= 4 and kind in ("empty", "const", "partial")
    p = b.p
    z = b.take(1)[0]
    f = b.forbid(length - 2)
    first = {0: b.coef(), z: b.coef(), glue: b.coef()}
    first.update({s: b.coef() for s in f})
    kk = b.rng.randrange(2, p - 1)
    second = {s: v * kk % p for s, v in first.items()}
    if kind != "empty":
        at = 0 if kind == "const" else f[len(f) // 2]
        second[at] = (second[at] + 1) % p or 1
        assert second[at] != first[at] * kk % p
    for m in (first, second):
        assert all(m.values())
        b.rows.append(R.Con({}, {}, m))
        b.n_lin += 1
    return dict(z=z, work_plus_rhs=2 * length + 1, survivor=None if kind != "partial" else f[len(f) // 2])


def star(b: Builder, length: int) -> int:
    """x + c_0 + sum_{k < length-1} c_k f_k = 0 with every f forbidden: the substitution of x has
    exactly `length` right-hand-side terms.  Returns x."""
    assert length >= 2
    x = b.take(1)[0]
    b.lin([x] + b.forbid(length - 1), const=True)
    return x


def twin_stars(b: Builder, length: int):
    """Two stars over the same length - 1 forbidden signals and constant whose right-hand sides are
    proportional: x1 = r1 * E and x2 = r2 * E for one expression E of `length` terms.  Returns
    (x1, x2, ratio): a * x1 + (a * ratio) * x2 substitutes to `length` explicit zeros, for any a."""
    assert length >= 3
    p = b.p
    x1, x2 = b.take(2)
    f = b.forbid(length - 1)
    e = {0: b.coef()}
    e.update({s: b.coef() for s in f})
    v1, v2, kk = b.coef(), b.coef(), b.rng.randrange(2, p - 1)
    b.rows.append(R.Con({}, {}, {**e, x1: v1}))
    b.rows.append(R.Con({}, {}, {**{s: v * kk % p for s, v in e.items()}, x2: v2}))
    b.n_lin += 2
    # x1 = -E / v1, x2 = -kk E / v2: a / v1 + a ratio kk / v2 = 0
    return x1, x2, (p - 1) * v2 % p * pow(v1 * kk % p, -1, p) % p


def quad(b: Builder, spec_a, spec_b, spec_c) -> int:
    """One non-linear row.  Each spec lists the entries of A, B, C: "p" a plain signal nothing
    substitutes, "c" the constant, an int L a signal substituted by a star of L terms, ("twin", L)
    both signals of twin_stars(L) with coefficients under which their 2 L terms cancel."""
    def lc(spec):
        m = {}
        for e in spec:
            if e == "c":
                m[0] = b.coef()
            elif e == "p":
                m[b.forbid(1)[0]] = b.coef()
            elif isinstance(e, tuple):
                assert e[0] == "twin"
                x1, x2, ratio = twin_stars(b, e[1])
                m[x1] = b.coef()
                m[x2] = m[x1] * ratio % b.p
            else:
                m[star(b, int(e))] = b.coef()
        return m
    return b.nonlin(lc(spec_a), lc(spec_b), lc(spec_c))


def late_star(b: Builder, length: int) -> int:
    """A non-linear row whose A is one constant term s: round 1's fix_constraint turns it into the
    linear row C - s * B, which holds one takeable signal x, the constant and length - 1 forbidden
    signals -- so round 2 (and no round before it) substitutes x by exactly `length` terms.  Returns x."""
    assert length >= 3
    x = b.take(1)[0]
    f = b.forbid(length - 1)
    c = {s: b.coef() for s in f[1:]}
    c[0] = b.coef()
    b.nonlin({0: b.coef()}, {x: b.coef(), f[0]: b.coef()}, c)
    return x


def late_twins(b: Builder, length: int):
    """twin_stars for round 2: two late_star rows whose linear forms are proportional but for their
    own signals x1, x2.  Returns (x1, x2, ratio) as twin_stars does."""
    assert length >= 3
    p = b.p
    x1, x2 = b.take(2)
    f = b.forbid(length - 1)
    c = {s: b.coef() for s in f[1:]}
    c[0] = b.coef()
    s1, s2, bx1, bx2, bf, kk = b.coef(), b.coef(), b.coef(), b.coef(), b.coef(), b.rng.randrange(2, p - 1)
    # C - s B: E - s1 bx1 x1 and kk E - s2 bx2 x2 with E = C - s1 bf f0
    b.nonlin({0: s1}, {x1: bx1, f[0]: bf}, dict(c))
    b.nonlin({0: s2}, {x2: bx2, f[0]: kk * s1 % p * bf % p * pow(s2, -1, p) % p}, {q: v * kk % p for q, v in c.items()})
    return x1, x2, (p - 1) * s2 % p * bx2 % p * pow(s1 * bx1 % p * kk % p, -1, p) % p


def storage_row(b: Builder, n_plain: int, late_lengths, twin_a=None, twin_c=None) -> int:
    """A non-linear row round 1 leaves as it is (A and B one plain signal each): C holds n_plain plain
    signals and one signal per entry of late_lengths that round 2 substitutes by that many terms.
    twin_a / twin_c = L: A is (C also holds) the two signals of late_twins(L) with coefficients under
    which round 2's substitutions cancel -- round 1 still leaves the row alone."""
    c = {b.forbid(1)[0]: b.coef() for _ in range(n_plain)}
    for ln in late_lengths:
        c[late_star(b, ln)] = b.coef()
    a = {b.forbid(1)[0]: b.coef()} if twin_a is None else {}
    for m, ln in ((a, twin_a), (c, twin_c)):
        if ln is not None:
            x1, x2, ratio = late_twins(b, ln)
            m[x1] = b.coef()
            m[x2] = m[x1] * ratio % b.p
    return b.nonlin(a, {b.forbid(1)[0]: b.coef()}, c)


def dep_sub(b: Builder, n_own: int, n_dep: int, dep_len: int, pad: int, cancel: int = 0, inherit: bool = False) -> dict:
    """A process_3 cluster whose normalised substitution for one signal s has n_own entries that no
    substitution holds (the constant slot and n_own - 1 forbidden signals) and n_dep entries that are
    themselves holders, each with dep_len right-hand-side terms.  `pad` more rows (sharing a
    forbidden signal of s's row) bring the cluster into the workgroup class.
    cancel = m: the first 2 m dependencies pair up, each pair over one shared forbidden signal q (in
    place of a fresh one: dep_len stays), and s's coefficient of the pair's second holder is solved so
    that q cancels in the composed right-hand side of s: m explicit zero keys, which the reference
    keeps.  inherit: one more holder t above s whose row contains s, so its composed right-hand
    side carries the zero keys of s.  The defaults consume nothing and give the plain rows."""
    assert n_own >= 2 and dep_len >= 2
    assert 2 * cancel <= n_dep and (cancel == 0 or dep_len >= 3)
    p = b.p
    h = b.take(n_dep)
    s = b.take(1)[0]           # above every h: take_signal_3 picks it in its own row
    t = b.take(1)[0] if inherit else None   # above s
    g = b.forbid(n_own - 1)
    q = b.forbid(cancel)
    first = b.n_lin
    for j in range(n_dep):
        if j < 2 * cancel:
            b.lin([h[j], q[j // 2]] + b.forbid(dep_len - 2))
            continue
        f = b.forbid(dep_len - 1)
        if dep_len == 2:        # two signals: keep it from being an equality
            b.rows.append(R.Con({}, {}, {h[j]: 1, f[0]: 2 + j}))
            b.n_lin += 1
        else:
            b.lin([h[j]] + f)
    keys = [s] + h + g
    if len(keys) < 3:
        keys += b.forbid(3 - len(keys))
    b.lin(keys)
    row_s = b.rows[-1].c
    for i in range(cancel):
        # h = -(b q + ..) / c per holder row: a1 b1 / c1 + a2 b2 / c2 = 0 cancels q in s
        r1, r2 = b.rows[-1 - n_dep + 2 * i].c, b.rows[-n_dep + 2 * i].c
        h1, h2 = h[2 * i], h[2 * i + 1]
        row_s[h2] = (p - 1) * row_s[h1] % p * r1[q[i]] % p * r2[h2] % p * pow(r1[h1] * r2[q[i]] % p, -1, p) % p
        assert row_s[h2] != 0
    ys = b.take(pad)
    for yv in ys:
        b.lin([yv, g[0]] + b.forbid(1))
    if inherit:
        b.lin([t, s] + b.forbid(1))
    return dict(s=s, t=t, zeros=q, first=first, n=n_dep + 1 + pad + int(inherit), probe=[s] + h[:4] + ys[:4] + ([t] if inherit else []))


def zero_sub(b: Builder, dep_len: int, pad: int) -> dict:
    """A process_3 cluster in which every non-constant key of one substitution cancels: two holders
    h1, h2 over the same dep_len - 1 forbidden signals with proportional rows, and s + a1 h1 + a2 h2
    = 0 with a1, a2 solved as in dep_sub(cancel=..): the composed right-hand side of s is the
    constant slot and dep_len - 1 explicit zeros.  t's row holds s and inherits them; `pad` more
    rows share a forbidden signal of the holders' rows."""
    assert dep_len >= 3
    p = b.p
    h1, h2, s, t = b.take(4)
    f = b.forbid(dep_len - 1)
    first = b.n_lin
    e = {q: b.coef() for q in f}
    c1, c2, kk, a1 = b.coef(), b.coef(), b.rng.randrange(2, p - 1), b.coef()
    a2 = (p - 1) * a1 % p * c2 % p * pow(c1 * kk % p, -1, p) % p
    for m in ({**e, h1: c1}, {**{q: v * kk % p for q, v in e.items()}, h2: c2}, {s: b.coef(), h1: a1, h2: a2}):
        assert all(m.values())
        b.rows.append(R.Con({}, {}, m))
        b.n_lin += 1
    ys = b.take(pad)
    for yv in ys:
        b.lin([yv, f[0]] + b.forbid(1))
    b.lin([t, s] + b.forbid(1))
    return dict(s=s, t=t, zeros=f, first=first, n=4 + pad, probe=[s, t, h1, h2] + ys[:4])


# ============================================================================ certificates
def linear_after_frames(sys_: "R.System"):
    """The linear list as the clustering sees it: after the eq and constant-eq phases
    (constraint_simplification.rs:442-530, restated in pyref.simplification)."""
    p, forb = sys_.p, set(sys_.forbidden)
    cons_eq, eqs, linear, non_linear = R.classify(sys_)
    subs, _ = R.eq_simplification(eqs, forb, sys_.max_signal, p, None)
    single = R.build_encoded_fast_substitutions(subs)
    for c in linear + cons_eq:
        if R.fast_encoded_constraint_substitution(c, single, p):
            R.fix_constraint(c, p)
    subs, _ = R.constant_eq_simplification(cons_eq, forb, p, None)
    const_subs = R.build_encoded_fast_substitutions(subs)
    for c in linear:
        if R.fast_encoded_constraint_substitution(c, const_subs, p):
            R.fix_constraint(c, p)
    return linear, non_linear, single, const_subs


def cluster_shapes(sys_: "R.System", old=False) -> List[dict]:
    """Per cluster, in arena order (ascending largest row index, cluster.hpp): rows, entries (with
    the constant terms, as rows.len counts them), distinct takeable signals, rows without a signal of
    their own, whether process_4 takes it, the workgroup class and the rank in k_cl_sizekey's order
    (workgroup class first, size descending, index).  A plain union-find over the keys: the same
    components build_clusters makes (cross-checked against it up to kClMid rows)."""
    linear = [c for c in linear_after_frames(sys_)[0] if not R.is_empty(c)]
    forb = sys_.forbidden
    parent = list(range(len(linear)))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    last: Dict[int, int] = {}
    occ: Dict[int, int] = defaultdict(int)
    for j, c in enumerate(linear):
        for s in c.c:
            if s == 0:
                continue
            occ[s] += 1
            if s in last:
                ra, rb = find(last[s]), find(j)
                if ra != rb:
                    parent[min(ra, rb)] = max(ra, rb)
            last[s] = j
    comp: Dict[int, List[int]] = defaultdict(list)
    for j in range(len(linear)):
        comp[find(j)].append(j)
    out = []
    for root in sorted(comp):          # the root is the component's largest row index
        rows = comp[root]
        assert root == rows[-1]
        sig = set()
        entries = no_unique = 0
        for j in rows:
            c = linear[j].c
            entries += len(c)
            tk = [s for s in c if s not in forb]
            sig.update(tk)
            no_unique += not any(occ[s] == 1 for s in tk)
        n = len(rows)
        p4 = P4_MIN <= n < P4_END and not old
        out.append(dict(rows=n, entries=entries, takeable=len(sig), no_unique=no_unique, p4=p4,
                        order_free=p4 and no_unique == 0,
                        wg=n >= k.kWaveMin or entries >= k.kHeavyNnz, row_ids=rows,
                        max_row_len=max(len(linear[j].c) for j in rows)))
    order = sorted(range(len(out)), key=lambda c: (not out[c]["wg"], -out[c]["rows"], c))
    for rank, c in enumerate(order):
        out[c]["rank"] = rank
        out[c]["index"] = c
    if len(linear) <= k.kClMid:
        ref = R.build_clusters(linear, sys_.max_signal)
        assert [len(cl) for cl in ref] == [c["rows"] for c in out], "union-find differs from build_clusters"
    return out


def cluster_rows(sys_: "R.System", shape: dict) -> List["R.Con"]:
    """The cluster's rows in the list order build_clusters gives them (the order process_3/4 pop from)."""
    linear = [c for c in linear_after_frames(sys_)[0] if not R.is_empty(c)]
    if len(linear) <= k.kClMid:
        for cl in R.build_clusters(linear, sys_.max_signal):
            if {id(c) for c in cl} == {id(linear[j]) for j in shape["row_ids"]}:
                return cl
        raise AssertionError("cluster not found")
    # large lists: the cluster alone replays to the same order (clusters are independent)
    cl = R.build_clusters([linear[j] for j in shape["row_ids"]], sys_.max_signal)
    assert len(cl) == 1
    return cl[0]


def merge_kind(work: "R.Con", forbidden) -> str:
    """What a conflict merge left: "empty" (0 = 0, dropped), "const" (only key 0, non-zero: 0 = c, a
    leftover row), "forbidden" (no takeable signal left: a leftover row) or "live" (the loop goes on)."""
    if R.is_empty(work):
        return "empty"
    if set(work.c) == {0}:
        return "const"
    return "forbidden" if R.take_signal_3(forbidden, work) is None else "live"


def elimination_trace(cluster: List["R.Con"], forbidden, p: int, p4: bool):
    """substitution_process_3 / _4 step by step with pyref's own pieces, recording what the ordered
    loops branch on: the length of every row as it is popped and, per conflict, (work length,
    holder right-hand-side length) in `merges` and (work length, right-hand-side length, length of
    the merged row, merge_kind of it) in `results`.  The holder it ends with is checked against pyref's."""
    pops, merges, results = [], [], []
    holder: dict = {}
    if not p4:
        cons = list(cluster)
        while cons:
            work = cons.pop()
            pops.append(len(work.c))
            while not R.is_empty(work):
                out = R.take_signal_3(forbidden, work)
                if out is None:
                    break
                coef, to = R.clear_signal_not_normalized(work.c, out, p)
                if out not in holder:
                    holder[out] = (coef, to)
                    break
                merges.append((len(work.c), len(holder[out][1])))
                work = R.merge_conflict(coef, to, holder[out][0], holder[out][1], p)
                results.append(merges[-1] + (len(work.c), merge_kind(work, forbidden)))
        ref: dict = {}
        R.substitution_process_3(forbidden, cluster, ref, p)
    else:
        vec = [c.clone() for c in cluster]
        occ: Dict[int, int] = {}
        rep: Dict[int, int] = {}
        for pos, c in enumerate(vec):
            for s in c.c:
                if s not in forbidden:
                    if s in occ:
                        occ[s] += 1
                    else:
                        occ[s], rep[s] = 1, pos
        deleted = set()
        for s, idx in sorted((s, rep[s]) for s, n in occ.items() if n == 1):
            if not R.is_empty(vec[idx]):
                act, vec[idx] = vec[idx], R.con_empty()
                for q in act.c:
                    if q not in forbidden and q in occ:
                        occ[q] -= 1
                holder[s] = R.clear_signal_not_normalized(act.c, s, p)
                occ.pop(s, None)
                deleted.add(s)
        while vec:
            work = vec.pop()
            for q in work.c:
                if q not in forbidden and q in occ:
                    occ[q] -= 1
            if R.is_empty(work):
                continue
            pops.append(len(work.c))
            while not R.is_empty(work):
                out = R.take_signal_4(forbidden, deleted, occ, work)
                if out is None:
                    break
                coef, to = R.clear_signal_not_normalized(work.c, out, p)
                if out not in holder:
                    deleted.add(out)
                    occ.pop(out, None)
                    holder[out] = (coef, to)
                    break
                merges.append((len(work.c), len(holder[out][1])))
                work = R.merge_conflict(coef, to, holder[out][0], holder[out][1], p)
                results.append(merges[-1] + (len(work.c), merge_kind(work, forbidden)))
        ref = {}
        R.substitution_process_4(forbidden, cluster, ref, p)
    assert holder == ref, "the trace diverged from pyref"
    return dict(pops=pops, merges=merges, results=results, holder=holder)


def compose_shape(sys_: "R.System", shape: dict, s: int, p4: bool = False) -> dict:
    """For the process_3 substitution of s, before composition: its length, how many of its entries
    are holders, and E = own entries + the (composed) lengths of those holders' right-hand sides --
    what d_compose_wave / d_compose_merge compare (kernels.hpp).  p4: the same for a process_4
    cluster, composed in its deletion order (create_nonoverlapping_substitutions_4); every holder
    among s's entries must then be final before s."""
    cl = cluster_rows(sys_, shape)
    holder: dict = {}
    if p4:
        _, order = R.substitution_process_4(sys_.forbidden, cl, holder, sys_.p)
        norm = R.normalize_substitutions(holder, sys_.p)
        pre = dict(norm[s].to)
        final = R.create_nonoverlapping_substitutions_4(copy.deepcopy(norm), order, sys_.p)
        deps = [q for q in pre if q in holder]
        assert all(order.index(q) < order.index(s) for q in deps)
        n_own = len(pre) - len(deps)
        tot = sum(len(final[q].to) for q in deps)
        return dict(length=len(pre), holders=len(deps), own=n_own, dep_total=tot, E=n_own + tot)
    R.substitution_process_3(sys_.forbidden, cl, holder, sys_.p)
    norm = R.normalize_substitutions(holder, sys_.p)
    pre = dict(norm[s].to)
    final = R.create_nonoverlapping_substitutions(copy.deepcopy(norm), sys_.p)
    deps = [q for q in pre if q in holder]
    assert all(q < s for q in deps)
    n_own = len(pre) - len(deps)
    tot = sum(len(final[q].to) for q in deps)
    return dict(length=len(pre), holders=len(deps), own=n_own, dep_total=tot, E=n_own + tot)


def nonlinear_shapes(sys_: "R.System", old=False) -> List[dict]:
    """Per non-linear row of round 1, what k_frames_wave<0> branches on: entries (of A, B and C, after
    frames 1-2), terms (an entry a linear substitution replaces counts its right-hand side, the
    d_frame_weight sum), runs (the most entries in one of A, B, C: in round 1 every entry is a run)
    and, when A or B ends as one constant term, the fix pass's terms len(C) + len(other)."""
    p = sys_.p
    res = R.simplification(sys_, rsio.R.Flags(no_rounds=1, use_old_heuristics=old), want_log=True)
    _, non_linear, single, const_subs = linear_after_frames(sys_)
    lin = {sb.frm: sb for sb in res.log if sb.frm not in single and sb.frm not in const_subs}
    out = []
    for c0 in non_linear:
        c = c0.clone()
        for fr in (single, const_subs):
            R.fast_encoded_constraint_substitution(c, fr, p)
        parts = (c.a, c.b, c.c)
        entries = sum(len(m) for m in parts)
        terms = sum(len(lin[s].to) if s in lin else 1 for m in parts for s in m)
        runs = max(len(m) for m in parts)
        d = c.clone()
        R.fast_encoded_constraint_substitution(d, R.build_encoded_fast_substitutions(list(lin.values())), p)
        R.remove_zero_con(d)
        fix = None
        if d.a and d.b:
            if R.is_constant_expression(d.a):
                fix = len(d.c) + len(d.b)
            elif R.is_constant_expression(d.b):
                fix = len(d.c) + len(d.a)
        out.append(dict(entries=entries, terms=terms, runs=runs, fix=fix))
    return out


def round2_shapes(sys_: "R.System", old=False) -> dict:
    """What k_frames_wave<1> branches on in round 2: per storage row left by round 1 (the non-linear
    rows that stayed non-linear, as round 1 wrote them), its entries and its terms under round 2's
    substitutions (k_round_count: an entry round 2 substitutes counts its right-hand side), and
    whether round 2 touches it; plus the number of round-2 substitutions (pyref's log at
    no_rounds = 2 beyond its log at no_rounds = 1)."""
    p = sys_.p
    log1 = R.simplification(sys_, R.Flags(no_rounds=1, use_old_heuristics=old), want_log=True).log
    log2 = R.simplification(sys_, R.Flags(no_rounds=2, use_old_heuristics=old), want_log=True).log
    assert [(s.frm, s.to) for s in log2[:len(log1)]] == [(s.frm, s.to) for s in log1]
    sub2 = {s.frm: s for s in log2[len(log1):]}
    _, non_linear, single, const_subs = linear_after_frames(sys_)
    lin1 = R.build_encoded_fast_substitutions([s for s in log1 if s.frm not in single and s.frm not in const_subs])
    rows = []
    for c0 in non_linear:
        c = c0.clone()
        for fr in (single, const_subs, lin1):
            R.fast_encoded_constraint_substitution(c, fr, p)
        R.fix_constraint(c, p)
        if R.is_linear(c):
            continue
        parts = (c.a, c.b, c.c)
        rows.append(dict(entries=sum(len(m) for m in parts), touched=any(s in sub2 for m in parts for s in m),
                         terms=sum(len(sub2[s].to) if s in sub2 else 1 for m in parts for s in m)))
    return dict(n_subs=len(sub2), rows=rows)


def linear_rounds(sys_: "R.System", rounds, old=False) -> int:
    """How many times pyref.simplification runs linear_simplification: what rs_stats.rounds counts."""
    n = [0]
    real = R.linear_simplification

    def counting(*a, **kw):
        n[0] += 1
        return real(*a, **kw)
    R.linear_simplification = counting
    try:
        R.simplification(sys_, R.Flags(no_rounds=(1 << 64) - 1 if rounds is None else rounds, use_old_heuristics=old))
    finally:
        R.linear_simplification = real
    return n[0]


def log_diff(got, ref) -> Optional[str]:
    """None when two logs [(from, {signal: value})] are equal entry for entry -- `from`, the keys, the
    values (zeros included) and the order --, else the first difference."""
    if len(got) != len(ref):
        return f"{len(got)} entries vs {len(ref)}"
    for i, (x, y) in enumerate(zip(got, ref)):
        if x != y:
            return f"entry {i}: {x} vs {y}"
    return None


def zero_keys(to: dict) -> List[int]:
    """The zero-valued non-constant keys of a right-hand side (the constant slot is 0 in every
    substitution without a constant term, so it tells nothing)."""
    return sorted(s for s, v in to.items() if s != 0 and v == 0)


def zero_entries(log) -> List[int]:
    """The positions of the log entries that hold a zero-valued non-constant key."""
    return [i for i, (_, to) in enumerate(log) if zero_keys(to)]


def pruned(log):
    """The log an implementation that dropped zero-valued non-constant keys would write."""
    return [(frm, {s: v for s, v in to.items() if s == 0 or v != 0}) for frm, to in log]


def log_family(name: str) -> str:
    """The family of a case of CASES, by the part of the table that makes it."""
    for pre in ("row", "merge", "compose", "giant", "round2", "frames"):
        if name.startswith(pre + "_"):
            return pre
    return "cluster"


# ============================================================================ the cases
class Case:
    """One boundary case: build() -> (System, info); certify(sys, info, old) -> [(what, got, want)];
    gpu variants: primes, old-heuristics flags, rounds (--O2round N, None = --O2); stats(old) ->
    {rs_stats field: value}; n_rounds: {rounds flag: linear rounds the run makes} where the CPU
    proof counts them (linear_rounds), asserted against rs_stats.rounds on the GPU."""

    def __init__(self, name: str, build: Callable, certify: Callable, primes=("bn128",), olds=(False,),
                 rounds=(None,), stats: Optional[Callable] = None, n_rounds: Optional[dict] = None):
        self.name, self.build, self.certify = name, build, certify
        self.primes, self.olds, self.rounds, self.stats = primes, olds, rounds, stats
        self.n_rounds = n_rounds
        assert n_rounds is None or set(n_rounds) == set(rounds)

    def __repr__(self):
        return self.name


def _seed(name: str) -> int:
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) & 0xffff


def _the(shapes, n_rows):
    m = [c for c in shapes if c["rows"] == n_rows]
    assert len(m) == 1, f"{len(m)} clusters of {n_rows} rows"
    return m[0]


CASES: List[Case] = []


def _add(*a, **kw):
    CASES.append(Case(*a, **kw))


def _filler_sizes(above: int, count: int):
    return [above + 1 + i for i in range(count)]


def _one_elim(**kw):
    """rs_stats of a run with a single linear round: the cases that carry stats hold only chains,
    blobs and probes, none of whose non-linear rows turns linear (rounds == 1 is itself asserted)."""
    d = dict(rounds=1)
    d.update(kw)
    return d


# ---------------------------------------------------------------- cluster-level boundaries
def _chain_case(name, n, tail=False, primes=("bn128",), olds=(False,), want=None, stats=None, probe_n=None, **chain_kw):
    def build(p):
        b = Builder(_seed(name), p)
        if tail:
            for f in fillers(b, _filler_sizes(n, k.kHeadLimit)):
                b.probes(f["probe"], 1)
        cl = chain(b, n, **chain_kw)
        b.probes(cl["probe"], probe_n)
        return b.system(), cl

    def certify(sys_, cl, old):
        c = _the(cluster_shapes(sys_, old), n)
        got = [("rows", c["rows"], n), ("in the tail", c["rank"] >= k.kHeadLimit, tail), ("workgroup class", c["wg"], want["wg"])]
        for key in ("p4", "order_free", "no_unique", "takeable", "entries"):
            if key in want:
                w = want[key](old) if callable(want[key]) else want[key]
                got.append((key, c[key], w))
        if "entries_below" in want:
            got.append(("entries < kHeavyNnz", c["entries"] < want["entries_below"], True))
        return got
    _add(name, build, certify, primes=primes, olds=olds, stats=stats)


def _cluster_cases():
    for d in (-1, 0, 1):  # kWaveMin: lane kernel | workgroup kernels
        n = k.kWaveMin + d
        _chain_case(f"kWaveMin{d:+d}", n, primes=("bn128", "goldilocks"), olds=(False, True),
                    want=dict(wg=d >= 0, entries_below=k.kHeavyNnz, p4=False),
                    stats=lambda old, d=d: _one_elim(small_launches=int(d < 0), head_launches=int(d >= 0), tail_launches=0,
                                                     max_cluster=k.kWaveMin + d, n_clusters=1))
    for d in (-1, 0, 1):  # kHeavyNnz: a small cluster's entries
        nnz = k.kHeavyNnz + d
        nm = f"kHeavyNnz{d:+d}"

        def build(p, nnz=nnz, nm=nm):
            b = Builder(_seed(nm), p)
            cl = blob(b, 20, nnz)
            b.probes(cl["probe"])
            return b.system(), cl

        def certify(sys_, cl, old, nnz=nnz, d=d):
            c = _the(cluster_shapes(sys_, old), 20)
            return [("rows < kWaveMin", c["rows"] < k.kWaveMin, True), ("entries", c["entries"], nnz), ("workgroup class", c["wg"], d >= 0)]
        _add(nm, build, certify,
             stats=lambda old, d=d: _one_elim(small_launches=int(d < 0), head_launches=int(d >= 0), n_clusters=1))
    for d in (0, 1):  # kClSmall: lane replay | wave replay
        _chain_case(f"kClSmall{d:+d}", k.kClSmall + d, olds=(False, True), want=dict(wg=True, p4=False, order_free=False))
    for d in (-1, 0, 1):  # the reference's 350-row rule
        n = P4_MIN + d
        _chain_case(f"p4_head{d:+d}", n, olds=(False, True), want=dict(wg=True, p4=lambda old, d=d: d >= 0 and not old, order_free=False),
                    stats=lambda old: _one_elim(head_launches=1, tail_launches=0, small_launches=0))
        _chain_case(f"p4_tail{d:+d}", n, tail=True, want=dict(wg=True, p4=d >= 0),
                    stats=lambda old: _one_elim(head_launches=1, tail_launches=1, small_launches=0, n_clusters=k.kHeadLimit + 1))
    _chain_case("p4_order_free", P4_MIN, primes=("bn128", "goldilocks"), unique=True,
                want=dict(wg=True, p4=True, order_free=True, no_unique=0))
    _chain_case("p4_one_ordered_row", P4_MIN, primes=("bn128", "goldilocks"), unique=True, no_unique_rows=(P4_MIN // 2,),
                want=dict(wg=True, p4=True, order_free=False, no_unique=1))
    for d in (-1, 0, 1):  # kFinWaveBelow: the tail's finish on one wave | the workgroup
        _chain_case(f"kFinWaveBelow{d:+d}", k.kFinWaveBelow + d, tail=True, want=dict(wg=True, p4=True))
    # kClMid (wave | host replay) and kWideMin (k_big_prep | the k_wide_* grid): one value today, so the
    # same cases cover both; should they part, kWideMin gets its own
    for nm, n0 in [("kClMid", k.kClMid)] + ([("kWideMin", k.kWideMin)] if k.kWideMin != k.kClMid else []):
        for d in (-1, 0, 1):
            _chain_case(f"{nm}_ordered{d:+d}", n0 + d, want=dict(wg=True, p4=True, order_free=False))
            _chain_case(f"{nm}_order_free{d:+d}", n0 + d, unique=True, want=dict(wg=True, p4=True, order_free=True))
    for d in (-1, 0, 1):  # kHeadLimit: the head takes that many clusters
        cnt = k.kHeadLimit + d
        nm = f"kHeadLimit{d:+d}"

        def build(p, cnt=cnt, nm=nm):
            b = Builder(_seed(nm), p)
            for f in fillers(b, [k.kWaveMin + i for i in range(cnt)]):
                b.probes(f["probe"], 2)
            return b.system(), None

        def certify(sys_, info, old, cnt=cnt):
            sh = cluster_shapes(sys_, old)
            return [("clusters", len(sh), cnt), ("all workgroup class", all(c["wg"] for c in sh), True),
                    ("distinct sizes", len({c["rows"] for c in sh}), cnt),
                    ("tail clusters", sum(c["rank"] >= k.kHeadLimit for c in sh), max(0, cnt - k.kHeadLimit)),
                    ("the tail one is the smallest", [c["rows"] for c in sh if c["rank"] >= k.kHeadLimit],
                     [k.kWaveMin] * max(0, cnt - k.kHeadLimit))]
        _add(nm, build, certify,
             stats=lambda old, cnt=cnt: _one_elim(head_launches=1, tail_launches=int(cnt > k.kHeadLimit), small_launches=0, n_clusters=cnt))
    for d in (0, 1):  # kTailSplit: one tail group | two
        n_tail = k.kTailSplit + k.kTailSplit // 4 + d
        nm = f"kTailSplit{d:+d}"

        def build(p, n_tail=n_tail, nm=nm):
            b = Builder(_seed(nm), p)
            for f in fillers(b, [k.kWaveMin + 1] * k.kHeadLimit + [k.kWaveMin] * n_tail):
                b.probes(f["probe"][:8], 1)
            return b.system(), None

        def certify(sys_, info, old, n_tail=n_tail):
            sh = cluster_shapes(sys_, old)
            tail = [c for c in sh if c["rank"] >= k.kHeadLimit]
            return [("tail clusters", len(tail), n_tail), ("all workgroup class", all(c["wg"] for c in sh), True),
                    ("tail rows", {c["rows"] for c in tail}, {k.kWaveMin})]
        _add(nm, build, certify,
             stats=lambda old, d=d: _one_elim(head_launches=1, tail_launches=1 + d, small_launches=0))
    for d in (-1, 0, 1):  # kSpecTabMax: the speculative loop | its one-wave fallback
        n_sig = k.kSpecTabMax + d
        rows4 = k.kSpecTabMax - 800       # process_4: rows + 1 + n_w + extra_shared distinct takeable signals
        assert P4_MIN <= rows4 < k.kGiantRows
        _chain_case(f"kSpecTabMax_p4{d:+d}", rows4, n_w=50, extra_shared=n_sig - (rows4 + 1) - 50,
                    want=dict(wg=True, p4=True, takeable=n_sig, order_free=False),
                    stats=lambda old: _one_elim(giant_launches=0, head_launches=1))
        rows3 = k.kSpecTabMax // 3 - 3    # old heuristics, process_3: the sum of the row lengths
        _chain_case(f"kSpecTabMax_p3{d:+d}", rows3, olds=(True,), const_rows=n_sig - 3 * rows3,
                    want=dict(wg=True, p4=False, entries=n_sig),
                    stats=lambda old: _one_elim(giant_launches=0, head_launches=1))
    for d in (-1, 0, 1):  # kGiantRows: the giant path
        _chain_case(f"kGiantRows{d:+d}", k.kGiantRows + d, olds=(False, True), want=dict(wg=True, order_free=False),
                    stats=lambda old, d=d: _one_elim(giant_launches=int(d >= 0), head_launches=1))
    _chain_case("kGiantRows_order_free", k.kGiantRows, olds=(False, True), unique=True,
                want=dict(wg=True, order_free=lambda old: not old),
                stats=lambda old: _one_elim(giant_launches=int(old), head_launches=1))
    for d in (0, 1):  # kClLds: LDS / host replay | the lane replay in global memory
        _chain_case(f"kClLds{d:+d}", k.kClLds + d, olds=(False, True), want=dict(wg=True, order_free=False), probe_n=400,
                    stats=lambda old: _one_elim(giant_launches=1))


# ---------------------------------------------------------------- row-length and work-list boundaries
PLACEMENTS = ("small", "tail", "head", "head512")


def _placed(b: Builder, where: str):
    """The cluster a long row goes into, in one of the four placements, and whether it is process_4.
      small    fewer than kWaveMin rows (its entries make it workgroup class: the last of the head)
      tail     a process_3 cluster behind kHeadLimit larger fillers: k_big_main<tail_cap>
      head     a process_4 cluster of 600 rows: the speculative loop
      head512  a process_4 head cluster of more than kSpecTabMax signals: d_big_main_cluster<spec_cap>"""
    glue = b.forbid(1)[0]
    if where == "small":
        n = 20
    elif where == "tail":
        n = k.kWaveMin + 8
        for f in fillers(b, _filler_sizes(n + 3, k.kHeadLimit)):
            b.probes(f["probe"], 1)
    elif where == "head":
        n = 600
    else:
        n = k.kSpecTabMax - 800
    low = b.take(k.spec_cap + 8) if where in ("small", "tail") else None   # ids below the chain's
    if where == "head512":
        cl = chain(b, n, n_w=50, extra_shared=900, glue=glue)
    else:
        cl = chain(b, n, glue=glue)
    cl["low"], cl["glue"], cl["where"] = low, glue, where
    b.probes(cl["probe"])
    return cl


def _placement_checks(c, where, old=False):
    got = [("in the tail", c["rank"] >= k.kHeadLimit, where == "tail"), ("workgroup class", c["wg"], True),
           ("p4", c["p4"], where in ("head", "head512"))]
    if where == "small":
        got.append(("rows < kWaveMin", c["rows"] < k.kWaveMin, True))
    if where == "head":
        got.append(("signals <= kSpecTabMax", c["takeable"] <= k.kSpecTabMax, True))
    if where == "head512":
        got += [("signals > kSpecTabMax", c["takeable"] > k.kSpecTabMax, True), ("rows < kGiantRows", c["rows"] < k.kGiantRows, True)]
    return got


def _row_case(name, where, length):
    def build(p):
        b = Builder(_seed(name), p)
        cl = _placed(b, where)
        wide_row(b, cl, length, fresh_ok=where in ("small", "tail"), contiguous=where == "head512")
        cl["n"] += 1
        return b.system(), cl

    def certify(sys_, cl, old):
        c = _the(cluster_shapes(sys_, old), cl["n"])
        tr = elimination_trace(cluster_rows(sys_, c), sys_.forbidden, sys_.p, c["p4"])
        return _placement_checks(c, where) + [("longest row", c["max_row_len"], length),
                                              ("longest row reaches the ordered loop", max(tr["pops"]), length)]
    _add(name, build, certify)


def _merge_case(name, where, total, cap):
    def build(p):
        b = Builder(_seed(name), p)
        cl = _placed(b, where)
        merge_pair(b, cl["glue"], total // 2, total - total // 2)
        cl["n"] += 2
        return b.system(), cl

    def certify(sys_, cl, old):
        c = _the(cluster_shapes(sys_, old), cl["n"])
        tr = elimination_trace(cluster_rows(sys_, c), sys_.forbidden, sys_.p, c["p4"])
        big = [m for m in tr["merges"] if m[0] + m[1] >= cap - 8]
        return _placement_checks(c, where) + [("conflicts near the capacity", len(big), 1),
                                              ("work + right-hand side", big[0][0] + big[0][1] if big else None, total),
                                              ("right-hand side <= capacity", bool(big) and big[0][1] <= cap, True)]
    _add(name, build, certify)


def _giant_row_case(name, length=None, pair=None):
    n = k.kGiantRows

    def build(p):
        b = Builder(_seed(name), p)
        glue = b.forbid(1)[0]
        cl = chain(b, n, glue=glue)
        b.probes(cl["probe"])
        if length is not None:
            wide_row(b, cl, length)
            cl["n"] += 1
        else:
            merge_pair(b, glue, pair[0], pair[1])
            cl["n"] += 2
        return b.system(), cl

    def certify(sys_, cl, old):
        c = _the(cluster_shapes(sys_, old), cl["n"])
        got = [("rows >= kGiantRows", c["rows"] >= k.kGiantRows, True), ("ordered", c["order_free"], False), ("p4", c["p4"], True)]
        if length is not None:
            return got + [("longest row", c["max_row_len"], length), ("it has no signal of its own", c["no_unique"] >= n - 1, True)]
        tr = elimination_trace(cluster_rows(sys_, c), sys_.forbidden, sys_.p, True)
        big = [m for m in tr["merges"] if set(m) == set(pair)]
        return got + [("the pair's conflict", len(big), 1), ("(work, right-hand side) as a set", set(big[0]) if big else None, set(pair))]
    _add(name, build, certify, stats=lambda old: _one_elim(giant_launches=1))


def _row_cases():
    lengths = [k.kSpecK - 1, k.kSpecK, k.kSpecK + 1, k.tail_cap, k.tail_cap + 1, k.spec_cap, k.spec_cap + 1]
    for where in ("small", "tail", "head"):
        for ln in lengths:
            _row_case(f"row_{where}_{ln}", where, ln)
    for ln in (k.spec_cap, k.spec_cap + 1):
        _row_case(f"row_head512_{ln}", "head512", ln)
    for where in ("small", "tail", "head"):
        for cap in (k.tail_cap, k.spec_cap):
            for d in (0, 1, 2):
                _merge_case(f"merge_{where}_{cap}{d:+d}", where, cap + d, cap)
    for d in (0, 1, 2):
        _merge_case(f"merge_head512_{k.spec_cap}{d:+d}", "head512", k.spec_cap + d, k.spec_cap)
    for d in (0, 1):
        _giant_row_case(f"giant_row_{k.kGhRowMax + d}", length=k.kGhRowMax + d)
    # a work row of `live` entries against a right-hand side rl: live - 1 + rl <= kGhRowMax | above
    half = k.kGhRowMax // 2
    for d in (0, 1):
        _giant_row_case(f"giant_merge_sum{d:+d}", pair=(half, k.kGhRowMax + 1 - half + d))
    # the right-hand side alone at kGhRhsMax | above.  kGhRowMax < kGhRhsMax, so `live - 1 + rl >
    # kGhRowMax` already holds for both: the `rl > kGhRhsMax` comparison is dominated, both cases spill,
    # and only giant_merge_sum separates the two branches.  Kept for parity at the named values.
    for d in (0, 1):
        _giant_row_case(f"giant_rhs_{k.kGhRhsMax + d}", pair=(3, k.kGhRhsMax + d))


# ---------------------------------------------------------------- composition boundaries
def _compose_case(name, n_own, n_dep, dep_len, tail):
    pad = k.kWaveMin

    def build(p):
        b = Builder(_seed(name), p)
        n = n_dep + 1 + pad
        if tail:
            for f in fillers(b, _filler_sizes(n, k.kHeadLimit)):
                b.probes(f["probe"], 1)
        cl = dep_sub(b, n_own, n_dep, dep_len, pad)
        b.probes(cl["probe"])
        return b.system(), cl

    def certify(sys_, cl, old):
        c = _the(cluster_shapes(sys_, old), cl["n"])
        cs = compose_shape(sys_, c, cl["s"])
        return [("in the tail", c["rank"] >= k.kHeadLimit, tail), ("workgroup class", c["wg"], True), ("p4", c["p4"], False),
                ("length", cs["length"], n_own + n_dep), ("holder entries", cs["holders"], n_dep), ("own entries", cs["own"], n_own),
                ("E", cs["E"], n_own + n_dep * dep_len)]
    _add(name, build, certify)


def _compose_cases():
    for tail in (False, True):
        t = "tail" if tail else "head"
        for d in (0, 1):        # one lane per entry: length 64 | 65
            _compose_case(f"compose_{t}_len{64 + d}", 64 + d - 6, 6, 3, tail)
        for d in (-1, 0, 1):    # E around kComposeCap (length <= 64)
            e = k.kComposeCap + d
            _compose_case(f"compose_{t}_E{d:+d}", e - 20 * 12, 20, 12, tail)
        for nd in (4, 5):       # the "few runs" switch
            _compose_case(f"compose_{t}_deps{nd}", 10, nd, 8, tail)
        for d in (0, 1):        # kMergeD dependencies | one more (past the sort: length > 64)
            _compose_case(f"compose_{t}_kMergeD{d:+d}", 8, k.kMergeD + d, 5, tail)
        for d in (-1, 0, 1):    # kMergeO own entries
            _compose_case(f"compose_{t}_kMergeO{d:+d}", k.kMergeO + d, 2, 3, tail)
        for d in (-1, 0, 1):    # kMergeK entries in all
            nd, dl = k.kMergeD, 30
            _compose_case(f"compose_{t}_kMergeK{d:+d}", k.kMergeK + d - nd * dl, nd, dl, tail)


# ---------------------------------------------------------------- frames boundaries
def _split(total: int, parts: int) -> List[int]:
    q, r = divmod(total, parts)
    return [q + (i < r) for i in range(parts)]


def _frames_case(name, rows_spec, want_rows=None, want_sum=None, rounds=(None,), n_rounds=None):
    """rows_spec: [(spec_a, spec_b, spec_c)]: the system's non-linear rows are exactly these, in
    order from position 0, so the first 64 share one wave's window of k_frames_wave<0>; every star is a
    one-row lane-class cluster, so no row waits for a head cluster."""
    def build(p):
        b = Builder(_seed(name), p)
        for sa, sb, sc in rows_spec:
            quad(b, sa, sb, sc)
        return b.system(), None

    def certify(sys_, info, old):
        nl = nonlinear_shapes(sys_, old)
        sh = cluster_shapes(sys_, old)
        got = [("non-linear rows", len(nl), len(rows_spec)), ("no workgroup-class cluster", any(c["wg"] for c in sh), False)]
        for key, want in (want_rows or {}).items():
            got.append((f"row 0 {key}", nl[0][key], want))
        for key, want in (want_sum or {}).items():
            got.append((f"first 64 rows' {key}", sum(r[key] or 0 for r in nl[:64]), want))
        return got
    _add(name, build, certify, rounds=rounds, n_rounds=n_rounds or {None: 1})


def _round2_case(name, n_plain, late_lengths, want):
    """One storage row at a limit of k_frames_wave<1>: round 1 turns the late_star rows linear, round 2
    eliminates their signals, and the storage row's terms / entries are the wanted ones only then."""
    def build(p):
        b = Builder(_seed(name), p)
        storage_row(b, n_plain, late_lengths)
        return b.system(), None

    def certify(sys_, info, old):
        r1 = nonlinear_shapes(sys_, old)
        r2 = round2_shapes(sys_, old)
        st = [r for r in r2["rows"] if r["touched"]]
        got = [("round-2 substitutions", r2["n_subs"], len(late_lengths)), ("storage rows round 2 touches", len(st), 1),
               ("round 1 leaves the row alone", (r1[-1]["terms"], r1[-1]["entries"]), (2 + n_plain + len(late_lengths),) * 2)]
        for key, w in want.items():
            got.append((f"round-2 {key}", st[0][key] if st else None, w))
        return got
    _add(name, build, certify, rounds=(None, 2), n_rounds={None: 2, 2: 2})


def _frames_cases():
    for d in (-1, 0, 1):  # one row's terms around kFwT
        t = k.kFwT + d
        _frames_case(f"frames_terms{d:+d}", [(["p"], ["p"], _split(t - 2, 7))], want_rows=dict(terms=t, entries=9))
    for d in (0, 1):      # one row's entries around kFwE
        e = k.kFwE + d
        _frames_case(f"frames_entries{d:+d}", [(["p"], ["p"], ["p"] * (e - 2))], want_rows=dict(entries=e, terms=e))
    per = _split(k.kFwT, 64)
    for d in (0, 1):      # 64 rows whose terms fill one batch exactly | cut it mid-wave
        rows = [(["p"], ["p"], [per[i] - 2 + (d if i == 40 else 0)]) for i in range(64)]
        _frames_case(f"frames_batch_terms{d:+d}", rows, want_sum=dict(terms=k.kFwT + d))
    pe = _split(k.kFwE, 64)
    for d in (0, 1):      # the same for entries
        rows = [(["p"], ["p"], ["p"] * (pe[i] - 2 + (d if i == 40 else 0))) for i in range(64)]
        _frames_case(f"frames_batch_entries{d:+d}", rows, want_sum=dict(entries=k.kFwE + d))
    for d in (0, 1):      # runs in one linear combination: ranked at once | by merge rounds
        r = k.kFwRunsRank + d
        _frames_case(f"frames_runs{d:+d}", [(["p"], ["p", 3], [4] * r)], want_rows=dict(runs=r))
    # 65 rows whose A is one constant term.  The fix queue is per wave and a wave sees one 64-row
    # window at these sizes (one 256-thread block per 256 rows), so the window's 64 rows queue without
    # the `fx_n + nfix > 64` flush and the 65th goes to another wave: the count flush is not reachable
    # from a test-sized input.  The case runs the fix pass with a full queue; the `fx_terms + tsum >
    # kFwT` half of the same test is what frames_fix_terms+1 takes.  (The rows turn linear with forbidden
    # signals only: a second linear round runs and eliminates nothing.)
    _frames_case("frames_fix_65_rows", [(["c"], ["p", "p"], ["p", 3])] * 65, want_sum=dict(fix=64 * 6), n_rounds={None: 2})
    for d in (0, 1):      # constant-A rows whose fix terms fill kFwT exactly | pass it
        tw = _split(k.kFwT, 64)
        rows = [(["c"], ["p"] * (tw[i] // 2), ["p"] * (tw[i] - tw[i] // 2 + (d if i == 63 else 0))) for i in range(64)]
        _frames_case(f"frames_fix_terms{d:+d}", rows, want_sum=dict(fix=k.kFwT + d, terms=k.kFwT + 64 + d), n_rounds={None: 2})
    # rounds >= 2: a storage row at the same limits under k_frames_wave<1>
    for d in (-1, 0, 1):
        t = k.kFwT + d
        _round2_case(f"round2_terms{d:+d}", 0, _split(t - 2, 7), dict(terms=t, entries=9))
    for d in (0, 1):
        e = k.kFwE + d
        _round2_case(f"round2_entries{d:+d}", e - 3, [5], dict(entries=e, terms=e + 4))


_cluster_cases()
_row_cases()
_compose_cases()
_frames_cases()
assert len({c.name for c in CASES}) == len(CASES)


def variants(case: Case):
    """(prime name, old heuristics, rounds) for every GPU run of a case."""
    return [(pr, old, rd) for pr in case.primes for old in case.olds for rd in case.rounds]
