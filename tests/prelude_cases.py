"""Inputs of known shape for everything a run does before its first elimination kernel, and the CPU
proof of that shape (no GPU needed).  Three families, each in the style of dispatch_shapes.py:

  eq_*       the equality classes (run.hpp eq_simplification: one lock-free union-find and per-class
             reductions in place of the reference's single-row and several-row rules,
             constraint_simplification.rs:131-195), the order of the kept forbidden-forbidden
             constraints and of the log, and unions of 8,200 rows in one launch;
  const_* / border
             the constant equalities (last row wins, the batch of eight of k_const_value, duplicates
             that only exist after the renaming) and what both frames leave of a linear or non-linear row;
  order_*    the list order inside a linear cluster -- the replay of the reference's arena merges
             (constraint_simplification.rs:45-99) -- on topologies that are no chain, at the sizes of
             every replay path of cluster.hpp (one lane, one wave, the host, one lane in global memory).

Certificates are plain Python over oracle/pyref.py.  replay_trace restates the arena replay and counts
what the replay kernels branch on; order_sensitivity proves that a case's result changes when the list
order does, so that parity with the oracle pins the order.  tests/test_prelude_cases.py proves every case
on the CPU and tests/test_gpu_prelude.py runs the same cases against the oracle on the GPU."""
from __future__ import annotations

from collections import OrderedDict
from typing import Callable, Dict, List, Optional, Sequence

import dispatch_shapes as ds
import input_contract as ic
import rsio

R = rsio.R
k = ds.k
Builder = ds.Builder
EQ_UNION_ROWS = 8200          # > 8,192: more than 128 waves of rows in one launch of k_eq_union


class Case(ds.Case):
    """A dispatch_shapes.Case plus: family; simplify -- also run through rs_engine_simplify, as given and
    with the keys of every eq row reversed; twice -- run twice on one engine and compare the two runs;
    path -- the replay path of the cluster under test (order_* only)."""

    def __init__(self, name, build, certify, family, primes=("bn128", "goldilocks"), olds=(False,), rounds=(None,),
                 simplify=False, twice=False, path=None):
        super().__init__(name, build, certify, primes=primes, olds=olds, rounds=rounds)
        self.family, self.simplify, self.twice, self.path = family, simplify, twice, path


CASES: List[Case] = []
_BUILT: "OrderedDict" = OrderedDict()


def built(case: Case, prime: str = "bn128"):
    """case.build at a prime, kept for the next few calls (the proofs of one case share it)."""
    key = (case.name, prime)
    if key not in _BUILT:
        _BUILT[key] = case.build(R.PRIMES[prime])
        while len(_BUILT) > 3:
            _BUILT.popitem(last=False)
    return _BUILT[key]


def _add(*a, **kw):
    CASES.append(Case(*a, **kw))


def _edges(p: int) -> List[int]:
    """input_contract.edge_coefficients without 1 and p - 1."""
    return [v for v in ic.edge_coefficients(p) if v not in (1, p - 1)]


# ============================================================================ gadgets: the prelude
def eq(b: Builder, x: int, y: int, kk: int = 1) -> int:
    """The equality kk x - kk y = 0, keys inserted in the order given.  Returns its index in `eq`."""
    p = b.p
    assert x != y and kk % p
    b.rows.append(R.Con({}, {}, {x: kk % p, y: (p - kk) % p}))
    b.n_eq = getattr(b, "n_eq", 0) + 1
    return b.n_eq - 1


def const_row(b: Builder, x: int, kk: int, value: Optional[int]) -> None:
    """The constant equality kk x + c = 0 that defines x = value (value None: kk x alone, x = 0 with an
    empty right-hand side; value 0 has no such row, a zero coefficient is not a valid entry)."""
    p = b.p
    m = {x: kk % p}
    if value is not None:
        c = (p - kk * value) % p
        assert c
        m[0] = c
    b.rows.append(R.Con({}, {}, m))


def cprobes(b: Builder, sigs: Sequence[int], per: int = 4) -> None:
    """Non-linear rows that hold `sigs` in C only, with one plain forbidden signal in A and in B: whatever
    the prelude makes of the signals, the rows stay non-linear, and its substitutions reach the output."""
    sigs = list(sigs)
    for i in range(0, len(sigs), per):
        c = {s: b.coef() for s in sigs[i:i + per]}
        c[0] = b.coef()
        b.nonlin({b.forbid(1)[0]: b.coef()}, {b.forbid(1)[0]: b.coef()}, c)


# ============================================================================ certificates: the prelude
def eq_view(sys_: "R.System") -> dict:
    """pyref's eq_simplification of the system and its equality classes: per class (in order of the
    largest row = cluster index) the rows, the signals, the forbidden ones and the representative by the
    reference's two rules."""
    _, eqs, _, _ = R.classify(sys_)
    forb = set(sys_.forbidden)
    log: list = []
    subs, cons = R.eq_simplification([c.clone() for c in eqs], forb, sys_.max_signal, sys_.p, log)
    parent: Dict[int, int] = {}

    def find(a):
        parent.setdefault(a, a)
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for c in eqs:
        x, y = sorted(c.c)
        parent[find(x)] = find(y)
    by: Dict[int, dict] = {}
    for j, c in enumerate(eqs):
        d = by.setdefault(find(min(c.c)), dict(rows=[], sigs=set()))
        d["rows"].append(j)
        d["sigs"].update(c.c)
    classes = sorted(by.values(), key=lambda d: d["rows"][-1])
    for d in classes:
        f = sorted(s for s in d["sigs"] if s in forb)
        d["forb"] = f
        if len(d["rows"]) == 1:
            x, y = sorted(d["sigs"])
            d["rep"] = None if len(f) == 2 else (f[0] if f else x)
        else:
            d["rep"] = f[0] if f else min(d["sigs"])
        d["subs"] = [s for s in subs if s.frm in d["sigs"]]
        d["cons"] = [c for c in cons if set(c.c) - {0} <= d["sigs"]]
    return dict(eqs=eqs, subs=subs, cons=cons, log=log, classes=classes)


def _class_of(view: dict, sigs) -> dict:
    m = [d for d in view["classes"] if d["sigs"] == set(sigs)]
    assert len(m) == 1, f"{len(m)} classes over {sorted(sigs)}"
    return m[0]


def class_checks(view: dict, p: int, label: str, sigs, rows: int, rep: Optional[int], n_subs: int, n_cons: int):
    """The class over exactly `sigs`: its rows, representative, substitutions (every one `-> rep`) and
    kept constraints (every one rep - f for a class of several rows)."""
    d = _class_of(view, sigs)
    got = [(f"{label}: rows", len(d["rows"]), rows), (f"{label}: representative", d["rep"], rep),
           (f"{label}: substitutions", len(d["subs"]), n_subs), (f"{label}: constraints", len(d["cons"]), n_cons),
           (f"{label}: every substitution is -> rep", all(s.to == {rep: 1} for s in d["subs"]), True)]
    if rows > 1:
        want = [{0: 0, rep: 1, f: p - 1} for f in d["forb"][1:]]
        got.append((f"{label}: constraints are rep - f", [c.c for c in d["cons"]] == want, True))
    return got


def const_view(sys_: "R.System") -> dict:
    """The constant equalities as constant_eq_simplification sees them (after the renaming), its
    substitutions, kept rows and the value each signal ends with (the last row's)."""
    p, forb = sys_.p, set(sys_.forbidden)
    cons_eq, eqs, _, _ = R.classify(sys_)
    subs, _ = R.eq_simplification(eqs, forb, sys_.max_signal, p, None)
    single = R.build_encoded_fast_substitutions(subs)
    for c in cons_eq:
        if R.fast_encoded_constraint_substitution(c, single, p):
            R.fix_constraint(c, p)
    log: list = []
    csubs, kept = R.constant_eq_simplification(cons_eq, forb, p, log)
    enc = R.build_encoded_fast_substitutions(csubs)
    value = {}
    for s, e in enc.items():     # (an empty right-hand side decodes to the linear expression {0: 0})
        value[s] = e.value if e.kind == "Number" else (e.coefs[0] if e.kind == "Linear" and set(e.coefs) == {0} else None)
    return dict(rows=cons_eq, subs=csubs, kept=kept, value=value, log=log, single=single)


def row_kind(c: "R.Con", forb, p: int) -> str:
    """What is left of a row: "empty", "0=c", "forbidden only" (one forbidden signal, no constant),
    "signal" / "signal+c" (one takeable signal), "equality" (two signals, k and -k), "linear" or
    "non-linear"."""
    if not R.is_linear(c):
        return "non-linear"
    if R.is_empty(c):
        return "empty"
    keys = [s for s in c.c if s]
    if not keys:
        return "0=c"
    if len(keys) == 1:
        if keys[0] in forb:
            return "forbidden only" if 0 not in c.c else "forbidden+c"
        return "signal+c" if 0 in c.c else "signal"
    if R.is_equality(c, p):
        return "equality"
    return "linear"


def border_view(sys_: "R.System") -> dict:
    """Every linear row after both frames (linear_after_frames) and every non-linear row after both
    frames and fix_constraint, with pyref's classification of it."""
    p, forb = sys_.p, set(sys_.forbidden)
    linear, non_linear, single, const_subs = ds.linear_after_frames(sys_)
    nl = []
    for c0 in non_linear:
        c = c0.clone()
        for fr in (single, const_subs):
            R.fast_encoded_constraint_substitution(c, fr, p)
        R.fix_constraint(c, p)
        nl.append(c)
    return dict(linear=linear, lin_kinds=[row_kind(c, forb, p) for c in linear], nl=nl, nl_kinds=[row_kind(c, forb, p) for c in nl])


def run_counts(sys_: "R.System", rounds, old: bool, want_log: bool = True) -> dict:
    """One pyref.simplification with its substitution log, counting what rs_stats reports: the linear
    rounds, the linear clusters of all rounds and the rows of the largest."""
    n = dict(rounds=0, n_clusters=0, max_cluster=0)
    real_l, real_f = R.linear_simplification, R.full_simplification

    def lin(*a, **kw):
        n["rounds"] += 1
        return real_l(*a, **kw)

    def full(cluster, *a, **kw):
        n["n_clusters"] += 1
        n["max_cluster"] = max(n["max_cluster"], len(cluster))
        return real_f(cluster, *a, **kw)
    R.linear_simplification, R.full_simplification = lin, full
    try:
        res = R.simplification(sys_, R.Flags(no_rounds=(1 << 64) - 1 if rounds is None else rounds, use_old_heuristics=old),
                               want_log=want_log)
    finally:
        R.linear_simplification, R.full_simplification = real_l, real_f
    n["log"] = rsio.pyref_log(res.log)
    return n


# ============================================================================ certificates: the list order
def replay_trace(keysets: Sequence[Sequence[int]], descending: bool = False) -> dict:
    """The arena replay of build_clusters (constraint_simplification.rs:45-99, Cluster::merge) over rows
    given by their non-constant keys, as cluster.hpp states it: row t starts a list of its own; for each
    of its keys in ascending order (descending: in descending order -- a wrong replay, for
    order_sensitivity) the list of the root of prev(key) is appended to t's, unless that root is already
    in t's list.  Finds halve their paths, as the kernels' do.  -> the lists (one per root, ascending
    root; each in list order, as row indices) and the counters the kernels branch on:
      multi_root_rows  rows that link two or more distinct roots;   max_roots  the most one row links
      max_find         the longest find path (steps to the root, before the find halves it)
      own_pairs        pairs whose root is already in the row's own list (or the row itself)
      max_pairs        the most pairs (keys) in a row
      first_at_63 / straddle / gt64 / gt128
                       window alignment of k_cl_replay_wave over the stream of all rows (every key is one
                       entry): some row's first entry is entry 63 mod 64, some row's entries straddle a
                       64-entry border, some row has more than 64 / more than 128 entries."""
    n = len(keysets)
    c2, tail, nxt = list(range(n)), list(range(n)), [-1] * n
    last: Dict[int, int] = {}
    cnt = dict(multi_root_rows=0, max_roots=0, max_find=0, own_pairs=0, max_pairs=0, first_at_63=False, straddle=False,
               gt64=False, gt128=False, links=0)
    q = 0
    for t, keys in enumerate(keysets):
        keys = sorted(keys, reverse=descending)
        m = len(keys)
        cnt["max_pairs"] = max(cnt["max_pairs"], m)
        if m:
            cnt["first_at_63"] |= q % 64 == 63
            cnt["straddle"] |= q // 64 != (q + m - 1) // 64
            cnt["gt64"] |= m > 64
            cnt["gt128"] |= m > 128
        q += m
        roots = 0
        for s in keys:
            p_ = last.get(s)
            last[s] = t
            if p_ is None:
                continue
            depth, x = 0, p_
            while c2[x] != x:
                x = c2[x]
                depth += 1
            cnt["max_find"] = max(cnt["max_find"], depth)
            while c2[p_] != p_:          # path halving
                g = c2[c2[p_]]
                c2[p_] = g
                p_ = g
            if p_ == t:
                cnt["own_pairs"] += 1
                continue
            nxt[tail[t]] = p_
            tail[t] = tail[p_]
            c2[p_] = t
            roots += 1
        cnt["links"] += roots
        cnt["multi_root_rows"] += roots >= 2
        cnt["max_roots"] = max(cnt["max_roots"], roots)
    lists = []
    for r in range(n):
        if c2[r] == r:
            x, out = r, []
            while x != -1:
                out.append(x)
                x = nxt[x]
            lists.append(out)
    cnt["lists"] = lists
    return cnt


def cluster_view(sys_: "R.System", old: bool, rows: int, linear=None) -> dict:
    """The one cluster of `rows` rows of the system's linear list (after the frames; `linear`: another
    list, a later round's): its shape (cluster_shapes), its rows in build_clusters' list order, and
    replay_trace of its keys, whose order must be that one."""
    if linear is None:
        linear = [c for c in ds.linear_after_frames(sys_)[0] if not R.is_empty(c)]
        shape = ds._the(ds.cluster_shapes(sys_, old), rows)
        ids = shape["row_ids"]
    else:
        shape, ids = None, list(range(len(linear)))
    mine = [linear[j] for j in ids]
    cl = R.build_clusters(mine, sys_.max_signal)
    assert len(cl) == 1 and len(cl[0]) == rows
    at = {id(c): i for i, c in enumerate(mine)}
    arena = [at[id(c)] for c in cl[0]]
    keysets = [[s for s in c.c if s] for c in mine]
    tr = replay_trace(keysets)
    return dict(shape=shape, rows=mine, arena=arena, trace=tr, keysets=keysets)


def order_sensitivity(view: dict, forb, p: int, old: bool) -> dict:
    """pyref's full_simplification of the cluster on its arena order and on three wrong ones: ascending
    row index, descending row index, and the replay that appends each row's lists in descending signal
    order.  -> {wrong order: whether its result differs from the arena order's}."""
    rows = view["rows"]

    def result(order):
        lconst, subs = R.full_simplification([rows[i].clone() for i in order], forb, p, old)
        return [c.c for c in lconst], [(s.frm, s.to) for s in subs]
    n = len(rows)
    wrong = dict(ascending=list(range(n)), descending=list(range(n - 1, -1, -1)),
                 descending_keys=replay_trace(view["keysets"], descending=True)["lists"][0])
    ref = result(view["arena"])
    return {nm: o != view["arena"] and result(o) != ref for nm, o in wrong.items()}


def cost(view: dict, forb, p: int, p4: bool) -> dict:
    """elimination_trace's cost figures: conflict merges, the longest work row and the longest holder."""
    tr = ds.elimination_trace([view["rows"][i] for i in view["arena"]], forb, p, p4)
    return dict(merges=len(tr["merges"]), max_work=max([m[0] for m in tr["merges"]] + tr["pops"] + [0]),
                max_holder=max([len(to) for _, to in tr["holder"].values()] + [0]), leftover=sum(r[3] != "live" for r in tr["results"]))


# ============================================================================ gadgets: the list order
def _row(b: Builder, keys) -> None:
    b.lin(keys, const=len(keys) == 2)


def _chain_rows(b: Builder, m: int, n_w: int = 5):
    """m rows x_i, x_{i+1} and, in every second row, w_{i mod n_w} with the w ids above the x ids
    (dispatch_shapes.chain: shared pivots, so which row is popped first matters).  -> (keysets, x)."""
    x = b.take(m + 1)
    w = b.take(min(n_w, m))
    return [[x[i], x[i + 1]] + ([w[i % len(w)]] if i % 2 == 0 else []) for i in range(m)], x


def tournament(b: Builder, n: int) -> List[List[int]]:
    """Disjoint rows merged pairwise, level by level: ceil(n / 2) leaves v, u, t (u and t spare), then rows
    over one spare signal of each of two clusters (the newest spares first: a leaf's largest signal is
    shared), until one cluster is left; an even n takes one more row over two spares of it."""
    leaves = (n + 1) // 2
    rows, pools = [], []
    for _ in range(leaves):
        v, u, t = b.take(3)
        rows.append([v, u, t])
        pools.append([u, t])
    while len(pools) > 1:
        nxt = []
        for i in range(0, len(pools) - 1, 2):
            a, c = pools[i], pools[i + 1]
            rows.append([a.pop(), c.pop()])
            nxt.append(a + c if len(a) >= len(c) else c + a)
        if len(pools) % 2:
            nxt.append(pools[-1])
        pools = nxt
    if len(rows) < n:
        rows.append([pools[0].pop(0), pools[0].pop(0)])
    assert len(rows) == n
    return rows


def late_star(b: Builder, n: int, j: int) -> List[List[int]]:
    """j chains, then one row of j + 1 keys -- a middle signal of every chain and one of its own -- that
    joins them: that row links j roots, each found from the middle of its chain."""
    assert n - 1 >= 2 * j
    parts = [_chain_rows(b, m) for m in ds._split(n - 1, j)]
    rows = [r for ks, _ in parts for r in ks]
    rows.append([x[len(x) // 2] for _, x in parts] + b.take(1))
    return rows


def interleaved(b: Builder, n: int, j: int) -> List[List[int]]:
    """j chains grown round-robin (row r belongs to chain r mod j) and joined at the end by one row over
    the first signal of every chain: its finds start at each chain's first row."""
    assert n - 1 >= 2 * j
    parts = [_chain_rows(b, m) for m in ds._split(n - 1, j)]
    rows = []
    for i in range(max(len(ks) for ks, _ in parts)):
        rows += [ks[i] for ks, _ in parts if i < len(ks)]
    rows.append([x[0] for _, x in parts] + b.take(1))
    return rows


def sliding(b: Builder, n: int, width: int = 16) -> List[List[int]]:
    """Row i holds three random signals of the window pool[i .. i + width): rows start lists of their own
    and later rows join a random number of them at random depths.  Redrawn until the rows are one cluster."""
    pool = b.take(n + width)
    for _ in range(50):
        rows = [b.rng.sample(pool[i:i + width], 3) for i in range(n)]
        if len(replay_trace(rows)["lists"]) == 1:
            return rows
    raise AssertionError("no connected draw")


def dense(b: Builder, n: int, lo: int = 65, hi: int = 200, groups: int = 4) -> List[List[int]]:
    """Rows of lo to hi keys over small pools: `groups` chains grown round-robin, every row filled up with
    forbidden signals drawn from its group's pool of hi - 2 (forbidden keys are pairs of the stream like
    any other, and glue), and one last row over the first signal of every chain."""
    parts = [_chain_rows(b, m) for m in ds._split(n - 1, groups)]
    pools = [b.forbid(hi - 2) for _ in parts]
    rows = []
    for i in range(max(len(ks) for ks, _ in parts)):
        rows += [ks[i] + b.rng.sample(pool, b.rng.randint(lo, hi) - len(ks[i])) for (ks, _), pool in zip(parts, pools) if i < len(ks)]
    rows.append([x[0] for _, x in parts] + b.take(1))
    return rows


TOPOLOGIES: Dict[str, Callable] = dict(
    tournament=tournament, sliding=sliding, dense=dense,
    interleaved4=lambda b, n: interleaved(b, n, 4), interleaved16=lambda b, n: interleaved(b, n, 16),
    interleaved64=lambda b, n: interleaved(b, n, 64),
    **{f"late_star{j}": (lambda b, n, j=j: late_star(b, n, j)) for j in (2, 16, 63, 64, 65, 130)})


def replay_path(n: int) -> str:
    """The replay a cluster of n rows takes (engine.hip gpu_clusters, cluster.hpp)."""
    if n <= k.kClSmall:
        return "lane"
    if n <= k.kClMid:
        return "wave"
    return "host" if n <= k.kClLds else "lane_global"


def _order_table():
    """(size, topologies): at least two topologies on every path, every late star, the dense rows (more
    than 64 and 128 pairs) on the wave path, the cheapest two at kClLds + 1."""
    return [(k.kClSmall - 1, ("tournament", "interleaved4")), (k.kClSmall, ("late_star2", "sliding", "late_star16")),
            (k.kClSmall + 1, ("tournament", "late_star16")),
            (701, ("late_star63", "late_star64", "late_star65", "late_star130", "dense", "sliding", "interleaved16")),
            (k.kClMid, ("tournament", "dense")), (k.kClMid + 1, ("tournament", "late_star65")),
            (5003, ("interleaved64", "sliding", "late_star16")), (k.kClLds, ("tournament", "interleaved64")),
            (k.kClLds + 1, ("tournament", "late_star64"))]


FORBIDDEN_SHARE = 0.55
SHARES = dict(sliding=0.8)     # (its rows conflict more often: more forbidden signals keep merges <= rows)


def dress(b: Builder, keysets: List[List[int]], share: float = FORBIDDEN_SHARE) -> List[List[int]]:
    """Forbids a random share of the gadget's signals.  A forbidden signal glues like any other,
    so the topology stays; but a row left without a takeable signal goes to the leftover constraints as
    it is, in the order the rows are popped from the list, and a takeable signal that several rows now
    hold as their largest makes them conflict: either way the result follows the list order."""
    own = sorted({s for keys in keysets for s in keys if s not in b.forb})
    b.forb.update(s for s in own if b.rng.random() < share)
    return keysets


def _order_build(name: str, topo: str, n: int):
    def build(p):
        b = Builder(ds._seed(name), p)
        sigs = set()
        for keys in dress(b, TOPOLOGIES[topo](b, n), SHARES.get(topo, FORBIDDEN_SHARE)):
            _row(b, keys)
            sigs.update(s for s in keys if s not in b.forb)
        sigs = sorted(sigs)
        b.probes(sigs, None if len(sigs) <= 2400 else 400)
        return b.system(), dict(n=n, topo=topo)
    return build


_ORDER: Dict[tuple, dict] = {}


def order_proof(case: Case, old: bool) -> dict:
    """Everything the order_* proofs need of one (case, heuristics), computed once: the cluster's view,
    the sensitivity of its result to the list order and its elimination cost."""
    key = (case.name, old)
    if key not in _ORDER:
        sys_, info = built(case)
        if info.get("round2"):
            view = cluster_view(sys_, old, info["n"], linear=round2_linear(sys_))
            p4 = ds.P4_MIN <= info["n"] < ds.P4_END and not old
            of = False
        else:
            view = cluster_view(sys_, old, info["n"])
            p4, of = view["shape"]["p4"], view["shape"]["order_free"]
        _ORDER[key] = dict(view=view, p4=p4, order_free=of, sens=order_sensitivity(view, sys_.forbidden, sys_.p, old),
                           cost=cost(view, sys_.forbidden, sys_.p, p4))
        view["rows"] = None      # (the big ones are not kept)
    return _ORDER[key]


def _order_certify(case_name: str):
    def certify(sys_, info, old):
        pr = order_proof(_BY[case_name], old)
        v, n = pr["view"], info["n"]
        tr = v["trace"]
        got = [("rows", len(v["arena"]), n), ("replay_trace's order is build_clusters'", tr["lists"] == [v["arena"]], True),
               ("no chain: the order is not the descending row index", v["arena"] != list(range(n - 1, -1, -1)), True),
               ("order-free", pr["order_free"], False), ("merges <= rows", pr["cost"]["merges"] <= n, True)]
        if not info["topo"].startswith("dense"):   # (dense rows are longer than kSpecK by construction)
            got.append(("rows and holders under kSpecK", max(pr["cost"]["max_work"], pr["cost"]["max_holder"]) < k.kSpecK, True))
        return got
    return certify


def _order_cases():
    for n, topos in _order_table():
        for topo in topos:
            nm = f"order_{topo}_{n}"
            _add(nm, _order_build(nm, topo, n), _order_certify(nm), "order", primes=("bn128",), olds=(False, True), path=replay_path(n))


# ---------------------------------------------------------------- one run with a cluster of every path
MULTI_SIZES = dict(lane_global=lambda: k.kClLds + 1, host=lambda: k.kClMid + 5, wave=lambda: 701)
MULTI_LANES = 300


def _multi_build(p):
    b = Builder(ds._seed("order_multi"), p)
    sigs = []
    plan = [("tournament", MULTI_SIZES["host"]()), ("late_star16", MULTI_SIZES["wave"]())]
    plan += [(("tournament", "sliding", "late_star2")[i % 3], 5 + (i * 7) % 60) for i in range(MULTI_LANES)]
    plan.insert(150, ("tournament", MULTI_SIZES["lane_global"]()))
    for topo, n in plan:
        keep = []
        for keys in dress(b, TOPOLOGIES[topo](b, n)):
            _row(b, keys)
            keep += [s for s in keys if s not in b.forb][:1]
        sigs += keep[:: max(1, len(keep) // 8)]
    b.probes(sigs)
    return b.system(), dict(sizes=sorted(n for _, n in plan))


def _multi_certify(sys_, info, old):
    sh = ds.cluster_shapes(sys_, old)
    got = [("cluster sizes", sorted(c["rows"] for c in sh), info["sizes"]),
           ("lane clusters", sum(c["rows"] <= k.kClSmall for c in sh), MULTI_LANES),
           ("no cluster is order-free", any(c["order_free"] for c in sh), False)]
    for path, n in MULTI_SIZES.items():
        got.append((f"one cluster on the {path} path", [replay_path(c["rows"]) for c in sh].count(path), 1))
        v = cluster_view(sys_, old, n())
        got.append((f"{path}: replay_trace's order is build_clusters'", v["trace"]["lists"] == [v["arena"]], True))
        got.append((f"{path}: no chain", v["arena"] != list(range(n() - 1, -1, -1)), True))
        got.append((f"{path}: the result follows the list order", all(order_sensitivity(v, sys_.forbidden, sys_.p, old).values()), True))
    return got


# ---------------------------------------------------------------- the host replay of a second round
ROUND2_FIRST = lambda: k.kClMid + 900     # noqa: E731 -- round 1's host-class cluster, the larger one
ROUND2_ROWS = lambda: k.kClMid + 1        # noqa: E731 -- round 2's


def _round2_build(p):
    """Round 1 replays a host-class late star of linear rows.  The rows of a host-class tournament are
    given as non-linear rows whose A is one constant term (dispatch_shapes.late_star's form): round 1's
    fix turns each into the linear row C - s B, over the same keys, and round 2 clusters them."""
    b = Builder(ds._seed("order_round2"), p)
    first = dress(b, late_star(b, ROUND2_FIRST(), 16))
    for keys in first:
        _row(b, keys)
    b.probes(sorted({s for keys in first for s in keys if s not in b.forb})[::7])
    second = dress(b, tournament(b, ROUND2_ROWS()))
    for keys in second:
        c = {s: b.coef() for s in keys[1:]}
        c[0] = b.coef()
        b.nonlin({0: b.coef()}, {keys[0]: b.coef()}, c)
    b.probes(sorted({s for keys in second for s in keys if s not in b.forb})[::7])
    return b.system(), dict(n=ROUND2_ROWS(), topo="tournament", round2=True)


def round2_linear(sys_: "R.System") -> List["R.Con"]:
    """The linear list of round 2: the non-linear rows that fix_constraint turns linear, in row order.
    (Their signals are in no linear row, so round 1 substitutes none of them: asserted.)"""
    lin1 = {s for c in R.classify(sys_)[2] for s in c.c}
    out = []
    for c0 in R.classify(sys_)[3]:
        c = c0.clone()
        R.fix_constraint(c, sys_.p)
        if R.is_linear(c):
            assert not (set(c.c) - {0}) & lin1
            out.append(c)
    return out


def _round2_certify(sys_, info, old):
    got = _order_certify("order_round2")(sys_, info, old)
    sh = ds.cluster_shapes(sys_, old)
    got += [("round 1's cluster", [c["rows"] for c in sh], [ROUND2_FIRST()]),
            ("round 1's cluster is host class and larger", replay_path(ROUND2_FIRST()) == "host" and ROUND2_FIRST() > info["n"], True),
            ("round 1's cluster is ordered", sh[0]["order_free"], False),
            ("round 2's cluster is host class", replay_path(info["n"]), "host"),
            ("round 2's rows", len(round2_linear(sys_)), info["n"])]
    return got


# ============================================================================ the eq cases
def _eq_system(b: Builder, sigs) -> "R.System":
    """Probes over the signals (C only) and two linear rows over some of them, so both frames rename."""
    sigs = sorted(set(sigs))
    cprobes(b, sigs)
    free = [s for s in sigs if s not in b.forb]
    for i in range(0, min(len(free), 12) - 1, 2):
        b.lin([free[i], free[i + 1]] + b.forbid(1))
    return b.system()


def _eq_single_build(p):
    b = Builder(ds._seed("eq_single"), p)
    E = _edges(p)
    I = {}
    a1, a2, a3, a4 = b.take(4)
    eq(b, a2, a1, E[3])                 # free-free, the larger id first
    eq(b, a3, a4, E[11])                # ... and second
    f1 = b.forbid(1)[0]
    x1, x2 = b.take(2)
    f2 = b.forbid(1)[0]
    eq(b, f1, x1)                       # forbidden-free, the forbidden id the smaller
    eq(b, x2, f2, E[20])                # ... and the larger
    I["subs"] = {a2: a1, a4: a3, x1: f1, x2: f2}
    I["multi"], I["kept"] = [], []

    def multi():
        f, x, g = b.forbid(1)[0], b.take(1)[0], b.forbid(1)[0]
        eq(b, f, x)
        eq(b, x, g, E[5])
        I["multi"].append((f, x, g))
    multi()
    g1, g2 = b.forbid(2)
    eq(b, g1, g2, E[7])                 # forbidden-forbidden, k != 1, kept as given
    I["kept"].append(dict(b.rows[-1].c))
    multi()
    g3, g4 = b.forbid(2)
    eq(b, g4, g3, E[-6])                # ... given with descending keys
    I["kept"].append(dict(b.rows[-1].c))
    multi()
    return _eq_system(b, [a1, a2, a3, a4, f1, x1, x2, f2, g1, g2, g3, g4] + [s for t in I["multi"] for s in t]), I


def _eq_single_certify(sys_, I, old):
    v = eq_view(sys_)
    p = sys_.p
    got = [("single-row substitutions", {s.frm: s.to for s in v["subs"] if s.frm in I["subs"]}, {f: {t: 1} for f, t in I["subs"].items()}),
           ("rows", len(v["eqs"]) < 100, True)]
    want = []
    for i, (f, x, g) in enumerate(I["multi"]):
        want.append({0: 0, f: 1, g: p - 1})
        if i < 2:
            want.append(I["kept"][i])
    got += [("kept constraints: the given rows between the classes' constraints", [c.c for c in v["cons"]], want),
            ("kept rows have k != 1", all(val not in (1, p - 1) for m in I["kept"] for val in m.values()), True),
            ("one kept row is given with descending keys", [list(m) == sorted(m) for m in I["kept"]], [True, False])]
    return got


def _eq_multi_build(p):
    b = Builder(ds._seed("eq_multi"), p)
    E = _edges(p)
    C = []     # (label, signals, rows, representative, substitutions, constraints)
    a, c, d = b.take(3)
    eq(b, a, c)
    eq(b, c, d, E[2])
    C.append(("no forbidden", [a, c, d], 2, a, 2, 0))
    f = b.forbid(1)[0]
    a, c = b.take(2)
    eq(b, c, a, E[4])
    eq(b, a, f)
    C.append(("one forbidden", [f, a, c], 2, f, 2, 0))
    f = b.forbid(1)[0]
    a = b.take(1)[0]
    g = b.forbid(1)[0]
    eq(b, f, a)
    eq(b, a, g, E[6])
    C.append(("two forbidden", [f, a, g], 2, f, 1, 1))
    f3 = b.forbid(3)
    eq(b, f3[2], f3[1], E[8])
    eq(b, f3[1], f3[0])
    C.append(("all forbidden", f3, 2, f3[0], 0, 2))
    a = b.take(1)[0]
    f = b.forbid(1)[0]
    c = b.take(1)[0]
    eq(b, a, f, E[9])
    eq(b, f, c)
    C.append(("the smallest forbidden id is not the smallest id", [a, f, c], 2, f, 2, 0))
    s5 = b.take(5)
    eq(b, s5[2], s5[3])
    eq(b, s5[0], s5[2], E[10])
    eq(b, s5[3], s5[4])
    eq(b, s5[1], s5[4])
    C.append(("the representative is in neither the first nor the last row", s5, 4, s5[0], 4, 0))
    f, g = b.forbid(2)
    x = b.take(1)[0]
    eq(b, g, f, E[12])                  # its own coefficients must not come out
    eq(b, g, x)
    C.append(("a forbidden-forbidden row inside a class", [f, g, x], 2, f, 1, 1))
    a, c = b.take(2)
    eq(b, a, c, E[13])
    eq(b, c, a, E[14])
    C.append(("the same equality twice", [a, c], 2, a, 1, 0))
    t3 = b.take(3)
    eq(b, t3[0], t3[1])
    eq(b, t3[1], t3[2], E[15])
    eq(b, t3[2], t3[0], E[16])
    C.append(("a row that closes a cycle", t3, 3, t3[0], 2, 0))
    a, c = b.take(2)
    eq(b, 1, a)
    eq(b, a, 2, E[17])
    eq(b, c, 3)
    eq(b, c, a)
    C.append(("public signals", [1, 2, 3, a, c], 4, 1, 2, 2))
    a = b.take(1)[0]
    sigs = [s for cl in C for s in cl[1]]
    cprobes(b, sigs)
    top = b.take(2)                     # the last ids: max_signal - 1 is in a class
    eq(b, top[1], a, E[18])
    eq(b, a, top[0])
    b.nonlin({1: b.coef()}, {2: b.coef()}, {s: b.coef() for s in [a] + top})
    C.append(("signal max_signal - 1", [a] + top, 2, a, 2, 0))
    sys_ = b.system()
    assert top[1] == sys_.max_signal - 1
    return sys_, C


def _eq_multi_certify(sys_, C, old):
    v = eq_view(sys_)
    got = [("classes", len(v["classes"]), len(C)), ("rows", len(v["eqs"]) < 100, True)]
    for label, sigs, rows, rep, n_subs, n_cons in C:
        got += class_checks(v, sys_.p, label, sigs, rows, rep, n_subs, n_cons)
    rep_rows = _class_of(v, C[5][1])["rows"]
    got.append(("the representative's only row is a middle one",
                [j for j in rep_rows if C[5][3] in v["eqs"][j].c] == rep_rows[1:2], True))
    return got


def _eq_order_build(p):
    """Three classes of several rows, each with a forbidden pair, whose first rows come in the order A, B,
    C, whose last rows in the order C, B, A and whose representatives in the order B, C, A; between them
    kept single rows (K) and single-row substitutions (S)."""
    b = Builder(ds._seed("eq_order"), p)
    E = _edges(p)
    fb, gb, fc, gc, fa, ga = b.forbid(6)             # representatives: B < C < A
    xa, xb, xc = b.take(3)
    k1, k2, k3, k4 = b.forbid(4)
    s = b.take(4)
    eq(b, ga, xa)            # 0  A (its second forbidden signal comes first)
    eq(b, fb, xb, E[1])      # 1  B
    eq(b, xc, fc)            # 2  C
    eq(b, s[1], s[0], E[2])  # 3  S
    eq(b, gc, xc, E[3])      # 4  C ends
    eq(b, k2, k1, E[4])      # 5  K
    eq(b, xb, gb)            # 6  B ends
    eq(b, s[2], s[3])        # 7  S
    eq(b, k3, k4, E[5])      # 8  K
    eq(b, xa, fa, E[6])      # 9  A ends
    return _eq_system(b, [fa, ga, fb, gb, fc, gc, xa, xb, xc, k1, k2, k3, k4] + s), dict(multi=[(fa, ga), (fb, gb), (fc, gc)])


def _eq_order_certify(sys_, I, old):
    v = eq_view(sys_)
    first_row: Dict[int, int] = {}
    for j, c in enumerate(v["eqs"]):
        for s in c.c:
            first_row.setdefault(s, j)
    keys = []      # per kept constraint, in pyref's order: (smallest row of its class, first row of its signals, representative)
    for c in v["cons"]:
        sg = set(c.c) - {0}
        d = [d for d in v["classes"] if sg <= d["sigs"]][0]
        keys.append((d["rows"][0], min(first_row[s] for s in sg if s != d["rep"]), d["rep"] if d["rep"] is not None else min(sg)))
    log = [(s.frm, s.to) for s in v["log"]]
    got = [("classes of several rows with a forbidden pair", sum(len(d["rows"]) > 1 and len(d["forb"]) >= 2 for d in v["classes"]), 3),
           ("kept single rows", sum(d["rep"] is None for d in v["classes"]), 2),
           ("single-row substitutions", sum(len(d["rows"]) == 1 and d["rep"] is not None for d in v["classes"]), 2),
           ("kept constraints", len(keys), 5)]
    for i, what in enumerate(("smallest row", "first row", "representative")):
        got.append((f"the constraints are not in the order by {what}", [q[i] for q in keys] != sorted(q[i] for q in keys), True))
    got += [("the log is not sorted by signal", log != sorted(log, key=lambda e: e[0]), True),
            ("the log is not in row order", log != sorted(log, key=lambda e: first_row[e[0]]), True)]
    return got


UNION_SHAPES = ("chain", "chain_reversed", "star_hub_smallest", "star_hub_largest", "pairing_tree", "chain_x8")


def _union_rows(shape: str, s: List[int], n: int):
    if shape == "chain":
        return [(s[i], s[i + 1]) for i in range(n)]
    if shape == "chain_reversed":
        return [(s[i], s[i + 1]) for i in range(n - 1, -1, -1)]
    if shape == "star_hub_smallest":
        return [(s[0], s[i + 1]) for i in range(n)]
    if shape == "star_hub_largest":
        return [(s[n], s[i]) for i in range(n)]
    if shape == "pairing_tree":            # pairs, then pairs of pairs
        rows, level = [], s[:n + 1]
        while len(level) > 1:
            rows += [(level[i], level[i + 1]) for i in range(0, len(level) - 1, 2)]
            level = level[::2]
        return rows
    assert shape == "chain_x8"
    return [(s[i], s[i + 1]) for i in range(n // 8) for _ in range(8)]


def _union_build(name, shape, n_forb):
    def build(p):
        b = Builder(ds._seed(name), p)
        n = EQ_UNION_ROWS
        s = b.take(n + 1)
        rows = _union_rows(shape, s, n)
        used = sorted({x for r in rows for x in r})
        mid = used[len(used) // 2: len(used) // 2 + n_forb]
        b.forb.update(mid)
        for x, y in rows:
            eq(b, x, y, b.coef())
        cprobes(b, b.rng.sample(used, 96) + mid)
        return b.system(), dict(sigs=used, forb=mid, rows=len(rows))
    return build


def _union_certify(sys_, I, old):
    v = eq_view(sys_)
    n_f = len(I["forb"])
    rep = min(I["forb"]) if n_f else min(I["sigs"])
    got = [("rows >= 8,193", I["rows"] >= 8193 and len(v["eqs"]) == I["rows"], True), ("one class", len(v["classes"]), 1),
           ("forbidden signals of the class", v["classes"][0]["forb"], sorted(I["forb"])),
           ("neither is the smallest or the largest id", all(min(I["sigs"]) < f < max(I["sigs"]) for f in I["forb"]), True)]
    return got + class_checks(v, sys_.p, "the class", I["sigs"], I["rows"], rep, len(I["sigs"]) - max(n_f, 1), max(n_f - 1, 0))


def _eq_cases():
    _add("eq_single", _eq_single_build, _eq_single_certify, "eq", simplify=True)
    _add("eq_multi", _eq_multi_build, _eq_multi_certify, "eq", simplify=True)
    _add("eq_order", _eq_order_build, _eq_order_certify, "eq", simplify=True)
    for shape in UNION_SHAPES:
        for n_forb in (0, 2):
            nm = f"eq_union_{shape}_f{n_forb}"
            _add(nm, _union_build(nm, shape, n_forb), _union_certify, "eq", twice=True)


# ============================================================================ the constant cases
def _const_forms_build(p):
    b = Builder(ds._seed("const_forms"), p)
    E = _edges(p)
    x0, x1, xa, xc = b.take(4)
    f0, f1 = b.forbid(2)
    const_row(b, x0, E[3], None)               # k x alone
    const_row(b, xc, E[4], 5)                  # three rows that contradict: 5, 9, 7 -- the last wins,
    const_row(b, x1, E[5], E[6])               # k x + c
    const_row(b, f0, E[7], None)               # forbidden: kept
    const_row(b, xa, 1, 3)                     # two rows that agree
    const_row(b, xc, E[8], 9)                  #   and it is not the one of largest value
    const_row(b, f1, E[9], E[10])              # forbidden with a constant: kept
    const_row(b, xa, 2, 3)
    const_row(b, xc, p - 1, 7)
    sigs = [x0, x1, xa, xc, f0, f1]
    cprobes(b, sigs, per=3)
    b.lin(sigs[:4] + b.forbid(1))
    b.lin([x1, xc] + b.forbid(2), const=True)
    return b.system(), dict(x0=x0, x1=x1, xa=xa, xc=xc, x1v=E[6], kept=[f0, f1])


def _const_forms_certify(sys_, I, old):
    v = const_view(sys_)
    log = [(s.frm, s.to) for s in v["log"]]
    return [("rows", len(v["rows"]), 9), ("substitutions", len(v["subs"]), 7), ("kept rows", [max(c.c) for c in v["kept"]], I["kept"]),
            ("k x alone: logged with an empty right-hand side", [to for f, to in log if f == I["x0"]], [{}]),
            ("k x alone: the value is 0", v["value"][I["x0"]], 0), ("k x + c", v["value"][I["x1"]], I["x1v"]),
            ("the log holds every duplicate", [to[0] for f, to in log if f == I["xc"]], [5, 9, 7]),
            ("the frames use the last row", v["value"][I["xc"]], 7),
            ("the agreeing rows", ([to[0] for f, to in log if f == I["xa"]], v["value"][I["xa"]]), ([3, 3], 3))]


def _const_renamed_build(p):
    b = Builder(ds._seed("const_renamed"), p)
    E = _edges(p)
    a, c = b.take(2)             # a constant on a class representative
    eq(b, c, a, E[1])
    const_row(b, a, E[2], 11)
    a2, c2 = b.take(2)           # on a removed member, after its representative's own row: the member's wins
    eq(b, a2, c2)
    const_row(b, a2, E[3], 21)
    const_row(b, c2, E[4], 22)
    a3, c3 = b.take(2)           # ... and before it: the representative's wins
    eq(b, c3, a3, E[5])
    const_row(b, c3, E[6], 31)
    const_row(b, a3, E[7], 32)
    f = b.forbid(1)[0]           # on a member of a class whose representative is forbidden: stays a constraint
    x = b.take(1)[0]
    eq(b, x, f)
    const_row(b, x, E[8], 41)
    sigs = [a, c, a2, c2, a3, c3, f, x]
    cprobes(b, sigs, per=3)
    b.lin([c, c2, c3] + b.forbid(1))
    b.lin([a, x] + b.forbid(1), const=True)
    return b.system(), dict(rep=a, first=(a2, [21, 22]), second=(a3, [31, 32]), forb=f, kept_row={f: E[8], 0: (p - E[8] * 41) % p})


def _const_renamed_certify(sys_, I, old):
    v = const_view(sys_)
    log = [(s.frm, s.to.get(0)) for s in v["log"]]
    got = [("a constant on a representative", v["value"][I["rep"]], 11), ("kept rows", [c.c for c in v["kept"]], [I["kept_row"]]),
           ("no input row repeats a signal", len({max(c.c) for c in R.classify(sys_)[0]}), 6)]
    for nm in ("first", "second"):
        s, vals = I[nm]
        got += [(f"{nm} pair: two rows on the representative after the renaming", [val for f, val in log if f == s], vals),
                (f"{nm} pair: the later row wins", v["value"][s], vals[1])]
    return got


BATCH_SIZES = (1, 7, 8, 9, 16, 17)


def _batch_coefs(p: int) -> List[int]:
    """1, p - 1 and the limb edges: 2^64 +- 1, 2^128, 2^192 (mod p), and the all-ones words."""
    ones = (1 << 64) - 1
    raw = [1, p - 1, ones, 1 << 64, (1 << 64) + 1, 1 << 128, (1 << 128) - 1, 1 << 192, (1 << 192) - 1, ones << 64, ones << 192,
           p - (1 << 64) % p, (p - 1) // 2]
    return [v % p for v in raw if v % p]


def _const_batch_build(name, n):
    def build(p):
        b = Builder(ds._seed(name), p)
        cf = _batch_coefs(p)
        xs = b.take(n)
        for i, x in enumerate(xs):
            const_row(b, x, cf[i % len(cf)], None if i % 5 == 3 else cf[(3 * i + 1) % len(cf)])
        cprobes(b, xs)
        b.lin(xs[:3] + b.forbid(3))
        return b.system(), dict(n=n, coefs={cf[i % len(cf)] for i in range(n)})
    return build


def _const_batch_certify(sys_, I, old):
    v = const_view(sys_)
    p = sys_.p
    got = [("rows", len(v["rows"]), I["n"]), ("every row defines its signal", len(v["value"]), I["n"]),
           ("batches of eight", -(-len(v["rows"]) // 8), -(-I["n"] // 8))]
    if I["n"] >= 8:
        got.append(("coefficients 1, p - 1 and a limb edge", {1, p - 1, (1 << 64) % p} <= I["coefs"], True))
    return got


def _const_mixed_build(p):
    b = Builder(ds._seed("const_batch_mixed"), p)
    cf = _batch_coefs(p)
    x = b.take(4)
    f = b.forbid(2)
    const_row(b, x[0], cf[2], cf[5])        # defines
    const_row(b, f[0], cf[3], cf[6])        # forbidden
    const_row(b, x[1], cf[1], 8)            # overridden by row 5
    const_row(b, x[2], cf[4], None)         # a zero constant
    const_row(b, x[3], 1, cf[7])            # defines
    const_row(b, x[1], cf[8], 6)            # defines (the last of its signal)
    const_row(b, f[1], p - 1, None)         # forbidden, no constant
    const_row(b, x[0], cf[9], cf[10])       # overrides row 0
    cprobes(b, x + f)
    b.lin(x[:3] + b.forbid(1))
    return b.system(), dict(x=x, last={x[0]: cf[10], x[1]: 6, x[2]: 0, x[3]: cf[7]})


def _const_mixed_certify(sys_, I, old):
    v = const_view(sys_)
    return [("one batch", len(v["rows"]), 8), ("forbidden rows", len(v["kept"]), 2), ("logged rows", len(v["log"]), 6),
            ("overridden rows", len(v["log"]) - len(v["value"]), 2), ("values", v["value"], I["last"])]


def _const_none_build(p):
    b = Builder(ds._seed("const_batch_none"), p)
    cf = _batch_coefs(p)
    f = b.forbid(8)
    for i, s in enumerate(f):
        const_row(b, s, cf[i], None if i % 3 == 0 else cf[i + 2])
    cprobes(b, f)
    return b.system(), None


def _const_none_certify(sys_, I, old):
    v = const_view(sys_)
    return [("one batch", len(v["rows"]), 8), ("no row defines anything", len(v["subs"]), 0), ("kept rows", len(v["kept"]), 8)]


def _border_build(p):
    b = Builder(ds._seed("border"), p)
    E = _edges(p)
    want_lin, want_nl = [], []

    def pair():
        x, y = b.take(2)
        eq(b, y, x, b.coef())
        return x, y

    def const(value):
        z = b.take(1)[0]
        const_row(b, z, b.coef(), value)
        return z
    m1 = p - 1
    x, y = pair()                       # a x - a y + b z, z = 0: vanishes
    b.rows.append(R.Con({}, {}, {x: E[1], y: p - E[1], const(None): E[2]}))
    want_lin.append(("empty", {}))
    x, y = pair()                       # ... z = 5: 0 = 5 b
    b.rows.append(R.Con({}, {}, {x: E[3], y: p - E[3], const(5): 2}))
    want_lin.append(("0=c", {0: 10}))
    x = b.take(1)[0]                    # one signal and a constant
    b.rows.append(R.Con({}, {}, {x: E[4], const(3): 1, 0: 4}))
    want_lin.append(("signal+c", {x: E[4], 0: 7}))
    f = b.forbid(1)[0]                  # one forbidden signal only
    x, y = pair()
    b.rows.append(R.Con({}, {}, {f: E[5], x: m1, y: 1}))
    want_lin.append(("forbidden only", {f: E[5]}))
    u, w = b.take(2)                    # two signals in equality form
    b.rows.append(R.Con({}, {}, {u: E[6], w: p - E[6], const(None): 1}))
    want_lin.append(("equality", {u: E[6], w: p - E[6]}))
    x, y = pair()                       # two keys renamed to one representative, a non-zero sum
    w = b.take(1)[0]
    b.rows.append(R.Con({}, {}, {x: 3, y: 4, w: E[7]}))
    want_lin.append(("linear", {x: 7, w: E[7]}))
    b.n_lin += 6
    z = const(3)                        # the only A signal is a constant: linear in round 1 through frame 2
    u, w, t = b.take(3)
    b.nonlin({z: 2}, {u: 1, w: 5}, {t: 1, 0: 1})
    want_nl.append(("linear", {0: 1, t: 1, u: p - 6, w: p - 30}))
    x, y = pair()                       # two C keys rename to one representative and cancel
    fa, fb, fc = b.forbid(3)
    b.nonlin({fa: E[8]}, {fb: E[9]}, {x: E[10], y: p - E[10], fc: 1})
    want_nl.append(("non-linear", {fc: 1}))
    return b.system(), dict(lin=want_lin, nl=want_nl)


def _border_certify(sys_, I, old):
    v = border_view(sys_)
    return [("linear rows after both frames", list(zip(v["lin_kinds"], [c.c for c in v["linear"]])), I["lin"]),
            ("non-linear rows after both frames", list(zip(v["nl_kinds"], [c.c for c in v["nl"]])), I["nl"]),
            ("A and B of the row that stays", [len(c.a) and len(c.b) for c in v["nl"]], [0, 1])]


def _const_cases():
    _add("const_forms", _const_forms_build, _const_forms_certify, "const")
    _add("const_renamed", _const_renamed_build, _const_renamed_certify, "const", simplify=True)
    for n in BATCH_SIZES:
        nm = f"const_batch_{n}"
        _add(nm, _const_batch_build(nm, n), _const_batch_certify, "const")
    _add("const_batch_mixed", _const_mixed_build, _const_mixed_certify, "const")
    _add("const_batch_none", _const_none_build, _const_none_certify, "const")
    _add("border", _border_build, _border_certify, "const", simplify=True)


_eq_cases()
_const_cases()
_order_cases()
_add("order_multi", _multi_build, _multi_certify, "order", primes=("bn128",), olds=(False, True))
_add("order_round2", _round2_build, _round2_certify, "order", primes=("bn128",), olds=(False, True), path="host")
_BY: Dict[str, Case] = {c.name: c for c in CASES}
assert len(_BY) == len(CASES)


def variants(case: Case):
    """(prime name, old heuristics, rounds) for every GPU run of a case."""
    return ds.variants(case)


# (case, old heuristics) pairs whose result does not change under every wrong list order
# (order_sensitivity): not run on the GPU.  tests/test_prelude_cases.py proves the list exact.
DROPPED: tuple = ()


def expected_stats(case: Case, sys_: "R.System", info, old: bool) -> dict:
    """rs_stats.rounds, n_clusters (summed over the rounds) and max_cluster of a run of the case, from
    cluster_shapes: one linear round over the clusters of the linear list, but for the two cases whose
    non-linear rows turn linear (a second round over them).  tests/test_prelude_cases.py proves the
    figures against a counted pyref run."""
    sh = ds.cluster_shapes(sys_, old)
    d = dict(rounds=1, n_clusters=len(sh), max_cluster=max([c["rows"] for c in sh] + [0]))
    if case.name == "border":          # one row turns linear through frame 2: a cluster of its own in round 2
        d.update(rounds=2, n_clusters=len(sh) + 1)
    if case.name == "order_round2":
        d.update(rounds=2, n_clusters=len(sh) + 1)
    return d


def has_host_replay(case: Case, old: bool) -> bool:
    """Whether a run of the case replays a cluster on the host: a cluster of more than kClMid and at most
    kClLds rows that is not order-free (no order_* cluster is: proved)."""
    return case.path == "host" or case.name == "order_multi"
