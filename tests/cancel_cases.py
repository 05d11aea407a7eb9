"""Inputs in which a coefficient provably cancels inside the path a case names, and the CPU proof.

The dispatch cases draw their coefficients at random, so nothing in them certifies a cancellation.
CANCEL_CASES (the Case class of dispatch_shapes.py) places one on every elimination path:

  merges        cancel_pair in the four placements of dispatch_shapes._placed and on the giant chain:
                a conflict merge whose result is empty (0 = 0, dropped), a non-zero constant alone
                (0 = c, a leftover row) or one forbidden key (length - 1 terms cancel);
  compositions  dep_sub(cancel=2, inherit=True) twins of one composition case per implementation,
                a lane-class one, a process_4 one and one on the giant chain: the composed right-hand
                side of s holds explicit zero keys (raw_substitution prunes nothing), t inherits them,
                and only the substitution log shows them; zero_sub per class: every key of s cancels;
  frames        twin_stars in A and / or C of a non-linear row of round 1 and, with late twins, of
                round 2: A vanishes, A is left a bare constant, C vanishes, the row disappears.

tests/test_cancel_cases.py proves each case on the CPU, tests/test_gpu_cancel.py runs it."""
from __future__ import annotations

from typing import List

import dispatch_shapes as ds
import rsio
from dispatch_shapes import Builder, Case, _filler_sizes, _one_elim, _placed, _placement_checks, _seed, _the, k

R = rsio.R
PRIMES = ("bn128", "goldilocks")
PAIR_LEN = 8
CANCEL_CASES: List[Case] = []


def _add(*a, **kw):
    kw.setdefault("primes", PRIMES)
    CANCEL_CASES.append(Case(*a, **kw))


def _leftover_rows(sys_, shape):
    """The rows the cluster's ordered loop leaves over (no takeable signal), as pyref makes them."""
    cl = ds.cluster_rows(sys_, shape)
    if shape["p4"]:
        return R.substitution_process_4(sys_.forbidden, cl, {}, sys_.p)[0]
    return R.substitution_process_3(sys_.forbidden, cl, {}, sys_.p)


def leftovers(sys_, shape) -> int:
    return len(_leftover_rows(sys_, shape))


def constant_rows(sys_, old=False) -> int:
    """pyref's result rows whose only key is the constant (0 = c)."""
    res = R.simplification(sys_, R.Flags(use_old_heuristics=old))
    return sum(1 for c in res.constraints if not c.a and not c.b and set(c.c) == {0})


# ---------------------------------------------------------------- conflict merges that cancel
MERGE_KIND = {"empty": ("empty", 0), "const": ("const", 1), "partial": ("forbidden", 1)}   # merge_kind, result length


def _merge_checks(sys_, bare, c, c0, kind, pair):
    tr = ds.elimination_trace(ds.cluster_rows(sys_, c), sys_.forbidden, sys_.p, c["p4"])
    want, rlen = MERGE_KIND[kind]
    hits = [r for r in tr["results"] if r[3] == want]
    got = [(f"merges that end {want}", len(hits), 1),
           ("work + right-hand side", hits[0][0] + hits[0][1] if hits else None, pair["work_plus_rhs"]),
           ("right-hand side", hits[0][1] if hits else None, PAIR_LEN),
           ("merged row", hits[0][2] if hits else None, rlen),
           ("leftover rows beyond the cluster's without the pair", leftovers(sys_, c) - leftovers(bare, c0), int(kind != "empty")),
           ("result rows 0 = c", constant_rows(sys_), int(kind == "const"))]
    if kind == "partial":
        got.append(("the surviving key", [set(r.c) for r in _leftover_rows(sys_, c)].count({pair["survivor"]}), 1))
    return got


def _cancel_merge_case(kind, where):
    name = f"cancel_{kind}_{where}"

    def build(p, with_pair=True):
        b = Builder(_seed(name), p)
        cl = _placed(b, where)
        if where == "small":   # entries, not rows, make it workgroup class: one long row with a signal of its own
            b.lin([b.take(1)[0], cl["glue"]] + b.forbid(k.kHeavyNnz))
            cl["n"] += 1
        if with_pair:
            cl["pair"] = ds.cancel_pair(b, cl["glue"], PAIR_LEN, kind)
            cl["n"] += 2
        return b.system(), cl

    def certify(sys_, cl, old):
        bare, cl0 = build(sys_.p, with_pair=False)
        c, c0 = _the(ds.cluster_shapes(sys_, old), cl["n"]), _the(ds.cluster_shapes(bare, old), cl0["n"])
        return _placement_checks(c, where) + [("rows without the pair", c0["rows"], c["rows"] - 2)] + \
            _merge_checks(sys_, bare, c, c0, kind, cl["pair"])
    _add(name, build, certify)


def _cancel_giant_case(kind):
    name = f"cancel_{kind}_giant"
    n = k.kGiantRows

    def build(p, with_pair=True):
        b = Builder(_seed(name), p)
        glue = b.forbid(1)[0]
        cl = ds.chain(b, n, glue=glue)
        b.probes(cl["probe"])
        if with_pair:
            cl["pair"] = ds.cancel_pair(b, glue, PAIR_LEN, kind)
            cl["n"] += 2
        return b.system(), cl

    def certify(sys_, cl, old):
        bare, cl0 = build(sys_.p, with_pair=False)
        c, c0 = _the(ds.cluster_shapes(sys_, old), cl["n"]), _the(ds.cluster_shapes(bare, old), cl0["n"])
        return [("rows >= kGiantRows", c["rows"] >= k.kGiantRows, True), ("ordered", c["order_free"], False), ("p4", c["p4"], True),
                ("rows without the pair", c0["rows"], c["rows"] - 2)] + _merge_checks(sys_, bare, c, c0, kind, cl["pair"])
    _add(name, build, certify, stats=lambda old: _one_elim(giant_launches=1))


# ---------------------------------------------------------------- compositions that keep explicit zeros
def zero_checks(sys_, cl, old, m):
    """pyref's log entry of s holds exactly the m zero keys the gadget built, t's the same ones, and the
    log with such keys pruned differs from the literal log in exactly the entries that hold one (the
    vacuity guard: an implementation that prunes cannot pass)."""
    log = rsio.pyref_log(R.simplification(sys_, R.Flags(use_old_heuristics=old), want_log=True).log)
    by = {frm: to for frm, to in log}
    assert len(by) == len(log)
    zs = sorted(cl["zeros"])
    pr = ds.pruned(log)
    differs = [i for i in range(len(log)) if log[i] != pr[i]]
    return [("zero keys", len(zs), m), ("zero keys of s", ds.zero_keys(by[cl["s"]]), zs), ("zero keys of t", ds.zero_keys(by[cl["t"]]), zs),
            ("every other key of s is non-zero", sum(1 for q, v in by[cl["s"]].items() if q and v), len(by[cl["s"]]) - 1 - m),
            ("the pruned log differs exactly where a zero key is", differs, ds.zero_entries(log)),
            ("s and t are among them", {log[i][0] for i in differs} >= {cl["s"], cl["t"]}, True)]


def _twin_case(name, twin_of, n_own, n_dep, dep_len, tail, relation, pad=None, lane=False):
    """dep_sub(cancel=2, inherit=True) at the numbers of the composition case `twin_of`; relation:
    [(what, function of compose_shape's dict, wanted)] -- the side of each constant, stated."""
    pad = k.kWaveMin if pad is None else pad

    def build(p):
        b = Builder(_seed(name), p)
        n = n_dep + 2 + pad
        if tail:
            for f in ds.fillers(b, _filler_sizes(n, k.kHeadLimit)):
                b.probes(f["probe"], 1)
        cl = ds.dep_sub(b, n_own, n_dep, dep_len, pad, cancel=2, inherit=True)
        b.probes(cl["probe"])
        return b.system(), cl

    def certify(sys_, cl, old):
        c = _the(ds.cluster_shapes(sys_, old), cl["n"])
        cs = ds.compose_shape(sys_, c, cl["s"])
        got = [("in the tail", c["rank"] >= k.kHeadLimit, tail), ("workgroup class", c["wg"], not lane), ("p4", c["p4"], False),
               ("length", cs["length"], n_own + n_dep), ("holder entries", cs["holders"], n_dep), ("own entries", cs["own"], n_own),
               ("E", cs["E"], n_own + n_dep * dep_len)]
        if lane:
            got += [("rows < kWaveMin", c["rows"] < k.kWaveMin, True), ("entries < kHeavyNnz", c["entries"] < k.kHeavyNnz, True)]
        got += [(what, f(cs), want) for what, f, want in relation]
        return got + zero_checks(sys_, cl, old, 2)
    _add(name, build, certify, stats=(lambda old: _one_elim(small_launches=1, head_launches=0, n_clusters=1)) if lane else None)
    CANCEL_CASES[-1].twin_of = twin_of


def _twin_cases():
    for tail in (False, True):
        t = "tail" if tail else "head"
        cap, mk, mo, md = k.kComposeCap, k.kMergeK, k.kMergeO, k.kMergeD
        # the numbers of dispatch_shapes._compose_cases; kMergeO+1 has four dependencies where its twin-of
        # has two (two pairs need four): own = kMergeO + 1 is what d_compose_merge refuses either way
        _twin_case(f"zero_{t}_len64", f"compose_{t}_len64", 58, 6, 3, tail,
                   [("length <= 64", lambda s: s["length"] <= 64, True), ("E <= kComposeCap", lambda s: s["E"] <= cap, True)])
        _twin_case(f"zero_{t}_len65", f"compose_{t}_len65", 59, 6, 3, tail,
                   [("length > 64", lambda s: s["length"], 65), ("holders <= kMergeD", lambda s: s["holders"] <= md, True),
                    ("own <= kMergeO", lambda s: s["own"] <= mo, True), ("E <= kMergeK", lambda s: s["E"] <= mk, True)])
        _twin_case(f"zero_{t}_E+1", f"compose_{t}_E+1", cap + 1 - 240, 20, 12, tail,
                   [("length <= 64", lambda s: s["length"] <= 64, True), ("E", lambda s: s["E"], cap + 1)])
        _twin_case(f"zero_{t}_kMergeD+1", f"compose_{t}_kMergeD+1", 8, md + 1, 5, tail,
                   [("length > 64", lambda s: s["length"] > 64, True), ("holders", lambda s: s["holders"], md + 1)])
        _twin_case(f"zero_{t}_kMergeO+1", f"compose_{t}_kMergeO+1", mo + 1, 4, 3, tail,
                   [("length > 64", lambda s: s["length"] > 64, True), ("own", lambda s: s["own"], mo + 1),
                    ("holders <= kMergeD", lambda s: s["holders"] <= md, True), ("E <= kMergeK", lambda s: s["E"] <= mk, True)])
        _twin_case(f"zero_{t}_kMergeK+1", f"compose_{t}_kMergeK+1", mk + 1 - md * 30, md, 30, tail,
                   [("length > 64", lambda s: s["length"] > 64, True), ("E", lambda s: s["E"], mk + 1),
                    ("holders <= kMergeD", lambda s: s["holders"] <= md, True), ("own <= kMergeO", lambda s: s["own"] <= mo, True)])
    # the lane kernel's d_raw_sub_into
    _twin_case("zero_lane", None, 4, 6, 4, False, [], pad=4, lane=True)


def _s_row_first(b: Builder, cl: dict, n_dep: int) -> int:
    """process_4 pops a cluster's rows oldest first (build_clusters puts a joining row in front), and a
    row popped after its holders' rows conflicts with them one by one -- merges, which drop zeros --
    instead of keeping them as entries.  With s's row ahead of its dependencies' rows s is taken
    first (it has the fewest occurrences), the holders after it, and the composition in deletion order
    meets every holder final.  Moves the row and returns a forbidden signal of it to glue a chain to."""
    assert b.n_nl == 0 and cl["first"] + n_dep < len(b.rows)
    row = b.rows.pop(cl["first"] + n_dep)
    assert cl["s"] in row.c
    b.rows.insert(cl["first"], row)
    return min(set(row.c) & b.forb - {0})


def _zero_p4_case():
    """dep_sub's rows glued to a 350-row ordered chain: a process_4 head cluster, composed in its deletion
    order (create_nonoverlapping_substitutions_4)."""
    name, n_own, n_dep, dep_len = "zero_p4_head", 6, 6, 4

    def build(p):
        b = Builder(_seed(name), p)
        cl = ds.dep_sub(b, n_own, n_dep, dep_len, 0, cancel=2, inherit=True)
        glue = _s_row_first(b, cl, n_dep)   # an own forbidden signal of s's row
        ch = ds.chain(b, ds.P4_MIN, unique=False, glue=glue)
        cl["n"] += ch["n"]
        b.probes(cl["probe"] + ch["probe"])
        return b.system(), cl

    def certify(sys_, cl, old):
        c = _the(ds.cluster_shapes(sys_, old), cl["n"])
        cs = ds.compose_shape(sys_, c, cl["s"], p4=True)
        return [("p4", c["p4"], True), ("ordered", c["order_free"], False), ("in the head", c["rank"] < k.kHeadLimit, True),
                ("signals <= kSpecTabMax", c["takeable"] <= k.kSpecTabMax, True),
                ("length", cs["length"], n_own + n_dep), ("holder entries", cs["holders"], n_dep), ("E", cs["E"], n_own + n_dep * dep_len)] + \
            zero_checks(sys_, cl, old, 2)
    _add(name, build, certify, stats=lambda old: _one_elim(head_launches=1, tail_launches=0, small_launches=0, giant_launches=0))


def _zero_giant_case():
    name, n_own, n_dep, dep_len = "zero_giant", 6, 6, 4

    def build(p):
        b = Builder(_seed(name), p)
        cl = ds.dep_sub(b, n_own, n_dep, dep_len, 0, cancel=2, inherit=True)
        glue = _s_row_first(b, cl, n_dep)
        ch = ds.chain(b, k.kGiantRows, glue=glue)
        cl["n"] += ch["n"]
        b.probes(cl["probe"] + ch["probe"])
        return b.system(), cl

    def certify(sys_, cl, old):
        c = _the(ds.cluster_shapes(sys_, old), cl["n"])
        cs = ds.compose_shape(sys_, c, cl["s"], p4=True)
        return [("rows >= kGiantRows", c["rows"] >= k.kGiantRows, True), ("p4", c["p4"], True), ("ordered", c["order_free"], False),
                ("length", cs["length"], n_own + n_dep), ("holder entries", cs["holders"], n_dep), ("E", cs["E"], n_own + n_dep * dep_len)] + \
            zero_checks(sys_, cl, old, 2)
    _add(name, build, certify, stats=lambda old: _one_elim(giant_launches=1))


def _zero_round2_case():
    """dep_sub's rows entered as non-linear rows whose A is the constant 1: round 1 turns each into the
    linear row C - B, so the cluster, its composition and the zero keys of s and t are round 2's.  (The
    round2_* cases of dispatch_shapes cannot hold a zero key: each of their late stars is a cluster of
    one row, which composes with nothing.)"""
    name, n_own, n_dep, dep_len, pad = "zero_round2", 6, 6, 4, 4

    def build(p):
        b = Builder(_seed(name), p)
        cl = ds.dep_sub(b, n_own, n_dep, dep_len, pad, cancel=2, inherit=True)
        assert b.n_nl == 0 and len(b.rows) == cl["n"]
        for i, row in enumerate(b.rows):
            m = dict(row.c)
            k0 = min(m)
            b.rows[i] = R.Con({0: 1}, {k0: p - m.pop(k0)}, m)
        b.n_lin, b.n_nl = 0, cl["n"]
        b.probes(cl["probe"])
        return b.system(), cl

    def certify(sys_, cl, old):
        r2 = ds.round2_shapes(sys_, old)
        log1 = R.simplification(sys_, R.Flags(no_rounds=1), want_log=True).log
        return [("round-1 substitutions", len(log1), 0), ("round-2 substitutions", r2["n_subs"], cl["n"]),
                ("storage rows round 2 touches", sum(r["touched"] for r in r2["rows"]), len(r2["rows"])),
                ("storage rows", len(r2["rows"]) > 0, True)] + zero_checks(sys_, cl, old, 2)
    _add(name, build, certify, rounds=(None, 2), n_rounds={None: 2, 2: 2})


def _all_cancel_case(cls):
    name, dep_len = f"zero_all_{cls}", 7
    pad = 4 if cls == "lane" else k.kWaveMin

    def build(p):
        b = Builder(_seed(name), p)
        if cls == "tail":
            for f in ds.fillers(b, _filler_sizes(4 + pad, k.kHeadLimit)):
                b.probes(f["probe"], 1)
        cl = ds.zero_sub(b, dep_len, pad)
        b.probes(cl["probe"])
        return b.system(), cl

    def certify(sys_, cl, old):
        c = _the(ds.cluster_shapes(sys_, old), cl["n"])
        cs = ds.compose_shape(sys_, c, cl["s"])
        log = dict(rsio.pyref_log(R.simplification(sys_, R.Flags(use_old_heuristics=old), want_log=True).log))
        return [("in the tail", c["rank"] >= k.kHeadLimit, cls == "tail"), ("workgroup class", c["wg"], cls != "lane"), ("p4", c["p4"], False),
                ("length", cs["length"], 3), ("holder entries", cs["holders"], 2), ("E", cs["E"], 1 + 2 * dep_len),
                ("s is all zeros", log[cl["s"]], {q: 0 for q in [0] + cl["zeros"]}),
                ("t's share of s is all zeros", {q: log[cl["t"]][q] for q in cl["zeros"]}, {q: 0 for q in cl["zeros"]})] + \
            zero_checks(sys_, cl, old, dep_len - 1)
    _add(name, build, certify)


# ---------------------------------------------------------------- cancellation in the non-linear frames
def result_rows(sys_, rounds=None):
    """(rows, quadratic rows, quadratic rows with an empty C) of pyref's result."""
    res = R.simplification(sys_, R.Flags(no_rounds=(1 << 64) - 1 if rounds is None else rounds))
    quad = [c for c in res.constraints if c.a]
    return len(res.constraints), len(quad), sum(1 for c in quad if not c.c)


# what: (A, B, C with T for the twins), result_rows, linear rounds.  A that vanishes or is left a bare
# constant turns the row linear (forbidden signals only): a second linear round runs, as it does on
# the empty row that "gone" leaves in the linear list.
FRAME_KINDS = {"A_vanishes": ((["T"], ["p"], ["p", "p", "c"]), (1, 0, 0), 2),
               "A_constant": ((["c", "T"], ["p", "p"], ["p", "p", "c"]), (1, 0, 0), 2),
               "C_vanishes": ((["p"], ["p"], ["T"]), (1, 1, 1), 1),
               "gone": ((["T"], ["p"], ["T"]), (0, 0, 0), 2)}
FRAME_CASE_NAMES: List[str] = []


def _frame_case(what, wide):
    """One non-linear row of round 1 (k_frames_wave<0>): twins of 3 terms each, or twins sized so that
    the row's terms are exactly kFwT (plain entries of B make up the remainder)."""
    (sa, sb, sc), rows, n_rounds = FRAME_KINDS[what]
    n_tw = (sa + sc).count("T")
    other = len(sa + sb + sc) - n_tw
    if wide:
        # several pairs of twins per vanishing part, each pair a two-row cluster under kHeavyNnz entries
        # (lane class: the row waits for no head cluster)
        L = k.kHeavyNnz // 2 - 4
        more = (k.kFwT - other) // (2 * L) - n_tw
        assert more >= 0
        if "T" in sc:
            sc = sc + ["T"] * (more // n_tw)
            more -= more // n_tw
        sa = sa + ["T"] * more if "T" in sa else sa
        n_tw = (sa + sc).count("T")
        sb = sb + ["p"] * (k.kFwT - other - 2 * n_tw * L)
    else:
        L = 3
    terms, entries = 2 * n_tw * L + len(sa + sb + sc) - n_tw, len(sa + sb + sc) + n_tw
    name = f"frames_{what}_{'kFwT' if wide else 'L3'}"
    FRAME_CASE_NAMES.append(name)

    def build(p):
        b = Builder(_seed(name), p)
        ds.quad(b, *([("twin", L) if e == "T" else e for e in sp] for sp in (sa, sb, sc)))
        return b.system(), None

    def certify(sys_, info, old):
        nl = ds.nonlinear_shapes(sys_, old)
        sh = ds.cluster_shapes(sys_, old)
        got = [("non-linear rows", len(nl), 1), ("no workgroup-class cluster", any(c["wg"] for c in sh), False),
               ("terms", nl[0]["terms"], terms), ("entries", nl[0]["entries"], entries),
               ("result rows, quadratic, quadratic with an empty C", result_rows(sys_), rows)]
        if wide:
            got.append(("terms", terms, k.kFwT))
        if what == "A_constant":
            got.append(("fix pass terms", nl[0]["fix"], len(sc) + len(sb)))
        return got
    _add(name, build, certify, n_rounds={None: n_rounds})


def _round2_frame_case(what):
    """The same under k_frames_wave<1>: late twins in A (and C) of a storage row round 1 leaves alone."""
    name, L = f"round2_{what}", 4
    FRAME_CASE_NAMES.append(name)
    gone = what == "gone"

    def build(p):
        b = Builder(_seed(name), p)
        ds.storage_row(b, 0 if gone else 2, [], twin_a=L, twin_c=L if gone else None)
        return b.system(), None

    def certify(sys_, info, old):
        r1 = ds.nonlinear_shapes(sys_, old)
        r2 = ds.round2_shapes(sys_, old)
        st = [r for r in r2["rows"] if r["touched"]]
        ent = 5 if gone else 5
        return [("round-2 substitutions", r2["n_subs"], 4 if gone else 2), ("storage rows round 2 touches", len(st), 1),
                ("round 1 leaves the row alone", (r1[-1]["terms"], r1[-1]["entries"]), (ent, ent)),
                ("round-2 terms", st[0]["terms"] if st else None, 4 * L + 1 if gone else 2 * L + 3),
                ("result rows at --O2round 2", result_rows(sys_, 2), (0, 0, 0) if gone else (1, 0, 0)),
                ("result rows at --O2", result_rows(sys_), (0, 0, 0) if gone else (1, 0, 0))]
    _add(name, build, certify, rounds=(None, 2), n_rounds={None: 3, 2: 2})


def run_id(run) -> str:
    c, pr, old, rd = run
    return c.name + ("" if pr == "bn128" else "-" + pr) + ("-old" if old else "") + (f"-round{rd}" if rd else "")


for _kind in ("empty", "const", "partial"):
    for _where in ds.PLACEMENTS:
        _cancel_merge_case(_kind, _where)
    _cancel_giant_case(_kind)
_twin_cases()
_zero_p4_case()
_zero_giant_case()
_zero_round2_case()
for _cls in ("lane", "head", "tail"):
    _all_cancel_case(_cls)
for _what in FRAME_KINDS:
    for _wide in (False, True):
        _frame_case(_what, _wide)
for _what in ("A_vanishes", "gone"):
    _round2_frame_case(_what)
assert len({c.name for c in CANCEL_CASES}) == len(CANCEL_CASES)
