"""Inputs of known shape for rounds 3 and later, and the CPU proof of that shape (no GPU needed).

Round 1 is the elimination over the input's linear rows; every later round eliminates over the rows
the round before it turned linear (constraint_simplification.rs:613-646).  Three things only wake up
there, and these cases pin each with hand-built rows in the style of dispatch_shapes.py:

  pos_*     the order of the rows one round turns linear: by the rank of the turning substitution,
            then by the row's first position in the never-pruned map[from] -- whose later part is what
            earlier rounds appended (apply_substitution_to_map, :369-377; csrc/maplists.hpp);
  turn_*    the rank at which a row turns: the first substitution of the round after which its A or B
            is constant or empty (d_round_turn, k_round_turn, the pre-expanded path of k_round_fill);
  empty_* / stale_*
            rows that come out empty, and visits of rows an earlier round already emptied: they
            decide how many rounds the reference's loop makes.

Every signal that is never eliminated is forbidden and every signal meant to be taken is the largest
takeable id of its linear row (take_signal_3), so pyref's log holds exactly the intended substitutions
round by round.  The gadgets:

  kick(x, E)      a non-linear row whose A is one constant term: round 1 turns it linear and round 2
                  substitutes x := E;
  driver          a storage row whose A vanishes under a substitution of round k and whose C is then
                  the linear row that round k + 1 eliminates;
  target          a storage row whose A or B becomes constant or empty in a chosen round; its C is
                  w + c f with w takeable and f forbidden and fresh, so every target is a cluster of
                  its own in the next round and the log shows the order of the list.

record() runs pyref.simplification with apply_substitution_to_map wrapped: it keeps pyref's own map
before every call and walks it, so a certificate reads the round, the rank and the list position of a
row from the reference's lists.  MODELS are wrong ways to order the turned rows; tests/test_round_cases.py
proves which case changes under which, and tests/test_gpu_rounds.py runs the cases on the GPU."""
from __future__ import annotations

from typing import Callable, Dict, List, Optional

import dispatch_shapes as ds
import rsio

R = rsio.R
k = ds.k
U64 = (1 << 64) - 1


# ============================================================================ gadgets
class RB:
    """A dispatch_shapes.Builder with named signals and named storage rows (ids in storage order: the
    non-linear rows that round 1 leaves non-linear)."""

    def __init__(self, name: str, p: int):
        self.b = ds.Builder(ds._seed(name), p)
        self.p = p
        self.rows: Dict[str, int] = {}
        self.sig: Dict[str, int] = {}
        self.n_st = 0

    def F(self) -> int:
        return self.b.forbid(1)[0]

    def T(self, *names) -> List[int]:
        """Fresh takeable signals, ascending in the order named."""
        ids = self.b.take(len(names))
        self.sig.update(zip(names, ids))
        return ids

    def c(self) -> int:
        return self.b.coef()

    def scale(self, m: dict, kk: int) -> dict:
        return {s: v * kk % self.p for s, v in m.items()}

    def add(self, *ms) -> dict:
        out: dict = {}
        for m in ms:
            for s, v in m.items():
                out[s] = (out.get(s, 0) + v) % self.p
        assert all(out.values()), "an input row holds no zero coefficient"
        return out

    def minus(self, x: int, E: dict, only=None) -> dict:
        """a (x - E), or a (x - the part of E over `only`): under x := E it becomes empty, or a times
        the rest of E."""
        part = E if only is None else {s: E[s] for s in only}
        return self.scale(self.add({x: 1}, self.scale(part, self.p - 1)), self.c())

    def kick(self, x: int, E: dict) -> None:
        """Round 1 turns {0: s} * {x: t} = s t E into s t (E - x) = 0; round 2 substitutes x := E."""
        s, t = self.c(), self.c()
        self.b.nonlin({0: s}, {x: t}, self.scale(E, s * t % self.p))

    def store(self, name: str, a: dict, c: dict, b: Optional[dict] = None) -> int:
        self.rows[name] = self.n_st
        self.n_st += 1
        self.b.nonlin(a, b if b is not None else {self.F(): self.c()}, c)
        return self.rows[name]

    def tail(self, name: str) -> dict:
        """The C of a target: w + c f.  Once the row is linear it is a cluster of its own whose only
        takeable signal is w."""
        w, = self.T("w:" + name)
        return {w: self.c(), self.F(): self.c()}

    def target(self, name: str, a: dict, b: Optional[dict] = None) -> int:
        return self.store(name, a, self.tail(name), b)

    def holder(self, name: str, x: int) -> int:
        """A storage row that holds x in C only: it is in map[x] and never turns."""
        return self.store(name, {self.F(): self.c()}, {x: self.c(), self.F(): self.c()})

    def done(self):
        return self.b.system(), dict(rows=dict(self.rows), sig=dict(self.sig))


# ============================================================================ the record of a run
def _walk(storage, m, subs, p, stale):
    """apply_substitution_to_map (:345-396) on copies, one event per visit: the rank q of the
    substitution, the position in map[from] as it stands, the row, whether the row is linear after
    the visit, and whether it was already empty when the round began."""
    st = [c.clone() for c in storage]
    mm = {s: list(v) for s, v in m.items()}
    events, lists = [], {}
    for q, sub in enumerate(subs):
        if sub.frm in mm:
            ids = list(mm[sub.frm])
            lists[q] = ids
            keys = sorted(sub.to)
            for pos, cid in enumerate(ids):
                con = st[cid].clone()
                R.apply_substitution(con, sub, p)
                R.fix_constraint(con, p)
                events.append(dict(q=q, pos=pos, cid=cid, linear=R.is_linear(con), stale=stale[cid]))
                st[cid] = con
                for s in keys:
                    mm.setdefault(s, []).append(cid)
    return events, lists


def _first(lst, x):
    return lst.index(x)


def _model_key(model: str, call: dict, hist: List[dict], minit: dict):
    """The sort key a model gives a turned row.  "engine" is run.hpp's: the rank of the turning
    substitution, then the first position in map[from]; each other one is wrong in one way."""
    froms, lists, turn, applicable = call["froms"], call["lists"], call["turn"], call["applicable"]

    def initial_then_id(q, cid, lst):
        return (q, 0, _first(lst, cid)) if cid in lst else (q, 1, cid)

    def key(cid):
        q = turn[cid]
        if model == "engine":
            return (q, _first(lists[q], cid))
        if model == "by_id":                 # ascending id per substitution
            return (q, cid)
        if model == "no_appended":           # the appended part ignored: such rows last, by id
            return initial_then_id(q, cid, minit.get(froms[q], []))
        if model == "last_occurrence":
            return (q, len(lists[q]) - 1 - _first(lists[q][::-1], cid))
        if model == "one_level":             # appends one level deep: minit[from_j] without list(from_j, b)
            lst = list(minit.get(froms[q], []))
            for h in hist:
                for f, keys in h["subs"]:
                    if froms[q] in keys:
                        lst += minit.get(f, [])
            return initial_then_id(q, cid, lst)
        if model in ("min_rank", "max_rank"):
            q2 = (min if model == "min_rank" else max)(applicable[cid])
            return (q2, _first(lists[q2], cid))
        if model == "pos_first":             # position before rank
            return (_first(lists[q], cid), q)
        if model == "rank_by_from":          # the round's substitutions in ascending `from`, not cluster first
            return (sorted(froms).index(froms[q]), _first(lists[q], cid))
        raise KeyError(model)
    return key


MODELS = ("by_id", "no_appended", "last_occurrence", "one_level", "min_rank", "max_rank", "pos_first", "rank_by_from")


def record(sys_: "R.System", rounds=None, old: bool = False, model: str = "engine") -> dict:
    """One pyref.simplification with its log, apply_substitution_to_map wrapped.  Per call (call i is
    round i + 2): pyref's map before it, the substitutions, the visits (_walk), the rows that turn
    (first linear visit of a row that was not empty when the round began) in the reference's order, and
    whether every linear visit was of a row emptied earlier.  The list handed back to pyref is the
    reference's own, with the turned rows reordered by `model` ("engine" must leave it as it is:
    asserted).  seq is the sequence of linear_simplification ("L") and apply ("A") calls and logs the
    `from` signals each linear_simplification logged."""
    calls: List[dict] = []
    seq: List[str] = []
    logs: List[List[int]] = []
    minit: dict = {}
    real_apply, real_lin = R.apply_substitution_to_map, R.linear_simplification

    def lin(log, linear, *a, **kw):
        seq.append("L")
        n0 = len(log)
        out = real_lin(log, linear, *a, **kw)
        logs.append([s.frm for s in log[n0:]])
        return out

    def apply(storage, m, subs, p):
        seq.append("A")
        if not calls:
            minit.update({s: list(v) for s, v in m.items()})
        stale = [R.is_empty(c) for c in storage]
        before = {s: list(v) for s, v in m.items()}
        rows0 = [c.clone() for c in storage]
        events, lists = _walk(storage, m, subs, p, stale)
        linear = real_apply(storage, m, subs, p)
        lin_ev = [e for e in events if e["linear"]]
        assert len(lin_ev) == len(linear), "the walk differs from apply_substitution_to_map"
        turn, content, order = {}, {}, []
        for e, con in zip(lin_ev, linear):
            if not e["stale"] and e["cid"] not in turn:
                turn[e["cid"]] = e["q"]
                content[e["cid"]] = con
                order.append(e["cid"])
        froms = [s.frm for s in subs]
        applicable = {cid: sorted(q for q, s in enumerate(subs) if q in lists and
                                  any(s.frm in part for part in (rows0[cid].a, rows0[cid].b, rows0[cid].c))) for cid in turn}
        call = dict(round=len(calls) + 2, before=before, subs=[(s.frm, sorted(s.to)) for s in subs], froms=froms, lists=lists,
                    events=events, turn=turn, applicable=applicable, order=order, n_linear=len(linear),
                    all_stale=bool(lin_ev) and all(e["stale"] for e in lin_ev),
                    pos={cid: _first(lists[q], cid) for cid, q in turn.items()})
        by_engine = sorted(order, key=_model_key("engine", call, calls, minit))
        assert by_engine == order, "(rank, first position) is not the reference's order"
        if model != "engine":
            new = sorted(order, key=_model_key(model, call, calls, minit))
            linear = [content[cid] for cid in new] + [R.con_empty()] * (len(linear) - len(new))
            call["model_order"] = new
        calls.append(call)
        return linear

    R.apply_substitution_to_map, R.linear_simplification = apply, lin
    try:
        res = R.simplification(sys_, R.Flags(no_rounds=U64 if rounds is None else rounds, use_old_heuristics=old), want_log=True)
    finally:
        R.apply_substitution_to_map, R.linear_simplification = real_apply, real_lin
    return dict(res=res, log=rsio.pyref_log(res.log), calls=calls, seq=seq, minit=minit, logs=logs)


def outcome(rec: dict):
    """What a GPU run is compared on: the constraints, the signal map and the log."""
    res = rec["res"]
    return ([(c.a, c.b, c.c) for c in res.constraints], res.signal_map, res.no_private_inputs_witness, rec["log"])


def pyref_rounds(rec: dict) -> int:
    return rec["seq"].count("L")


def rounds_model(sys_: "R.System", rounds=None, old: bool = False, rec: Optional[dict] = None) -> int:
    """rs_stats.rounds: pyref's calls of linear_simplification, less the trailing iterations whose
    whole list is stale visits -- visits, through the never-pruned map, of rows that an EARLIER round
    turned linear and emptied (is_linear(empty) holds, so the reference lists them again and loops once
    more over nothing).  A row that turns in the round itself and comes out empty is no stale visit."""
    rec = rec or record(sys_, rounds, old)
    n, seq, at = 0, rec["seq"], -1
    for i, what in enumerate(seq):
        if what == "A":
            at += 1
        elif not (at >= 0 and seq[i - 1] == "A" and rec["calls"][at]["all_stale"]):
            n += 1
    return n


def log_by_round(rec: dict) -> List[List[int]]:
    """The `from` signals pyref logs in round 1, 2, ..."""
    return rec["logs"]


def maplists_input(rec: dict) -> str:
    """The text tests/maplists_check.cpp reads in its file mode: the initial lists, then per round the
    queries (the signals the round substitutes, resolved before its batch is added) and its batch (`from`
    and right-hand-side keys of every substitution, in rank order)."""
    out = [f"{len(rec['minit'])}"]
    for s in sorted(rec["minit"]):
        out.append(" ".join(map(str, [s, len(rec["minit"][s])] + rec["minit"][s])))
    out.append(str(len(rec["calls"])))
    for c in rec["calls"]:
        out.append(" ".join(map(str, [len(c["froms"])] + c["froms"])))
        out.append(str(len(c["subs"])))
        for f, keys in c["subs"]:
            out.append(" ".join(map(str, [f, len(keys)] + keys)))
    return "\n".join(out) + "\n"


def maplists_expected(rec: dict) -> List[str]:
    """The lines the file mode prints: `round signal length rows...`, the part of pyref's map[signal]
    beyond the initial list, for every signal a round substitutes (empty lists are not printed)."""
    out = []
    for i, c in enumerate(rec["calls"]):
        for f in c["froms"]:
            ext = c["before"].get(f, [])[len(rec["minit"].get(f, [])):]
            if ext:
                out.append(" ".join(map(str, [i, f, len(ext)] + ext)))
    return out


# ============================================================================ the cases
class Case(ds.Case):
    """A dispatch_shapes.Case plus: turn_round -- the round in which the rows under test turn (also
    the N of the --O2round N variant); order -- the names of ALL rows that turn in it, in the
    reference's order; log -- the signal names pyref substitutes in round 2, 3, ... up to turn_round;
    models -- the wrong models the case is named for; facts(view) -> more [(what, got, want)]."""

    def __init__(self, name, build, turn_round, order, log, models=(), facts: Optional[Callable] = None,
                 primes=("bn128",), py_rounds=None):
        rounds = (None, turn_round) if name.startswith(("pos_", "turn_")) else (None,)
        super().__init__(name, build, None, primes=primes, olds=(False, True), rounds=rounds)
        self.turn_round, self.order, self.log, self.models, self.facts = turn_round, tuple(order), log, tuple(models), facts
        self.py_rounds = py_rounds      # (pyref's linear rounds, rounds_model) under --O2
        self.certify = self._certify

    def _certify(self, sys_, info, old):
        rec = record(sys_, None, old)
        rows, sig = info["rows"], info["sig"]
        name_of = {v: n for n, v in rows.items()}
        calls = rec["calls"]
        at = calls[self.turn_round - 2]
        got = [("rows turned in the round, in order", [name_of.get(c, c) for c in at["order"]], list(self.order))]
        sig_of = {v: n for n, v in sig.items()}
        lg = log_by_round(rec)
        got.append(("round 1 substitutes nothing", lg[0], []))
        for r, want in enumerate(self.log, start=2):
            got.append((f"round {r} substitutes", [sig_of.get(s, s) for s in lg[r - 1]], list(want)))
        if self.py_rounds is not None:
            got.append(("(pyref's rounds, rounds_model)", (pyref_rounds(rec), rounds_model(sys_, rec=rec)), self.py_rounds))
        if self.facts is not None:
            got += self.facts(View(rec, info, self))
        return got


class View:
    """What a case's facts read: per named row its (round, rank, first position) of turning, pyref's
    map before a round, and the initial lists."""

    def __init__(self, rec, info, case):
        self.rec, self.rows, self.sig, self.case = rec, info["rows"], info["sig"], case
        self.name_of = {v: n for n, v in self.rows.items()}

    def turn(self, name):
        cid = self.rows[name]
        for c in self.rec["calls"]:
            if cid in c["turn"]:
                return (c["round"], c["turn"][cid], c["pos"][cid])
        return None

    def lst(self, rnd, signame):
        """pyref's map[signal] before round `rnd`, as row names."""
        return [self.name_of.get(c, c) for c in self.rec["calls"][rnd - 2]["before"].get(self.sig[signame], [])]

    def init(self, signame):
        return [self.name_of.get(c, c) for c in self.rec["minit"].get(self.sig[signame], [])]

    def rank_from(self, rnd):
        sig_of = {v: n for n, v in self.sig.items()}
        return [sig_of.get(f, f) for f in self.rec["calls"][rnd - 2]["froms"]]


CASES: List[Case] = []
_BUILT: dict = {}


def built(case: Case, prime: str = "bn128"):
    key = (case.name, prime)
    if key not in _BUILT:
        _BUILT[key] = case.build(R.PRIMES[prime])
    return _BUILT[key]


def _add(*a, **kw):
    CASES.append(Case(*a, **kw))


def _ws(*names):
    return ["w:" + n for n in names]


# ---------------------------------------------------------------- position in map[from]
def _pos_initial_r2(p):
    g = RB("pos_initial_r2", p)
    xb, xa = g.T("xb", "xa")                  # xa's cluster comes first although xb < xa
    Ea, Eb = {g.F(): g.c(), 0: g.c()}, {g.F(): g.c()}
    g.kick(xa, Ea)
    g.kick(xb, Eb)
    for nm, x, E in (("T0", xb, Eb), ("T1", xa, Ea), ("T2", xb, Eb), ("T3", xa, Ea)):
        g.target(nm, g.minus(x, E))
    return g.done()


_add("pos_initial_r2", _pos_initial_r2, 2, ["T1", "T3", "T0", "T2"], [["xa", "xb"]], models=("pos_first",), py_rounds=(4, 3),
     facts=lambda v: [("every turned row is in the initial list", [v.init("xa"), v.init("xb")], [["T1", "T3"], ["T0", "T2"]]),
                      ("(round, rank, position)", [v.turn(n) for n in ("T0", "T1", "T2", "T3")], [(2, 1, 0), (2, 0, 0), (2, 1, 1), (2, 0, 1)])])


def _five_rows(name, driver_only=False):
    def build(p):
        g = RB(name, p)
        y, x1, x2 = g.T("y", "x1", "x2")
        f3, f4 = g.F(), g.F()          # (every row has a B of its own: a shared one would join the turned rows into one cluster)
        E1, E2 = {y: g.c(), f3: g.c()}, {y: g.c(), f4: g.c()}
        g.kick(x1, E1)
        if not driver_only:
            g.kick(x2, E2)
            g.target("T0", g.minus(x2, E2, only=[f4]))
        g.store("D", g.minus(x1, E1), {y: 1, 0: p - 7})
        if not driver_only:
            g.target("T2", g.minus(x1, E1, only=[f3]))
        return g.done()
    return build


def _five_facts(v):
    return [("map[y] before round 3", v.lst(3, "y"), ["D", "D", "T2", "T0"]), ("its initial part", v.init("y"), ["D"]),
            ("(round, rank, position)", [v.turn(n) for n in ("D", "T2", "T0")], [(2, 0, 0), (3, 0, 2), (3, 0, 3)]),
            ("stale visits ahead of the rows that turn in round 3", [(e["cid"] == v.rows["D"], e["stale"]) for e in v.rec["calls"][1]["events"][:2]],
             [(True, True)] * 2),
            ("all stale, per list (the last call has no substitution)", [c["all_stale"] for c in v.rec["calls"]], [False, False, True, False])]


_add("pos_appended_r3", _five_rows("pos_appended_r3"), 3, ["T2", "T0"], [["x1", "x2"], ["y"]], models=("by_id", "no_appended"),
     py_rounds=(5, 4), facts=_five_facts)


def _depth(d):
    name = f"pos_appended_depth{d}"

    def build(p):
        g = RB(name, p)
        z = g.T(*[f"z{i}" for i in range(d, 0, -1)])[::-1]      # z[0] = z1 > z2 > ... > zd
        xa, xb = g.T("xa", "xb")
        fa, fb = g.F(), g.F()
        Ea, Eb = {z[0]: g.c(), fa: g.c()}, {z[0]: g.c(), fb: g.c()}
        g.kick(xa, Ea)
        g.kick(xb, Eb)
        g.target("Tlo", g.minus(xb, Eb, only=[fb]))
        prev = (xa, Ea)
        for i in range(d):                                  # D{i+1} turns in round i + 2 and gives z{i+1}'s substitution
            nxt = {z[i + 1]: g.c()} if i + 1 < d else {0: g.c()}
            g.store(f"D{i + 1}", g.minus(*prev), g.minus(z[i], nxt))
            prev = (z[i], nxt)
        g.target("Thi", g.minus(xa, Ea, only=[fa]))
        return g.done()

    def facts(v):
        last = f"z{d}"
        return [("neither row is in an initial list past x", [n for n in ("Tlo", "Thi") for i in range(1, d + 1) if n in v.init(f"z{i}")], []),
                ("the two reach the last list by different routes", (v.init("xa")[-1], v.init("xb")), ("Thi", ["Tlo"])),
                ("order in map[z_d] before the round", [n for n in v.lst(d + 2, last) if n in ("Tlo", "Thi")][:2], ["Thi", "Tlo"]),
                ("(round, rank)", [v.turn(n)[:2] for n in ("Thi", "Tlo")], [(d + 2, 0)] * 2),
                ("positions ascend against the ids", v.turn("Thi")[2] < v.turn("Tlo")[2] and v.rows["Thi"] > v.rows["Tlo"], True),
                ("batches before the round", len(v.rec["calls"][:d]), d)]
    _add(name, build, d + 2, ["Thi", "Tlo"], [["xa", "xb"]] + [[f"z{i}"] for i in range(1, d + 1)], models=("by_id", "no_appended", "one_level"),
         py_rounds=(d + 4, d + 3), facts=facts)


for _d in (2, 3, 5):
    _depth(_d)


def _pos_both(p):
    g = RB("pos_both", p)
    y, x1, x2 = g.T("y", "x1", "x2")
    f3, f4 = g.F(), g.F()
    E1, E2 = {y: g.c(), f3: g.c()}, {y: g.c(), f4: g.c()}
    g.kick(x1, E1)
    g.kick(x2, E2)
    g.target("Ra", g.minus(x1, E1, only=[f3]))
    g.store("D", g.minus(x1, E1), {y: 1, 0: p - 7})
    g.target("Rb", g.add(g.minus(x2, E2, only=[f4]), {y: 3}))
    return g.done()


_add("pos_both", _pos_both, 3, ["Rb", "Ra"], [["x1", "x2"], ["y"]], models=("last_occurrence", "by_id"), py_rounds=(5, 4),
     facts=lambda v: [("map[y] before round 3", v.lst(3, "y"), ["D", "Rb", "Ra", "D", "Rb"]), ("its initial part", v.init("y"), ["D", "Rb"]),
                      ("(round, rank, position)", [v.turn(n) for n in ("Rb", "Ra")], [(3, 0, 1), (3, 0, 2)])])


def _pos_duplicate(p):
    g = RB("pos_duplicate", p)
    y, x1, x2 = g.T("y", "x1", "x2")
    f3, f4 = g.F(), g.F()
    E1, E2 = {y: 1, f3: g.c()}, {y: 1, f4: g.c()}
    g.kick(x1, E1)
    g.kick(x2, E2)
    g.target("R2", g.minus(x2, E2, only=[f4]))
    g.store("D", g.minus(x1, E1), {y: 1, 0: p - 7})
    g.target("R1", g.add({x1: 2, f3: (p - 2) * E1[f3] % p}, {x2: 3, f4: (p - 3) * E2[f4] % p}))     # 2 y + 3 y after round 2
    return g.done()


_add("pos_duplicate", _pos_duplicate, 3, ["R1", "R2"], [["x1", "x2"], ["y"]], models=("last_occurrence", "by_id"), py_rounds=(5, 4),
     facts=lambda v: [("map[y] before round 3", v.lst(3, "y"), ["D", "D", "R1", "R2", "R1"]), ("its initial part", v.init("y"), ["D"]),
                      ("(round, rank, position)", [v.turn(n) for n in ("R1", "R2")], [(3, 0, 2), (3, 0, 3)])])


def _pos_cluster_vs_from(p):
    g = RB("pos_cluster_vs_from", p)
    ylo, yhi, xlo, xhi = g.T("ylo", "yhi", "xlo", "xhi")
    fl, fh = g.F(), g.F()
    Eh, El = {yhi: g.c(), fh: g.c()}, {ylo: g.c(), fl: g.c()}
    g.kick(xhi, Eh)                                  # the first cluster holds the larger `from`
    g.kick(xlo, El)
    g.target("T0", g.minus(xlo, El, only=[fl]))
    g.store("Dlo", g.minus(xlo, El), {ylo: 1, 0: p - 5})
    g.store("Dhi", g.minus(xhi, Eh), {yhi: 1, 0: p - 7})
    g.target("T1", g.minus(xhi, Eh, only=[fh]))
    return g.done()


_add("pos_cluster_vs_from", _pos_cluster_vs_from, 3, ["T1", "T0"], [["xhi", "xlo"], ["yhi", "ylo"]], models=("rank_by_from", "pos_first"),
     py_rounds=(5, 4),
     facts=lambda v: [("ranks of rounds 2 and 3 descend by `from`", [v.rank_from(2), v.rank_from(3)], [["xhi", "xlo"], ["yhi", "ylo"]]),
                      ("round 2 turns the drivers by rank, against their ids", [v.turn("Dhi"), v.turn("Dlo")], [(2, 0, 0), (2, 1, 1)]),
                      ("(round, rank, position)", [v.turn("T1"), v.turn("T0")], [(3, 0, 2), (3, 1, 1)])])


# ---------------------------------------------------------------- turn rank
def _turn_second(p):
    g = RB("turn_second", p)
    xlo, xhi = g.T("xlo", "xhi")
    Eh, El = {g.F(): g.c(), 0: g.c()}, {g.F(): g.c(), g.F(): g.c()}
    g.kick(xhi, Eh)                                  # rank 0 is the larger id
    g.kick(xlo, El)
    g.target("R", g.add(g.minus(xhi, Eh), g.minus(xlo, El)))
    g.target("Q", g.minus(xhi, Eh))
    return g.done()


_add("turn_second", _turn_second, 2, ["Q", "R"], [["xhi", "xlo"]], models=("min_rank", "pos_first"), primes=("bn128", "goldilocks"), py_rounds=(4, 3),
     facts=lambda v: [("(round, rank, position)", [v.turn("Q"), v.turn("R")], [(2, 0, 1), (2, 1, 0)]),
                      ("R holds both substituted signals", v.rec["calls"][0]["applicable"][v.rows["R"]], [0, 1])])


def _turn_cancel(p):
    g = RB("turn_cancel", p)
    x, z = g.T("x", "z")
    E = {g.F(): g.c(), g.F(): g.c(), 0: g.c()}
    g.kick(x, E)
    g.kick(z, g.scale(E, p - 1))
    a = g.c()
    g.target("R", {x: a, z: a})                      # a (x + z): E - E only after both
    g.target("Q", g.minus(x, E))
    return g.done()


_add("turn_cancel", _turn_cancel, 2, ["Q", "R"], [["x", "z"]], models=("min_rank", "pos_first"), primes=("bn128", "goldilocks"), py_rounds=(4, 3),
     facts=lambda v: [("(round, rank, position)", [v.turn("Q"), v.turn("R")], [(2, 0, 1), (2, 1, 0)]),
                      ("R's A is x + z alone", sorted(built(v.case)[0].rows[2].a) == sorted([v.sig["x"], v.sig["z"]]), True)])


def _turn_b_first(p):
    g = RB("turn_b_first", p)
    x1, x2 = g.T("x1", "x2")
    E2 = {g.F(): g.c(), 0: g.c()}
    g.kick(x1, {0: g.c()})                           # rank 0: B = b x1 becomes constant
    g.kick(x2, E2)
    g.target("Q", g.minus(x2, E2))
    g.target("R", g.minus(x2, E2), {x1: g.c()})      # A would vanish at rank 1
    return g.done()


_add("turn_b_first", _turn_b_first, 2, ["R", "Q"], [["x1", "x2"]], models=("max_rank",), primes=("bn128", "goldilocks"), py_rounds=(4, 3),
     facts=lambda v: [("(round, rank, position)", [v.turn("R"), v.turn("Q")], [(2, 0, 0), (2, 1, 0)]),
                      ("R holds both substituted signals", v.rec["calls"][0]["applicable"][v.rows["R"]], [0, 1])])


def _turn_dup_signal(p):
    g = RB("turn_dup_signal", p)
    x, x2 = g.T("x", "x2")
    val = g.c()
    E2 = {g.F(): g.c()}
    g.kick(x, {0: val})
    g.kick(x2, E2)
    g.holder("H", x)
    a = g.c()
    g.target("R", {x: a, 0: (p - a) * val % p}, {x: g.c()})     # x in A and in B: A vanishes and B is constant at once
    g.target("Q", g.minus(x2, E2))
    return g.done()


_add("turn_dup_signal", _turn_dup_signal, 2, ["R", "Q"], [["x", "x2"]], models=("pos_first",), primes=("bn128", "goldilocks"), py_rounds=(4, 3),
     facts=lambda v: [("(round, rank, position)", [v.turn("R"), v.turn("Q"), v.turn("H")], [(2, 0, 1), (2, 1, 0), None]),
                      ("x is in A and in B", [v.sig["x"] in m for m in (built(v.case)[0].rows[3].a, built(v.case)[0].rows[3].b)], [True, True])])


def _turn_c_only(p):
    g = RB("turn_c_only", p)
    x0, x1 = g.T("x0", "x1")
    E0, E1 = {g.F(): g.c(), 0: g.c()}, {g.F(): g.c()}
    g.kick(x0, E0)
    g.kick(x1, E1)
    c = g.tail("R")
    c[x0] = g.c()
    g.store("R", g.minus(x1, E1), c)                 # x0 (rank 0) in C only, x1 (rank 1) turns it
    g.target("Q", g.minus(x0, E0))
    g.holder("N", x0)                                # substituted in C only: stays non-linear
    return g.done()


_add("turn_c_only", _turn_c_only, 2, ["Q", "R"], [["x0", "x1"]], models=("min_rank", "pos_first"), primes=("bn128", "goldilocks"), py_rounds=(4, 3),
     facts=lambda v: [("(round, rank, position)", [v.turn("Q"), v.turn("R"), v.turn("N")], [(2, 0, 1), (2, 1, 0), None]),
                      ("R's position is from map[x1], not map[x0]", (v.init("x1"), v.init("x0")), (["R"], ["R", "Q", "N"])),
                      ("N is visited and stays", any(e["cid"] == v.rows["N"] and not e["linear"] for e in v.rec["calls"][0]["events"]), True)])


def _turn_rank_over_pos(p):
    g = RB("turn_rank_over_pos", p)
    x0, x1 = g.T("x0", "x1")
    E0, E1 = {g.F(): g.c(), 0: g.c()}, {g.F(): g.c()}
    g.kick(x0, E0)
    g.kick(x1, E1)
    for i in range(5):
        g.holder(f"H{i}", x0)
    g.target("r0", g.minus(x0, E0))
    g.target("r1", g.minus(x1, E1))
    return g.done()


_add("turn_rank_over_pos", _turn_rank_over_pos, 2, ["r0", "r1"], [["x0", "x1"]], models=("pos_first",), primes=("bn128", "goldilocks"), py_rounds=(4, 3),
     facts=lambda v: [("(round, rank, position)", [v.turn("r0"), v.turn("r1")], [(2, 0, 5), (2, 1, 0)])])


def _turn_limit(name, n_plain, late_lengths, want):
    """The round2_terms / round2_entries row of dispatch_shapes, but its A is a signal that round 2 makes
    constant: the row (L) turns, at rank 0 and position 1 behind a holder; a short row S with a smaller id
    turns at rank 1, position 0."""
    def build(p):
        g = RB(name, p)
        xb, xa = g.T("xb", "xa")
        g.kick(xa, {0: g.c()})                       # the first cluster of round 2: rank 0
        g.kick(xb, {0: g.c()})
        g.store("S", {xb: g.c()}, {g.F(): g.c(), g.F(): g.c()})
        g.holder("H", xa)
        c = {g.F(): g.c() for _ in range(n_plain)}
        for ln in late_lengths:
            c[ds.late_star(g.b, ln)] = g.c()
        g.store("L", {xa: g.c()}, c)
        return g.done()

    def facts(v):
        sys_ = built(v.case)[0]
        r2 = ds.round2_shapes(sys_)
        return [("(round, rank, position)", [v.turn("L"), v.turn("S"), v.turn("H")], [(2, 0, 1), (2, 1, 0), None]),
                ("storage rows", len(r2["rows"]), 3)] + [(f"L's round-2 {key}", r2["rows"][2][key], w) for key, w in want.items()]
    _add(name, build, 2, ["L", "S"], [], models=("pos_first",), primes=("bn128", "goldilocks"), py_rounds=(3, 3), facts=facts)


for _dd in (-1, 0, 1):
    _turn_limit(f"turn_limit_terms{_dd:+d}", 0, ds._split(k.kFwT + _dd - 2, 7), dict(terms=k.kFwT + _dd, entries=9, touched=True))
for _dd in (0, 1):
    _turn_limit(f"turn_limit_entries{_dd:+d}", k.kFwE + _dd - 3, [5], dict(entries=k.kFwE + _dd, terms=k.kFwE + _dd + 4, touched=True))


# ---------------------------------------------------------------- emptied rows and the round count
def _empty_same_round(p):
    g = RB("empty_same_round", p)
    y, x1 = g.T("y", "x1")
    E1 = {y: g.c(), g.F(): g.c()}
    val = {0: g.c()}
    g.kick(x1, E1)
    g.store("D", g.minus(x1, E1), g.minus(y, val))
    g.store("E", g.minus(y, val), g.minus(y, val))   # round 3: A and C both cancel
    return g.done()


_add("empty_same_round", _empty_same_round, 3, ["E"], [["x1"], ["y"]], py_rounds=(4, 4),
     facts=lambda v: [("(round, rank, position)", v.turn("E"), (3, 0, 1)),
                      ("the list after round 3 holds only empty rows, one of them turned in it",
                       (v.rec["calls"][1]["n_linear"], v.rec["calls"][1]["all_stale"]), (3, False))])
_add("stale_only", _five_rows("stale_only", driver_only=True), 2, ["D"], [["x1"], ["y"]], py_rounds=(4, 3),
     facts=lambda v: [("round 3 visits the emptied driver alone", [(e["cid"], e["stale"], e["linear"]) for e in v.rec["calls"][1]["events"]],
                       [(0, True, True)] * 2)])
_add("stale_mixed", _five_rows("stale_mixed"), 3, ["T2", "T0"], [["x1", "x2"], ["y"], _ws("T2", "T0")], models=("by_id", "no_appended"),
     py_rounds=(5, 4), facts=_five_facts)

assert len({c.name for c in CASES}) == len(CASES)
BY = {c.name: c for c in CASES}


def variants(case: Case):
    """(prime name, old heuristics, rounds) for every GPU run of a case."""
    return ds.variants(case)


# which wrong model changes which case (its constraints, signal map or log; under --O2 and under
# --O2round N alike), in the order of MODELS; tests/test_round_cases.py proves the table exact
CATCHES: Dict[str, tuple] = {
    "pos_initial_r2": ("pos_first", "rank_by_from"),
    "pos_appended_r3": ("by_id", "no_appended"),
    "pos_appended_depth2": ("by_id", "no_appended", "one_level"),
    "pos_appended_depth3": ("by_id", "no_appended", "one_level"),
    "pos_appended_depth5": ("by_id", "no_appended", "one_level"),
    "pos_both": ("by_id", "last_occurrence"),
    "pos_duplicate": ("by_id", "no_appended", "last_occurrence"),
    "pos_cluster_vs_from": ("pos_first", "rank_by_from"),
    "turn_second": ("min_rank", "pos_first", "rank_by_from"),
    "turn_cancel": ("min_rank", "pos_first"),
    "turn_b_first": ("max_rank",),
    "turn_dup_signal": ("pos_first",),
    "turn_c_only": ("min_rank", "pos_first"),
    "turn_rank_over_pos": ("pos_first",),
    "turn_limit_terms-1": ("max_rank", "pos_first", "rank_by_from"),
    "turn_limit_terms+0": ("max_rank", "pos_first", "rank_by_from"),
    "turn_limit_terms+1": ("max_rank", "pos_first", "rank_by_from"),
    "turn_limit_entries+0": ("max_rank", "pos_first", "rank_by_from"),
    "turn_limit_entries+1": ("max_rank", "pos_first", "rank_by_from"),
    "empty_same_round": (),
    "stale_only": (),
    "stale_mixed": ("by_id", "no_appended"),
}
