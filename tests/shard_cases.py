"""The sharded elimination's deal and exchange filter as a CPU model, and inputs for the deal's remainders.

With the elimination sharded over W ranks (engine.hip, "sharded elimination") every rank eliminates
the kHeadLimit largest workgroup-class clusters itself (replicated: owner W) and a snake share of the
rest of the workgroup list and of the lane-class list; the substitutions of the dealt clusters reach
the other ranks through the packed exchange, a right-hand side only when its `from` is needed (round
1: the relevant set; rounds >= 2: the keys of the non-linear signal map; with the log on: always).
None of it needs a GPU to be stated:

  owner_of        each cluster's owner from dispatch_shapes.cluster_shapes (the deal);
  exchange_model  the substitutions round 1 exchanges, their right-hand-side lengths as the pool
                  stores them, the relevant set, and the two lists the filter splits them into;
  round2_model    the same for round 2 (the rows round 1 turned linear; the storage rows' signals);
  deal_cases      inputs with t dealt workgroup clusters and s dealt lane clusters at every remainder
                  of the snake's period;
  SHARD_DISPATCH / SHARD_CANCEL / SHARD_EXTRA  the certified cases the sharded GPU tests run.

tests/test_shard_cases.py proves the model and the cases on the CPU, tests/test_gpu_shard_cases.py
runs them on in-process groups."""
from __future__ import annotations

from typing import Dict, List, Optional

import cancel_cases as cc
import dispatch_shapes as ds
import rsio
from dispatch_shapes import Builder, Case, _filler_sizes, _seed, k

R = rsio.R
DISPATCH_WORLD, CANCEL_WORLD = 3, 2
DEAL_WORLDS = (2, 3, 4)
ENTRY_BYTES = 36     # what shard_exchange counts per exchanged entry: a 4-byte key and a 32-byte value

SHARD_DISPATCH: List[Case] = ds.CASES
SHARD_CANCEL: List[Case] = cc.CANCEL_CASES


# ============================================================================ the deal
def snake(pos: int, world: int) -> int:
    """The rank position `pos` of a size-ordered list goes to: the ranks are walked 0, 1, .., W - 1,
    then back W - 1, .., 0, and so on (the comment above snake_rank) -- forwards on the even laps over
    the ranks, backwards on the odd ones."""
    lap, at = divmod(pos, world)
    return at if lap % 2 == 0 else world - 1 - at


def snake_count(n: int, world: int, r: int) -> int:
    """How many of the positions 0 .. n - 1 rank r owns (snake_count's closed form, from its
    comment): a forward and a backward lap together give every rank two; of what remains, rank r's
    forward place is the r-th and its backward place the r-th from the end of the pair of laps."""
    pair = 2 * world
    full, rem = divmod(n, pair)
    return 2 * full + (1 if rem > r else 0) + (1 if rem > pair - 1 - r else 0)


def snake_pick(j: int, world: int, r: int) -> int:
    """The list position of rank r's j-th cluster (k_shard_pick's closed form, from its comment):
    its members alternate between the forward place (even j) and the backward place (odd j) of the
    j // 2-th pair of laps."""
    pair = 2 * world
    return (j // 2) * pair + (r if j % 2 == 0 else pair - 1 - r)


def owner_of(shapes: List[dict], world: int) -> List[int]:
    """Each cluster's owner, in the order of `shapes` (dispatch_shapes.cluster_shapes, whose `rank`
    is the place in k_cl_sizekey's order): `world` for a replicated cluster, else the rank it is
    dealt to.

    The device sorts the clusters once (k_cl_sizekey: workgroup class first, rows descending, index)
    and uses the two halves of that one list, in this order: D.big is `sorted` itself with n_big =
    the workgroup-class count, and D.small = sorted[n_big + i] (k_cl_small_ids with h = 0) -- gpu_clusters'
    "elimination split".  run_linear_simplification then replicates the first min(n_big, kHeadLimit)
    of D.big (k_fill_u8_ids with owner W), deals D.big + n_rep by position (k_shard_owner: the
    position counts from the first cluster behind the head) and deals D.small by position.  So with
    rank = the place in `sorted`: rank < min(n_wg, kHeadLimit) is replicated, a workgroup cluster
    behind that goes to snake(rank - kHeadLimit), a lane cluster to snake(rank - n_wg)."""
    n_wg = sum(1 for c in shapes if c["wg"])
    n_rep = min(n_wg, k.kHeadLimit)
    out = []
    for c in shapes:
        if c["wg"]:
            assert c["rank"] < n_wg
            out.append(world if c["rank"] < n_rep else snake(c["rank"] - k.kHeadLimit, world))
        else:
            assert c["rank"] >= n_wg
            out.append(snake(c["rank"] - n_wg, world))
    return out


def shares(shapes: List[dict], world: int) -> dict:
    """Per rank, the cluster indices it is dealt: `tail` (workgroup class behind the head) and `lane`,
    each in list order; `replicated` the head's."""
    own = owner_of(shapes, world)
    by_rank = sorted(range(len(shapes)), key=lambda c: shapes[c]["rank"])
    out = dict(replicated=[c for c in by_rank if own[c] == world], tail=[[] for _ in range(world)], lane=[[] for _ in range(world)])
    for c in by_rank:
        if own[c] < world:
            out["tail" if shapes[c]["wg"] else "lane"][own[c]].append(c)
    return out


# ============================================================================ the exchange
def _round_model(shapes, rows, subs, relevant, world) -> dict:
    """rows: the round's non-empty linear rows as `shapes` indexes them; subs: the round's log entries
    [(from, to)]."""
    own = owner_of(shapes, world)
    cluster_of: Dict[int, int] = {}
    for c in shapes:
        for j in c["row_ids"]:
            for s in rows[j].c:
                if s:
                    assert cluster_of.setdefault(s, c["index"]) == c["index"]
    exchanged = []
    for frm, to in subs:
        assert 0 in to, "a right-hand side without its constant slot"
        c = cluster_of[frm]
        if own[c] < world:
            exchanged.append(dict(frm=frm, cluster=c, owner=own[c], len=len(to), zeros=ds.zero_keys(to)))
    return dict(world=world, shapes=shapes, owner=own, exchanged=exchanged, relevant=relevant, n_subs=len(subs),
                kept=[e for e in exchanged if e["frm"] in relevant], dropped=[e for e in exchanged if e["frm"] not in relevant])


def filtered_bytes(model: dict) -> int:
    """What the filter saves in one exchange: the entries of the exchanged right-hand sides whose
    `from` nothing needs (a record travels either way; an entry is a 4-byte key and a 32-byte value)."""
    return ENTRY_BYTES * sum(e["len"] for e in model["dropped"])


def _log1(sys_, old):
    return rsio.pyref_log(R.simplification(sys_, R.Flags(no_rounds=1, use_old_heuristics=old), want_log=True).log)


def exchange_model(sys_: "R.System", flags: "R.Flags", world: int, log1=None) -> dict:
    """Round 1 of a sharded run of `sys_` at `world` ranks, from pyref alone (log1: the log of the run
    at no_rounds = 1 as [(from, to)], pyref's when not given):

      exchanged  the substitutions of the clusters with owner < world, each with `frm`, its cluster
                 and owner and `len`, the right-hand side's length as the pool stores it.  That is
                 the length of the logged `to` map: explicit zero keys count (raw_substitution keeps
                 them and nothing prunes the pool), and so does the constant key -- every pool map
                 holds key 0 whether or not the row had a constant term (d_raw_sub_into: "both maps
                 hold key 0"; k_eliminate and k_big_emit write h_len = the map's length with it, and
                 log_linear_round copies h_len entries per substitution, which is why every logged
                 `to` has a key 0);
      relevant   build_relevant_set as k_mark_relevant restates it: the signals of the non-linear rows
                 as they came in, renamed by the eq substitutions that are plain signals, minus those
                 a constant equality defines;
      kept / dropped   exchanged with `frm` in / not in relevant: with the log off only the first
                 travel with their entries; with it on (`need` null) all do."""
    old = bool(flags.use_old_heuristics)
    linear, non_linear, single, const_subs = ds.linear_after_frames(sys_)
    relevant = set()
    for c in non_linear:
        for s in R.take_cloned_signals(c):
            e = single.get(s)
            s2 = e.symbol if e is not None and e.kind == "Signal" else s
            if s2 not in const_subs:
                relevant.add(s2)
    shapes = ds.cluster_shapes(sys_, old)
    if flags.flag_s:
        return _round_model(shapes, [], [], relevant, world)
    rows = [c for c in linear if not R.is_empty(c)]
    log1 = _log1(sys_, old) if log1 is None else log1
    subs = [(frm, to) for frm, to in log1 if frm not in single and frm not in const_subs]
    return _round_model(shapes, rows, subs, relevant, world)


def round2_system(sys_: "R.System", old=False):
    """(the rows round 1 turned linear as a System of their own, the storage rows round 1 left): round
    2's linear_simplification sees exactly the first (the frames of dispatch_shapes.round2_shapes)."""
    p = sys_.p
    log1 = R.simplification(sys_, R.Flags(no_rounds=1, use_old_heuristics=old), want_log=True).log
    _, non_linear, single, const_subs = ds.linear_after_frames(sys_)
    lin1 = R.build_encoded_fast_substitutions([s for s in log1 if s.frm not in single and s.frm not in const_subs])
    turned, storage = [], []
    for c0 in non_linear:
        c = c0.clone()
        for fr in (single, const_subs, lin1):
            R.fast_encoded_constraint_substitution(c, fr, p)
        R.fix_constraint(c, p)
        if not R.is_linear(c):
            storage.append(c)
        elif not R.is_empty(c):
            turned.append(c)
    sys2 = R.System(p, sys_.max_signal, sys_.n_pub_out, sys_.n_pub_in, sys_.n_priv_in, set(sys_.forbidden), turned)
    cons_eq, eqs, lin, nl = R.classify(sys2)
    assert not cons_eq and not eqs and not nl and len(lin) == len(turned), "a turned row the clustering would not see as linear"
    return sys2, storage


def round2_model(sys_: "R.System", flags: "R.Flags", world: int) -> dict:
    """exchange_model for round 2: the clusters of the rows round 1 turned linear, the substitutions
    pyref logs at no_rounds = 2 beyond those at no_rounds = 1, and as the needed set the keys of the
    non-linear signal map when round 2 starts -- the signals of the storage rows (`nlmap`)."""
    old = bool(flags.use_old_heuristics)
    sys2, storage = round2_system(sys_, old)
    log1 = _log1(sys_, old)
    log2 = rsio.pyref_log(R.simplification(sys_, R.Flags(no_rounds=2, use_old_heuristics=old), want_log=True).log)
    assert log2[:len(log1)] == log1
    needed = set(R.build_non_linear_signal_map(storage))
    return _round_model(ds.cluster_shapes(sys2, old), sys2.rows, log2[len(log1):], needed, world)


# ============================================================================ the cluster a case is about
def family(name: str) -> str:
    """ds.log_family, with the cancellation cases under the family of the path they cancel on."""
    if name.startswith("cancel_"):
        return "merge"
    if name.startswith("zero_round2"):
        return "round2"
    if name.startswith("zero_"):
        return "compose"
    return ds.log_family(name)


def is_round2(name: str) -> bool:
    return family(name) == "round2"


def under_test(shapes: List[dict], info) -> Optional[dict]:
    """The cluster a case is about: the one of info["n"] rows where the builder names it; else the
    last workgroup-class cluster of the size order (the kHeadLimit and kTailSplit cases put theirs
    there) or, with none, the largest lane-class one (the frames cases' stars); None without clusters."""
    if isinstance(info, dict) and "n" in info:
        return ds._the(shapes, info["n"])
    if not shapes:
        return None
    wg = [c for c in shapes if c["wg"]]
    return max(wg, key=lambda c: c["rank"]) if wg else min(shapes, key=lambda c: c["rank"])


def kind_of(model: dict, info) -> str:
    """"replicated" or "exchanged" for the cluster under test ("none": the round has no cluster)."""
    c = under_test(model["shapes"], info)
    if c is None:
        return "none"
    return "replicated" if model["owner"][c["index"]] == model["world"] else "exchanged"


# ============================================================================ cases the families lacked
SHARD_EXTRA: List[Case] = []


def _extra_frames():
    """frames: every star of the frames cases is a one-row lane-class cluster, so none is replicated,
    and each is a signal of its row, so none is filtered.  Here row 0 holds a star of kHeavyNnz terms
    (kHeavyNnz + 1 entries: workgroup class, the head's only cluster) and a short one; a third star
    no row holds is exchanged and not relevant."""
    name = "frames_head_star"

    def build(p):
        b = Builder(_seed(name), p)
        ds.quad(b, ["p"], ["p"], [k.kHeavyNnz, 3])
        idle = ds.star(b, 5)
        return b.system(), dict(idle=idle)

    def certify(sys_, info, old):
        sh = ds.cluster_shapes(sys_, old)
        nl = ds.nonlinear_shapes(sys_, old)
        m = exchange_model(sys_, R.Flags(use_old_heuristics=old), DISPATCH_WORLD)
        return [("clusters (rows, workgroup class) in size order", [(c["rows"], c["wg"]) for c in sorted(sh, key=lambda c: c["rank"])],
                 [(1, True), (1, False), (1, False)]),
                ("entries of the long star's row", max(c["entries"] for c in sh), k.kHeavyNnz + 1),
                ("row 0 terms", nl[0]["terms"], 2 + k.kHeavyNnz + 3),
                ("owners in size order", [m["owner"][c["index"]] for c in sorted(sh, key=lambda c: c["rank"])], [DISPATCH_WORLD, 0, 1]),
                ("exchanged and not relevant", [e["frm"] for e in m["dropped"]], [info["idle"]]),
                ("exchanged and relevant", len(m["kept"]), 1)]
    SHARD_EXTRA.append(Case(name, build, certify, n_rounds={None: 1}))


def _extra_round2():
    """round2: each late star of the round2_* cases is a one-row lane-class cluster of round 2, so none
    is replicated.  Here one late star has kHeavyNnz terms: its row is round 2's only workgroup-class
    cluster (replicated), beside a short one (dealt)."""
    name = "round2_head_star"

    def build(p):
        b = Builder(_seed(name), p)
        ds.storage_row(b, 2, [k.kHeavyNnz, 4])
        return b.system(), None

    def certify(sys_, info, old):
        r2 = ds.round2_shapes(sys_, old)
        m = round2_model(sys_, R.Flags(use_old_heuristics=old), DISPATCH_WORLD)
        sh = sorted(m["shapes"], key=lambda c: c["rank"])
        st = [r for r in r2["rows"] if r["touched"]]
        return [("round-2 substitutions", r2["n_subs"], 2), ("storage rows round 2 touches", len(st), 1),
                ("round-2 terms", st[0]["terms"] if st else None, 4 + k.kHeavyNnz + 4),
                ("round-2 clusters (rows, workgroup class)", [(c["rows"], c["wg"]) for c in sh], [(1, True), (1, False)]),
                ("owners", [m["owner"][c["index"]] for c in sh], [DISPATCH_WORLD, 0]),
                ("exchanged and needed", len(m["kept"]), 1)]
    SHARD_EXTRA.append(Case(name, build, certify, rounds=(None, 2), n_rounds={None: 2, 2: 2}))


def _extra_row():
    """row: the row cases probe every signal of the cluster they are about, so in the tail placement
    every exchanged right-hand side is relevant and the filter drops nothing.  Here the tail placement
    of dispatch_shapes._placed carries two probes only: the long row (one past the tail loop's
    capacity) is still exchanged, and most of its cluster's substitutions are filtered."""
    name, length = f"row_tail_{k.tail_cap + 1}_two_probes", k.tail_cap + 1

    def build(p):
        b = Builder(_seed(name), p)
        glue = b.forbid(1)[0]
        n = k.kWaveMin + 8
        for f in ds.fillers(b, _filler_sizes(n + 3, k.kHeadLimit)):
            b.probes(f["probe"], 1)
        low = b.take(k.spec_cap + 8)     # ids below the chain's
        cl = ds.chain(b, n, glue=glue)
        cl["low"] = low
        b.probes(cl["probe"], 2)
        ds.wide_row(b, cl, length, fresh_ok=True)
        cl["n"] += 1
        return b.system(), cl

    def certify(sys_, cl, old):
        c = ds._the(ds.cluster_shapes(sys_, old), cl["n"])
        tr = ds.elimination_trace(ds.cluster_rows(sys_, c), sys_.forbidden, sys_.p, c["p4"])
        m = exchange_model(sys_, R.Flags(use_old_heuristics=old), DISPATCH_WORLD)
        mine = [e for e in m["exchanged"] if e["cluster"] == c["index"]]
        return ds._placement_checks(c, "tail") + [("longest row", c["max_row_len"], length),
                                                  ("longest row reaches the ordered loop", max(tr["pops"]), length),
                                                  ("the cluster is the only one exchanged", len(mine) == len(m["exchanged"]) > 0, True),
                                                  ("some of its substitutions are relevant", 0 < len(m["kept"]) <= 6, True),
                                                  ("most are not", len(m["dropped"]) >= len(mine) - 6, True)]
    SHARD_EXTRA.append(Case(name, build, certify, n_rounds={None: 1}))


_extra_frames()
_extra_round2()
_extra_row()


# ============================================================================ inputs for the deal
class DealCase:
    """kHeadLimit replicated fillers, t dealt workgroup-class clusters, s dealt lane-class clusters."""

    def __init__(self, t: int, s: int):
        self.t, self.s, self.name = t, s, f"t{t}_s{s}"

    def __repr__(self):
        return self.name

    def build(self, p):
        b = Builder(_seed("deal_" + self.name), p)
        head = ds.fillers(b, _filler_sizes(k.kWaveMin, k.kHeadLimit))          # kWaveMin + 1 + i rows
        for f in head:
            b.probes(f["probe"], 1)
        # the tail: distinct row counts from kWaveMin down; below kWaveMin rows the entries make the class
        tail = []
        for i in range(self.t):
            n = k.kWaveMin - i
            assert n >= 4 and 3 * n <= k.kHeavyNnz
            tail.append(ds.chain(b, n) if i == 0 else ds.blob(b, n, k.kHeavyNnz))
        lane = [ds.chain(b, 4 + i) for i in range(self.s)]
        assert 3 * (4 + self.s) < k.kHeavyNnz and 4 + self.s <= k.kWaveMin
        for cl in tail + lane:      # every signal of a dealt cluster reaches a non-linear row
            b.probes(cl["probe"])
        return b.system(), dict(tail=[c["n"] for c in tail], lane=[c["n"] for c in lane])


def deal_counts(world: int) -> List[int]:
    """The list lengths at which the snake's closed forms change: none, one, a lap of the ranks less
    one, a lap, one more, a pair of laps less one, the pair, one more."""
    return sorted({0, 1, world - 1, world, world + 1, 2 * world - 1, 2 * world, 2 * world + 1})


_DEAL: Dict[tuple, DealCase] = {}


def deal_cases(world: int) -> List[DealCase]:
    """t over deal_counts(world) with three lane clusters, then s over the same counts with one tail
    cluster (the inputs do not depend on `world`; the counts do)."""
    out = []
    for t, s in [(t, 3) for t in deal_counts(world)] + [(1, s) for s in deal_counts(world) if s != 3]:
        out.append(_DEAL.setdefault((t, s), DealCase(t, s)))
    return out


# ============================================================================ what the GPU tests run
LARGEST = {"dispatch": "kFinWaveBelow+1", "cancel": "zero_tail_kMergeD+1"}   # by rows (test_shard_cases proves it): the empty input follows


def first_variant(case: Case):
    return ds.variants(case)[0]
