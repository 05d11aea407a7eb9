"""CPU certificates for the sharded path's cases (shard_cases.py; no GPU):
  * the snake deal: owner_of and the two closed forms (snake_count, k_shard_pick, re-derived from
    their comments) against dealing the positions one by one, at every list length up to 4 W + 3;
  * every deal case has exactly kHeadLimit replicated clusters, t dealt workgroup clusters and s dealt
    lane clusters, and the cases of a world together leave a rank without a tail cluster, a rank
    without a lane cluster and give every rank a forward and a backward place;
  * every certified dispatch case (world 3) and cancellation case (world 2): whether the cluster it is
    about is replicated or exchanged, the exact census per family, and that per family the filter
    both keeps and drops an exchanged right-hand side (a filter that drops everything, or a log-on
    run that cannot differ from a log-off one, would otherwise pass);
  * round 2: the round-2 clusters of the round2 family are dealt and their `from` is needed;
  * the compose cancellations exchange a right-hand side with an explicit zero key."""
import itertools

import pytest

import dispatch_shapes as ds
import rsio
import shard_cases as sc

R = rsio.R
BN = R.PRIMES["bn128"]
k = ds.k


# ---------------------------------------------------------------------------- the snake
def _dealt_one_by_one(n, world):
    """members[r] = the positions rank r gets when 0 .. n - 1 are handed out along 0, 1, .., W - 1,
    W - 1, .., 0, 0, 1, .."""
    walk = itertools.cycle(list(range(world)) + list(reversed(range(world))))
    members = [[] for _ in range(world)]
    for pos in range(n):
        members[next(walk)].append(pos)
    return members


def _synthetic(n_wg, n_lane):
    """Shapes as owner_of reads them: n_wg workgroup-class clusters then n_lane lane-class ones, ranked
    in that order, listed in another."""
    sh = [dict(wg=r < n_wg, rank=r, index=r) for r in range(n_wg + n_lane)]
    return sh[1::2] + sh[0::2]


@pytest.mark.parametrize("world", [2, 3, 4])
def test_snake_against_brute_force(world):
    H = k.kHeadLimit
    for n in range(4 * world + 4):
        members = _dealt_one_by_one(n, world)
        assert sorted(p for m in members for p in m) == list(range(n))
        for r in range(world):
            assert sc.snake_count(n, world, r) == len(members[r]), (n, r)
            assert [sc.snake_pick(j, world, r) for j in range(len(members[r]))] == members[r], (n, r)
        # the same list as the tail behind a full head, and as the lane list behind it
        for n_wg, n_lane in ((H + n, 2), (H, n), (H - 1, n), (0, n), (H + 3, n)):
            sh = _synthetic(n_wg, n_lane)
            own = dict((c["rank"], o) for c, o in zip(sh, sc.owner_of(sh, world)))
            assert [own[r] for r in range(min(n_wg, H))] == [world] * min(n_wg, H)
            tail = _dealt_one_by_one(max(0, n_wg - H), world)
            lane = _dealt_one_by_one(n_lane, world)
            for r in range(world):
                assert [q - H for q in range(H, n_wg) if own[q] == r] == tail[r], (n_wg, n_lane, r)
                assert [q - n_wg for q in range(n_wg, n_wg + n_lane) if own[q] == r] == lane[r], (n_wg, n_lane, r)


def test_deal_counts():
    assert sc.deal_counts(2) == [0, 1, 2, 3, 4, 5]
    assert sc.deal_counts(3) == [0, 1, 2, 3, 4, 5, 6, 7]
    assert sc.deal_counts(4) == [0, 1, 3, 4, 5, 7, 8, 9]
    for w in sc.DEAL_WORLDS:
        cs = sc.deal_cases(w)
        assert len({c.name for c in cs}) == len(cs)
        assert {(c.t, c.s) for c in cs} == {(t, 3) for t in sc.deal_counts(w)} | {(1, s) for s in sc.deal_counts(w)}


# ---------------------------------------------------------------------------- the deal cases
_DEAL_SHAPES = {}


def _deal_shapes(case):
    if case.name not in _DEAL_SHAPES:
        sys_, info = case.build(BN)
        _DEAL_SHAPES[case.name] = (ds.cluster_shapes(sys_), info, len(sys_.rows))
    return _DEAL_SHAPES[case.name]


_DEALS = [(w, c) for w in sc.DEAL_WORLDS for c in sc.deal_cases(w)]


@pytest.mark.parametrize("world,case", _DEALS, ids=[f"{c.name}-w{w}" for w, c in _DEALS])
def test_deal_case(world, case):
    shapes, info, n_rows = _deal_shapes(case)
    H = k.kHeadLimit
    assert n_rows < 12000
    by_rank = sorted(shapes, key=lambda c: c["rank"])
    assert len(shapes) == H + case.t + case.s
    assert [c["wg"] for c in by_rank] == [True] * (H + case.t) + [False] * case.s
    # the order is decided by size alone: distinct row counts inside each list
    assert [c["rows"] for c in by_rank[:H]] == [k.kWaveMin + H - i for i in range(H)]
    assert [c["rows"] for c in by_rank[H:H + case.t]] == info["tail"] == [k.kWaveMin - i for i in range(case.t)]
    assert [c["rows"] for c in by_rank[H + case.t:]] == sorted(info["lane"], reverse=True) and len(set(info["lane"])) == case.s
    assert all(c["entries"] >= k.kHeavyNnz for c in by_rank[H + 1:H + case.t])      # under kWaveMin rows: heavy
    assert all(c["entries"] < k.kHeavyNnz and c["rows"] < k.kWaveMin for c in by_rank[H + case.t:])
    sh = sc.shares(shapes, world)
    assert len(sh["replicated"]) == H
    for r in range(world):
        assert len(sh["tail"][r]) == sc.snake_count(case.t, world, r)
        assert len(sh["lane"][r]) == sc.snake_count(case.s, world, r)
        assert [shapes[c]["rank"] - H for c in sh["tail"][r]] == [sc.snake_pick(j, world, r) for j in range(len(sh["tail"][r]))]
        assert [shapes[c]["rank"] - H - case.t for c in sh["lane"][r]] == [sc.snake_pick(j, world, r) for j in range(len(sh["lane"][r]))]


@pytest.mark.parametrize("world", sc.DEAL_WORLDS)
def test_deal_cases_cover_the_remainders(world):
    no_tail = no_lane = False
    parities = {(lst, r): set() for lst in ("tail", "lane") for r in range(world)}
    for case in sc.deal_cases(world):
        sh = sc.shares(_deal_shapes(case)[0], world)
        no_tail |= any(not sh["tail"][r] for r in range(world)) and any(sh["tail"][r] for r in range(world))
        no_lane |= any(not sh["lane"][r] for r in range(world)) and any(sh["lane"][r] for r in range(world))
        for lst in ("tail", "lane"):
            for r in range(world):
                parities[lst, r] |= {j & 1 for j in range(len(sh[lst][r]))}
    assert no_tail, "no case leaves a rank without a tail cluster while another has one"
    assert no_lane, "no case leaves a rank without a lane cluster while another has one"
    assert all(v == {0, 1} for v in parities.values()), parities


# ---------------------------------------------------------------------------- replicated or exchanged
_LISTS = {"dispatch": (sc.SHARD_DISPATCH, sc.DISPATCH_WORLD), "cancel": (sc.SHARD_CANCEL, sc.CANCEL_WORLD),
          "extra": (sc.SHARD_EXTRA, sc.DISPATCH_WORLD)}
_MODELS = {}


def _model(lst, case):
    """(kind, model of the round the case is about, rows, info) at the case's first variant."""
    key = (lst, case.name)
    if key not in _MODELS:
        prime, old, _rounds = sc.first_variant(case)
        sys_, info = case.build(R.PRIMES[prime])
        fl = R.Flags(use_old_heuristics=old)
        m = sc.round2_model(sys_, fl, _LISTS[lst][1]) if sc.is_round2(case.name) else sc.exchange_model(sys_, fl, _LISTS[lst][1])
        slim = dict(kept=m["kept"], dropped=m["dropped"], exchanged=m["exchanged"], n_subs=m["n_subs"])
        _MODELS[key] = (sc.kind_of(m, info), slim, len(sys_.rows), info)
    return _MODELS[key]


_ALL = [(lst, c) for lst in _LISTS for c in _LISTS[lst][0]]


@pytest.mark.parametrize("lst,case", _ALL, ids=[f"{lst}-{c.name}" for lst, c in _ALL])
def test_kind(lst, case):
    kind, m, _rows, _info = _model(lst, case)
    assert kind in ("replicated", "exchanged", "none")
    assert len(m["kept"]) + len(m["dropped"]) == len(m["exchanged"]) <= m["n_subs"]
    if kind == "none":
        assert m["n_subs"] == 0
    if kind == "replicated" and lst != "extra" and not sc.is_round2(case.name):
        # what the case names is in the head; in the tail placements it would not be
        assert "_tail" not in case.name


def _census(lst):
    out = {}
    for case in _LISTS[lst][0]:
        key = (sc.family(case.name), _model(lst, case)[0])
        out[key] = out.get(key, 0) + 1
    return out


# A retuned constant that moves a case across the head's edge, or a new case, shows up here.
CENSUS = {
    "dispatch": {("cluster", "exchanged"): 11, ("cluster", "replicated"): 31, ("compose", "exchanged"): 15, ("compose", "replicated"): 15,
                 ("frames", "exchanged"): 8, ("frames", "none"): 6, ("giant", "replicated"): 6, ("merge", "exchanged"): 6,
                 ("merge", "replicated"): 15, ("round2", "exchanged"): 5, ("row", "exchanged"): 7, ("row", "replicated"): 16},
    "cancel": {("compose", "exchanged"): 9, ("compose", "replicated"): 9, ("frames", "exchanged"): 8, ("merge", "exchanged"): 3,
               ("merge", "replicated"): 12, ("round2", "exchanged"): 3},
    "extra": {("frames", "replicated"): 1, ("round2", "replicated"): 1, ("row", "exchanged"): 1},
}


@pytest.mark.parametrize("lst", list(_LISTS))
def test_census(lst):
    assert _census(lst) == CENSUS[lst]


def test_every_family_has_both_kinds():
    """Over the three lists together.  The giant family is the exception by construction: the giant
    path (giant_loop.hpp) takes head clusters only -- run_linear_simplification looks for giants among
    the first n_head positions -- and the head is replicated, so no input places it on the exchanged
    side; a cluster of kGiantRows rows behind kHeadLimit larger ones would be an ordinary tail cluster
    of an input of over a million rows."""
    have = {}
    for lst in _LISTS:
        for (fam, kind), n in _census(lst).items():
            have.setdefault(fam, set()).add(kind)
    assert set(have) == {"cluster", "row", "merge", "compose", "giant", "round2", "frames"}
    for fam, kinds in have.items():
        if fam == "giant":
            assert kinds == {"replicated"}
        else:
            assert kinds >= {"replicated", "exchanged"}, f"{fam}: {kinds}"


def test_the_filter_is_observable():
    """Per family, some case exchanges a right-hand side the filter keeps and some case one it drops
    (round 1's relevant set; for the round2 family round 2's needed set).  Giant: see above -- its
    inputs are one cluster, nothing is exchanged."""
    kept, dropped = {}, {}
    for lst in _LISTS:
        for case in _LISTS[lst][0]:
            fam = sc.family(case.name)
            _, m, _, _ = _model(lst, case)
            kept[fam] = kept.get(fam, 0) + bool(m["kept"])
            dropped[fam] = dropped.get(fam, 0) + bool(m["dropped"])
    for fam in ("cluster", "row", "merge", "compose", "round2", "frames"):
        assert kept[fam] >= 1, f"{fam}: no case exchanges a needed right-hand side"
        assert dropped[fam] >= 1, f"{fam}: no case exchanges a right-hand side the filter drops"
    assert kept["giant"] == dropped["giant"] == 0


def test_round2_clusters_are_dealt():
    """The round-2 cluster of every round2_* case (and of zero_round2) is dealt, not replicated, and
    the filter of rounds >= 2 keeps it: its `from` is a key of a storage row.  round2_head_star is
    the replicated one."""
    n = 0
    for lst in ("dispatch", "cancel"):
        for case in _LISTS[lst][0]:
            if not sc.is_round2(case.name):
                continue
            kind, m, _, _ = _model(lst, case)
            assert kind == "exchanged", case.name
            assert m["exchanged"] and len(m["exchanged"]) == m["n_subs"], case.name
            assert m["kept"], case.name
            if case.name.startswith("round2_terms") or case.name.startswith("round2_entries"):
                assert not m["dropped"], case.name      # every late star is a key of the storage row
            n += 1
    assert n == 5 + 2 + 1
    assert _model("extra", [c for c in sc.SHARD_EXTRA if c.name == "round2_head_star"][0])[0] == "replicated"


def test_zero_keys_survive_the_model():
    """The compose cancellations on the exchanged side hand over a right-hand side with an explicit
    zero-valued non-constant key: s's and t's, with exactly the keys the gadget built."""
    n = 0
    for case in sc.SHARD_CANCEL:
        if sc.family(case.name) != "compose":
            continue
        kind, m, _, info = _model("cancel", case)
        by = {e["frm"]: e for e in m["exchanged"]}
        if kind == "exchanged":
            assert by[info["s"]]["zeros"] == sorted(info["zeros"]) == by[info["t"]]["zeros"], case.name
            n += 1
        else:
            assert info["s"] not in by and info["t"] not in by
    assert n >= 8      # six tail compositions, the lane one, zero_all_tail and zero_all_lane


def test_largest_cases():
    for lst, name in sc.LARGEST.items():
        rows = {c.name: _model(lst, c)[2] for c in _LISTS[lst][0]}
        assert rows[name] == max(rows.values()), (lst, max(rows, key=rows.get))


# ---------------------------------------------------------------------------- the added cases
@pytest.mark.parametrize("case", sc.SHARD_EXTRA, ids=[c.name for c in sc.SHARD_EXTRA])
def test_extra_case(case):
    """Shape, linear rounds, and refcpu's log equal to pyref's literal one (its licence as the GPU
    test's reference, as tests/test_dispatch_shapes.py gives it for the dispatch cases)."""
    prime, old, _ = sc.first_variant(case)
    sys_, info = case.build(R.PRIMES[prime])
    checks = case.certify(sys_, info, old)
    for rd, want in (case.n_rounds or {}).items():
        checks.append((f"linear rounds at rounds={rd}", ds.linear_rounds(sys_, rd, old), want))
    bad = [(what, got, want) for what, got, want in checks if got != want or type(got) is not type(want)]
    assert not bad, f"{case.name}: (quantity, certificate, intended) {bad}"
    h = rsio.InputHolder(sys_)
    for rd in case.rounds:
        fl = rsio.flags("O2", rd, old, log=True)
        res = R.simplification(sys_, rsio.py_flags(fl), want_log=True)
        cons, sm, npiw, log = rsio.oracle_run_log(h.inp, fl, threads=8)
        assert ds.log_diff(log, rsio.pyref_log(res.log)) is None
        assert rsio.same_result(res, (cons, sm, len(sm), npiw)) is None
