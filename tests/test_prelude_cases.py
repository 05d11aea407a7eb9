"""CPU proofs for the cases of prelude_cases.py (no GPU):
  * every case's certificate equals what the case claims (equality classes, constants, the border to
    the linear rows, the list order of a cluster), and the table holds exactly the named cases;
  * replay_trace's order is build_clusters' on every order_* case, no case is a chain or order-free,
    every counter class occurs on every replay path and the three window conditions on the wave path;
  * each order_* result changes under three wrong list orders (the pairs that do not are DROPPED, at
    most one in ten), within the cost caps of elimination_trace;
  * refcpu's substitution log equals pyref's literal one on every case, which licenses refcpu as the
    reference of tests/test_gpu_prelude.py, and the rs_stats figures that file asserts are pyref's."""
import pytest

import dispatch_shapes as ds
import input_contract as ic
import prelude_cases as pc
import rsio

R = rsio.R
k = ds.k


# ---------------------------------------------------------------------------- replay_trace itself
def test_replay_trace_on_small_inputs():
    # a chain: every row prepends itself to the one list and links one root at depth 0
    tr = pc.replay_trace([[1, 2], [2, 3], [3, 4], [4, 5]])
    assert tr["lists"] == [[3, 2, 1, 0]] and (tr["multi_root_rows"], tr["max_roots"], tr["max_find"], tr["own_pairs"]) == (0, 1, 0, 0)
    # two lists joined by a row that holds 5 (of row 1's list) before 9 (of row 3's): [row] ++ list(1) ++ list(3)
    rows = [[1, 5], [5, 6], [8, 9], [9, 10], [5, 9]]
    tr = pc.replay_trace(rows)
    assert tr["lists"] == [[4, 1, 0, 3, 2]] and (tr["multi_root_rows"], tr["max_roots"]) == (1, 2)
    assert pc.replay_trace(rows, descending=True)["lists"] == [[4, 3, 2, 1, 0]]
    # a pair whose root is already in the row's own list, found one step up
    tr = pc.replay_trace([[1, 2], [2, 3], [1, 3]])
    assert tr["lists"] == [[2, 1, 0]] and tr["own_pairs"] == 1 and tr["max_find"] == 1
    # window alignment: 63 single-key rows, then a row whose first entry is entry 63 and which straddles
    tr = pc.replay_trace([[100 + i] for i in range(63)] + [list(range(1, 70))])
    assert tr["first_at_63"] and tr["straddle"] and tr["gt64"] and not tr["gt128"] and tr["max_pairs"] == 69
    # the same lists as build_clusters, on a random input of several clusters
    b = ds.Builder(3, R.PRIMES["bn128"])
    for keys in pc.sliding(b, 40) + pc.tournament(b, 21):
        pc._row(b, keys)
    lin = R.classify(b.system())[2]
    at = {id(c): i for i, c in enumerate(lin)}
    assert [[at[id(c)] for c in cl] for cl in R.build_clusters(lin, b.nxt)] == pc.replay_trace([[s for s in c.c if s] for c in lin])["lists"]


# ---------------------------------------------------------------------------- shape proofs
_SHAPES = [(c, old) for c in pc.CASES for old in c.olds]


@pytest.mark.parametrize("case,old", _SHAPES, ids=[f"{c.name}{'-old' if o else ''}" for c, o in _SHAPES])
def test_shape(case, old):
    sys_, info = pc.built(case)
    checks = case.certify(sys_, info, old)
    assert checks
    bad = [(what, got, want) for what, got, want in checks if got != want or type(got) is not type(want)]
    assert not bad, f"{case.name}: (quantity, certificate, intended) {bad}"
    if case.family != "order":
        assert len(sys_.rows) < 100 or case.name.startswith("eq_union_")


def test_case_table_is_exact():
    want = {"eq_single", "eq_multi", "eq_order", "const_forms", "const_renamed", "const_batch_mixed", "const_batch_none", "border",
            "order_multi", "order_round2"}
    want |= {f"eq_union_{s}_f{f}" for s in ("chain", "chain_reversed", "star_hub_smallest", "star_hub_largest", "pairing_tree", "chain_x8")
             for f in (0, 2)}
    want |= {f"const_batch_{n}" for n in (1, 7, 8, 9, 16, 17)}
    sizes = {"lane": (k.kClSmall - 1, k.kClSmall), "wave": (k.kClSmall + 1, 701, k.kClMid), "host": (k.kClMid + 1, 5003, k.kClLds),
             "lane_global": (k.kClLds + 1,)}
    table = dict(pc._order_table())
    assert sorted(table) == sorted(n for ns in sizes.values() for n in ns)
    for path, ns in sizes.items():
        assert all(pc.replay_path(n) == path for n in ns)
        assert len({t for n in ns for t in table[n]}) >= 2, f"fewer than two topologies on the {path} path"
    want |= {f"order_{t}_{n}" for n, ts in table.items() for t in ts}
    assert {c.name for c in pc.CASES} == want
    topos = {t for ts in table.values() for t in ts}
    assert {f"late_star{j}" for j in (2, 16, 63, 64, 65, 130)} | {"tournament", "sliding", "dense"} <= topos
    assert any(t.startswith("interleaved") for t in topos)
    by = {c.name: c for c in pc.CASES}
    for c in pc.CASES:
        if c.family == "order":
            assert c.olds == (False, True)
        else:
            assert c.primes == ("bn128", "goldilocks")
        assert c.twice == c.name.startswith("eq_union_")
    # through rs_engine_simplify too, as given and with the keys of every eq row reversed: A1, A2's forbidden cases, B2, B4
    assert {c.name for c in pc.CASES if c.simplify} == {"eq_single", "eq_multi", "eq_order", "const_renamed", "border"}
    for nm in ("eq_single", "eq_multi", "eq_order", "const_renamed", "border"):
        h = rsio.InputHolder(pc.built(by[nm])[0], "bn128")
        assert ic.permute(h, "reversed", [ic.EQ])[1][ic.EQ] == int(h.inp.eq.n_rows) > 0


# ---------------------------------------------------------------------------- the list order
_ORDER = [(c, old) for c in pc.CASES for old in c.olds if c.family == "order" and c.name != "order_multi"]


def test_order_sensitivity_and_dropped_pairs():
    """The arena-order result differs from the result on each wrong order, for every (case, heuristics)
    but the DROPPED ones -- which are exactly the pairs that fail, and at most one in ten."""
    fails = {(c.name, old): pc.order_proof(c, old)["sens"] for c, old in _ORDER if not all(pc.order_proof(c, old)["sens"].values())}
    assert set(fails) == set(pc.DROPPED), fails
    assert 10 * len(pc.DROPPED) <= len(_ORDER)


def test_counters_cover_every_path():
    seen = {}
    for c, old in _ORDER:
        tr = pc.order_proof(c, old)["view"]["trace"]
        s = seen.setdefault(c.path, set())
        s |= {nm for nm, on in (("two roots in a row", tr["multi_root_rows"] > 0), ("many roots in a row", tr["max_roots"] >= 16),
                                ("a find path of 4 or more", tr["max_find"] >= 4), ("a pair in the row's own list", tr["own_pairs"] > 0),
                                ("a row of more than 3 pairs", tr["max_pairs"] > 3), ("first pair at entry 63", tr["first_at_63"]),
                                ("a row across a window border", tr["straddle"]), ("more than 64 pairs", tr["gt64"]),
                                ("more than 128 pairs", tr["gt128"])) if on}
    assert set(seen) == {"lane", "wave", "host", "lane_global"}
    classes = {"two roots in a row", "many roots in a row", "a find path of 4 or more", "a pair in the row's own list", "a row of more than 3 pairs"}
    for path, s in seen.items():
        assert classes <= s, f"{path}: {classes - s} never occurs"
    assert {"first pair at entry 63", "a row across a window border", "more than 64 pairs", "more than 128 pairs"} <= seen["wave"]


# ---------------------------------------------------------------------------- the log's reference, and rs_stats
_LIC = {}


def _licence(case):
    if case.name not in _LIC:
        prime, old, rounds = pc.variants(case)[0]
        sys_, info = pc.built(case, prime)
        fl = rsio.flags("O2", rounds, old, log=True)
        n = pc.run_counts(sys_, rounds, old)
        h = rsio.InputHolder(sys_)      # (kept alive over the call: it owns the arrays)
        got = rsio.oracle_run_log(h.inp, fl, threads=8)[3]
        want = pc.expected_stats(case, sys_, info, old)
        _LIC[case.name] = (ds.log_diff(got, n.pop("log")), n, want)
    return _LIC[case.name]


@pytest.mark.parametrize("case", pc.CASES, ids=[c.name for c in pc.CASES])
def test_refcpu_log_is_pyrefs(case):
    """refcpu's substitution log equals pyref's literal one, entry for entry, on every case; and the
    rounds, clusters and largest cluster tests/test_gpu_prelude.py asserts are those of the pyref run."""
    d, counted, want = _licence(case)
    assert d is None, f"refcpu's log differs from pyref's: {d}"
    assert counted == want
