"""CPU proofs for the cases of round_cases.py (no GPU):
  * every case's certificate holds under both heuristics: pyref's log round by round, the rows that
    turn in the case's round in the reference's order, and the counted (round, rank, position) facts
    read from pyref's own never-pruned map; the table holds exactly the named cases;
  * (rank of the turning substitution, first position in map[from]) -- run.hpp's order key -- is the
    reference's order on every round of every case (asserted inside round_cases.record);
  * sensitivity: which wrong model of that order changes which case's result is CATCHES, exactly; every
    case is caught by the models it is named for and every model by some case;
  * pyref and refcpu agree on the arrays and the log of every variant, which licenses refcpu as the
    reference of tests/test_gpu_rounds.py;
  * rounds_model, the definition of rs_stats.rounds, equals pyref's count of linear rounds on every
    earlier certified family and differs from it on the stale cases.
csrc/maplists.hpp against pyref's lists of these cases is tests/test_oracle.py
test_map_lists_against_pyref."""
import pytest

import cancel_cases as cc
import dispatch_shapes as ds
import prelude_cases as pc
import round_cases as rc
import rsio

R = rsio.R


# ---------------------------------------------------------------------------- certificates
_SHAPES = [(c, old) for c in rc.CASES for old in c.olds]


@pytest.mark.parametrize("case,old", _SHAPES, ids=[f"{c.name}{'-old' if o else ''}" for c, o in _SHAPES])
def test_shape(case, old):
    sys_, info = rc.built(case)
    checks = case.certify(sys_, info, old)
    assert len(checks) >= 4
    bad = [(what, got, want) for what, got, want in checks if got != want or type(got) is not type(want)]
    assert not bad, f"{case.name}: (quantity, certificate, intended) {bad}"
    assert len(sys_.rows) < 100 and all(c["rows"] < ds.P4_MIN for c in ds.cluster_shapes(sys_, old))


def test_case_table_is_exact():
    want = {"pos_initial_r2", "pos_appended_r3", "pos_both", "pos_duplicate", "pos_cluster_vs_from", "turn_second", "turn_cancel",
            "turn_b_first", "turn_dup_signal", "turn_c_only", "turn_rank_over_pos", "empty_same_round", "stale_only", "stale_mixed"}
    want |= {f"pos_appended_depth{d}" for d in (2, 3, 5)}
    want |= {f"turn_limit_terms{d:+d}" for d in (-1, 0, 1)} | {f"turn_limit_entries{d:+d}" for d in (0, 1)}
    assert {c.name for c in rc.CASES} == want == set(rc.CATCHES)
    for c in rc.CASES:
        assert c.olds == (False, True)
        if c.name.startswith(("pos_", "turn_")):     # the truncated run ends with the round's list as its last rows
            assert c.rounds == (None, c.turn_round) and c.models
        assert c.primes == (("bn128", "goldilocks") if c.name.startswith("turn_") else ("bn128",))
    # both sides of the k_frames_wave<1> batch limit (k_round_turn from turn_list | the pre-expanded path)
    assert ds.k.kFwT > 9 and ds.k.kFwE > 9
    # the stale cases are one input with and without the rows that turn in round 3
    five, one = rc.built(rc.BY["stale_mixed"])[0], rc.built(rc.BY["stale_only"])[0]
    assert (len(five.rows), len(one.rows)) == (5, 2)


def test_certificates_hold_at_goldilocks():
    """The turn_* cases also run at goldilocks (d_round_turn multiplies): the same certificates there."""
    for case in rc.CASES:
        for prime in case.primes[1:]:
            sys_, info = rc.built(case, prime)
            bad = [(what, got, want) for what, got, want in case.certify(sys_, info, False) if got != want]
            assert not bad, f"{case.name} at {prime}: {bad}"


# ---------------------------------------------------------------------------- sensitivity
_SENS = {}


def _caught(case):
    """The wrong models under which the case's result (constraints, signal map, log) changes; per rounds
    flag.  record(..., model) hands pyref the turned rows in the model's order instead of its own."""
    if case.name not in _SENS:
        sys_, _ = rc.built(case)
        _SENS[case.name] = {rd: tuple(m for m in rc.MODELS if rc.outcome(rc.record(sys_, rd, model=m)) != rc.outcome(rc.record(sys_, rd)))
                            for rd in case.rounds}
    return _SENS[case.name]


@pytest.mark.parametrize("case", rc.CASES, ids=[c.name for c in rc.CASES])
def test_sensitivity(case):
    got = _caught(case)
    for rd, models in got.items():
        assert models == rc.CATCHES[case.name], f"--O2round {rd}" if rd else "--O2"
        assert set(case.models) <= set(models)


def test_every_wrong_model_is_caught():
    issue_models = {"by_id", "no_appended", "last_occurrence", "one_level", "min_rank", "max_rank", "pos_first"}
    assert issue_models <= set(rc.MODELS)
    for m in rc.MODELS:
        assert [c.name for c in rc.CASES if m in rc.CATCHES[c.name]], f"no case changes under {m}"
        assert [c.name for c in rc.CASES if m in c.models], f"no case is named for {m}"
    # under --O2round N the arrays alone change (the list order is the order of the last rows)
    for case in rc.CASES:
        if case.models:
            sys_, _ = rc.built(case)
            base = rc.outcome(rc.record(sys_, case.turn_round))[:3]
            assert rc.outcome(rc.record(sys_, case.turn_round, model=case.models[0]))[:3] != base, case.name


def test_wrong_model_is_the_engine_order_when_nothing_distinguishes():
    """The harness itself: the "engine" key reproduces pyref (asserted in record on every call), and a
    wrong model on a case it is not listed for leaves the result as it is."""
    case = rc.BY["turn_b_first"]
    sys_, _ = rc.built(case)
    base = rc.outcome(rc.record(sys_))
    plain = R.simplification(sys_, R.Flags(), want_log=True)
    assert base[3] == rsio.pyref_log(plain.log) and base[0] == [(c.a, c.b, c.c) for c in plain.constraints]
    assert rc.outcome(rc.record(sys_, model="by_id")) == base


# ---------------------------------------------------------------------------- the reference's licence
_RUNS = [(c, pr, old, rd) for c in rc.CASES for pr, old, rd in rc.variants(c)]


def run_id(run):
    c, pr, old, rd = run
    return c.name + ("" if pr == "bn128" else "-" + pr) + ("-old" if old else "") + (f"-round{rd}" if rd else "")


@pytest.mark.parametrize("run", _RUNS, ids=[run_id(r) for r in _RUNS])
def test_refcpu_is_pyref(run):
    case, prime, old, rounds = run
    sys_, _ = rc.built(case, prime)
    h = rsio.InputHolder(sys_, prime)
    fl = rsio.flags("O2", rounds, old, log=True)
    res = R.simplification(sys_, rsio.py_flags(fl), want_log=True)
    cons, sm, npiw, log = rsio.oracle_run_log(h.inp, fl, threads=8)
    d = ds.log_diff(log, rsio.pyref_log(res.log))
    assert d is None, f"refcpu's log differs from pyref's: {d}"
    assert rsio.same_result(res, (cons, sm, len(sm), npiw)) is None
    assert rsio.oracle_run(h.inp, fl, threads=1)[2] == ds.linear_rounds(sys_, rounds, old)


# ---------------------------------------------------------------------------- rounds_model
def test_rounds_model_on_the_stale_cases():
    """pyref loops once more over a list that holds nothing but rows an earlier round emptied; the model
    does not count that iteration.  A row that comes out empty in the round that turns it still counts."""
    got = {}
    for nm in ("stale_only", "stale_mixed", "empty_same_round"):
        sys_, _ = rc.built(rc.BY[nm])
        for old in (False, True):
            got[nm, old] = (ds.linear_rounds(sys_, None, old), rc.rounds_model(sys_, None, old))
    assert got == {("stale_only", False): (4, 3), ("stale_only", True): (4, 3), ("stale_mixed", False): (5, 4), ("stale_mixed", True): (5, 4),
                   ("empty_same_round", False): (4, 4), ("empty_same_round", True): (4, 4)}
    # truncation: --O2round N ends the loop before the stale iteration, so there is nothing to take off
    sys_, _ = rc.built(rc.BY["stale_mixed"])
    assert [(ds.linear_rounds(sys_, n, False), rc.rounds_model(sys_, n)) for n in (1, 2, 3, 4, 5, 6)] == \
        [(1, 1), (2, 2), (3, 3), (4, 4), (5, 4), (5, 4)]


_EARLIER = [(fam, c) for fam, cases in (("dispatch", ds.CASES), ("prelude", pc.CASES), ("cancel", cc.CANCEL_CASES)) for c in cases]


@pytest.mark.parametrize("fam,case", _EARLIER, ids=[f"{f}-{c.name}" for f, c in _EARLIER])
def test_rounds_model_is_pyrefs_count_on_the_earlier_families(fam, case):
    """No earlier certified case ends on a stale list: on each (at its first variant, the run its own CPU
    proof makes) the model equals pyref's count, which is what those families' GPU tests assert."""
    prime, old, rounds = ds.variants(case)[0]
    sys_ = (pc.built(case, prime) if fam == "prelude" else case.build(R.PRIMES[prime]))[0]
    rec = rc.record(sys_, rounds, old)
    assert rc.rounds_model(sys_, rec=rec) == rc.pyref_rounds(rec)
    assert not any(c["all_stale"] for c in rec["calls"])
