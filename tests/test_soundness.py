"""CPU soundness tests: tests/soundness.py's oracle-free check (output rows + substitution log say
exactly what the input said; the wire map is the stable compaction) on both oracles -- the literal
Python restatement (oracle/pyref.py) and the C++ one (oracle/refcpu.cpp, log on) -- over satisfiable
gen_circuit systems on every prime and flag set, on the reference-held docs vector and the golden
fixtures; coverage certificates that keep the suite from passing vacuously; the checker's self-test
(seven mutations of a result, each of which a named check must flag); and the census of
rsio.gen_system's inconsistent seeds.  Everywhere the tolerance is exact equality in F_p."""
import copy
import json
import os

import pytest

import dispatch_shapes as ds
import rsio
import soundness as S
from test_oracle import G, GOLD, _fixture_system, _fixtures

R = rsio.R


def _pyref(sys_, key):
    lvl, rd, old = S.FLAG_SETS[key]
    return R.simplification(sys_, G.flags_of(lvl, rd, old), want_log=True)


def _refcpu(sys_, key, threads=2):
    lvl, rd, old = S.FLAG_SETS[key]
    h = rsio.InputHolder(sys_)  # keeps the arrays behind the RsInput alive
    return rsio.oracle_run_log(h.inp, rsio.flags(lvl, rd, old), threads)


# ------------------------------------------------------------------ both oracles, all six checks
@pytest.mark.parametrize("prime", sorted(S.PRIMES))
def test_oracles_sound_small(prime):
    for seed in range(30):
        sys_, wit = S.small_circuit(prime, seed)
        for key in S.FLAG_SETS:
            S.check(sys_, _pyref(sys_, key), wit)
            S.check(sys_, _refcpu(sys_, key, 1 + seed % 3), wit)


@pytest.mark.parametrize("key", ["O2", "old"])
def test_oracles_sound_large_cluster(key):
    for i in range(2):
        sys_, wit = S.large_circuit("bn128", i)
        S.check(sys_, _pyref(sys_, key), wit)
        S.check(sys_, _refcpu(sys_, key, 4), wit)


# ------------------------------------------------------------------ reference-held vectors
def test_docs_basic_sound():
    """basic.circom (tests/golden/docs_basic.json, the one vector the reference's docs hold): the
    docs' own --O1 / --O2 constraints, wire numbers and substitutions pass every check."""
    sys_ = G.docs_system()
    for lvl in ("O1", "O2"):
        res = R.simplification(sys_, G.flags_of(lvl), want_log=True)
        assert R.to_json_constraints(res.constraints, res.signal_map) == G.DOCS["constraints"][lvl]
        log = [(int(f), {int(k): int(v) for k, v in to.items()}) for f, to in G.DOCS["substitutions"][lvl].items()]
        S.check(sys_, (res.constraints, res.signal_map, res.no_private_inputs_witness, log))


GOLDEN_LEFT_OUT = (2, 14)  # (fixture vectors with a contradicting log, all): oracle_bn128.json at --O1 and --O2


def test_golden_fixtures_sound():
    """Every tests/golden/oracle_*.json vector (a gen_system system with its pinned result) whose log
    defines no signal twice with different right-hand sides passes every check.  gen_system makes
    contradicting constant equalities on purpose (x = 3 and x = 5); the reference keeps one
    substitution per signal (build_encoded_fast_substitutions, simplification_utils.rs:520-527: a
    HashMap insert per substitution, the last one wins), so such a system loses the other equation
    and is left out here.  The count left out is pinned and may not exceed half."""
    total, left_out = 0, []
    for fname in _fixtures():
        with open(os.path.join(GOLD, fname)) as f:
            fx = json.load(f)
        sys_ = _fixture_system(fx)
        for ex in fx["expected"]:
            total += 1
            log = R.simplification(sys_, G.flags_of(ex["level"], ex["rounds"], ex["old"]), want_log=True).log
            if not S.consistent_log(sys_, log):
                left_out.append((fname, ex["level"], ex["rounds"], ex["old"]))
                continue
            cons = G.rows_from_json(ex["constraints"])
            sm = {int(k): v for k, v in ex["signal_map"].items()}
            S.check(sys_, (cons, sm, ex["no_private_inputs_witness"], log))
    assert 2 * len(left_out) <= total, (len(left_out), total)
    assert (len(left_out), total) == GOLDEN_LEFT_OUT, left_out



# ------------------------------------------------------------------ coverage certificates
def test_coverage_certificates(monkeypatch):
    """What the cases above reach, asserted with pyref so the suite cannot pass vacuously."""
    sizes = {3: [], 4: []}
    p3, p4 = R.substitution_process_3, R.substitution_process_4
    monkeypatch.setattr(R, "substitution_process_3", lambda f, c, h, p: (sizes[3].append(len(c)), p3(f, c, h, p))[1])
    monkeypatch.setattr(R, "substitution_process_4", lambda f, c, h, p: (sizes[4].append(len(c)), p4(f, c, h, p))[1])
    T = S.p4_threshold()
    assert T == ds.P4_MIN  # the reference's rule as test_dispatch_shapes.py states it
    for i in range(2):
        sys_, _ = S.large_circuit("bn128", i)
        for key, proc in (("O2", 4), ("old", 3)):
            sizes[3].clear(), sizes[4].clear()
            _pyref(sys_, key)
            assert max(sizes[proc]) >= T, "the large cluster goes through process_%d" % proc
            assert key != "old" or not sizes[4]
    # the certified round-2 case: round 2's linear_simplification logs substitutions
    prime, seed = S.ROUND2
    sys_, _ = S.small_circuit(prime, seed)
    assert len(_pyref(sys_, "O2round2").log) > len(_pyref(sys_, "O2round1").log)
    seen = dict(empty=0, turns_linear=0, repeated=0, private_gone=0, constant_def=0, process_3=0)
    for prime in ("bn128", "f257"):
        for seed in range(30):
            sys_, _ = S.small_circuit(prime, seed)
            sizes[3].clear()
            cons, sm, npiw, log = S.as_result(_pyref(sys_, "O2"))
            seen["process_3"] += bool(sizes[3])
            # every log entry uses up one input row: more rows gone than entries = a row became empty
            seen["empty"] += len(sys_.rows) - len(cons) - len(log) > 0
            seen["turns_linear"] += sum(1 for c in cons if c.a or c.b) < sum(1 for c in sys_.rows if c.a or c.b)
            seen["repeated"] += len({f for f, _ in log}) < len(log)
            seen["private_gone"] += npiw < sys_.n_priv_in
            seen["constant_def"] += any(set(d) <= {0} for d in S.resolve_log(sys_, log)[0].values())
    assert all(seen.values()), seen


# ------------------------------------------------------------------ the checker's self-test
def _mutations(sys_, res):
    """(name, mutated result, the checks of which one must flag it)."""
    p = sys_.p
    cons, sm, npiw, log = S.as_result(res)
    fresh = lambda: (copy.deepcopy(cons), dict(sm), npiw, copy.deepcopy(log))  # noqa: E731
    out = []
    c, s, n, l = fresh()
    k = next(iter(c[0].c))
    c[0].c[k] = (c[0].c[k] + 1) % p
    out.append(("one coefficient of one output row + 1", (c, s, n, l), {"forward", "reverse"}))
    c, s, n, l = fresh()
    i = next(i for i, x in enumerate(c) if x.a and x.b and x.c)
    c[i].c = {k: -v % p for k, v in c[i].c.items()}
    out.append(("the sign of a non-linear row's C side flipped", (c, s, n, l), {"forward", "reverse"}))
    c, s, n, l = fresh()
    polys = [S.row_poly(x, {}, p) for x in c]
    full = S.rank(polys, p)
    i = next(i for i in range(len(c)) if S.rank(polys[:i] + polys[i + 1:], p) < full)
    del c[i]
    out.append(("one output row deleted (the first whose removal lowers the rank)", (c, s, n, l), {"forward"}))
    c, s, n, l = fresh()
    del l[len(l) // 2]
    out.append(("one log entry deleted", (c, s, n, l), {"no leak", "forward"}))
    c, s, n, l = fresh()
    i = next(i for i, (_, to) in enumerate(l) if to)
    k = next(iter(l[i][1]))
    l[i][1][k] = (l[i][1][k] + 1) % p
    out.append(("one log coefficient + 1", (c, s, n, l), {"forward", "witnesses"}))
    c, s, n, l = fresh()
    a, b = sorted(s)[1:3]
    s[a], s[b] = s[b], s[a]
    out.append(("two wires swapped", (c, s, n, l), {"witness map"}))
    c, s, n, l = fresh()
    out.append(("no_private_inputs_witness + 1", (c, s, n + 1, l), {"witness map"}))
    return out


@pytest.mark.parametrize("prime", ["bn128", "f257"])
def test_checker_flags_every_mutation(prime):
    sys_, wit = S.small_circuit(prime, 7)
    res = _pyref(sys_, "O2")
    assert S.failing_checks(sys_, res, wit) == {}
    muts = _mutations(sys_, res)
    assert len(muts) == 7
    for name, bad, want in muts:
        flagged = set(S.failing_checks(sys_, bad, wit))
        assert flagged & want, f"{name}: flagged {sorted(flagged)}, wanted one of {sorted(want)}"


def test_checker_flags_cycle_and_forbidden():
    sys_, wit = S.small_circuit("f257", 3)
    cons, sm, npiw, log = S.as_result(_pyref(sys_, "O2"))
    (f0, to0) = next((f, to) for f, to in log if any(k for k in to))
    k0 = next(k for k in to0 if k)
    with pytest.raises(S.Unsound, match="cycle"):
        S.check(sys_, (cons, sm, npiw, [(f0, {k0: 1}), (k0, {f0: 1})]))
    with pytest.raises(S.Unsound, match="forbidden"):
        S.check(sys_, (cons, sm, npiw, log + [(1, {0: 1})]))


# ------------------------------------------------------------------ gen_system's inconsistent seeds
CENSUS = (252, 2, 800)  # (contradicting logs, stale wires, runs)


def test_gen_system_census():
    """Over the seeds test_gpu_parity.py's test_random_small uses: how many (system, level) runs substitute a
    signal twice with different right-hand sides (gen_system's deliberate duplicate constant
    equalities: x = 3 and x = 5).  On all the others the result is equivalent to the input; on
    those the reference keeps one substitution per signal and the equivalence may be lost.

    stale_wire counts the consistent runs on which the witness-map check, and nothing else, finds a
    wire too many: goldilocks seed 8 at --O2 and --O2round 2, signal 8.  It sits in two non-linear
    rows after round 1, round 2 substitutes 0 for a factor of each, the rows turn linear without it,
    and the reference's non_linear_map (constraint_simplification.rs:603-609, filled further at :637,
    never pruned) still has its key when rebuild_witness asks contains_key (:113).  The reference
    keeps that wire; the check is stricter than the reference there, so the count is pinned, not 0."""
    inconsistent = stale_wire = total = 0
    for p in [257, 97, R.PRIMES["bn128"], R.PRIMES["secq256r1"], R.PRIMES["goldilocks"]]:
        for seed in range(40):
            sys_ = rsio.gen_system(seed, p, n_sig=40 + seed % 50, n_rows=60 + seed % 80)
            for lvl, rd in (("O1", None), ("O2", None), ("O2", 1), ("O2", 2)):
                res = R.simplification(sys_, G.flags_of(lvl, rd), want_log=True)
                total += 1
                if not S.consistent_log(sys_, res.log):
                    inconsistent += 1
                    continue
                bad = S.failing_checks(sys_, res)
                assert set(bad) <= {"witness map"}, (p, seed, lvl, rd, bad)  # equivalence holds
                if bad:
                    assert "too many, [] missing" in bad["witness map"], bad
                    stale_wire += 1
    assert (inconsistent, stale_wire, total) == CENSUS
