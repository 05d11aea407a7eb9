"""CPU proofs for the certified cancellations of cancel_cases.py (no GPU):
  * the gadgets do what they say (a unit check each, on pyref alone);
  * every case's certificate holds with exact numbers, at each prime the GPU test runs it with: the
    placement, exactly one merge of the wanted kind at the built lengths, the leftover counts, the
    zero keys of s and t, and the vacuity guard (the log with zero keys pruned differs exactly there);
  * refcpu's log equals pyref's literal log on every variant, which licenses refcpu as the GPU test's
    reference on the cases too large for pyref there."""
import pytest

import cancel_cases as cc
import dispatch_shapes as ds
import rsio

R = rsio.R
BN = R.PRIMES["bn128"]


# ---------------------------------------------------------------------------- the gadgets
@pytest.mark.parametrize("kind", ["empty", "const", "partial"])
def test_cancel_pair(kind):
    b = ds.Builder(3, BN)
    glue = b.forbid(1)[0]
    pair = ds.cancel_pair(b, glue, 8, kind)
    r1, r2 = b.rows[-2].c, b.rows[-1].c
    assert len(r1) == len(r2) == 9 and set(r1) == set(r2) and pair["work_plus_rhs"] == 17
    assert [s for s in r1 if s not in b.forb] == [pair["z"]]
    ratio = r2[pair["z"]] * pow(r1[pair["z"]], -1, BN) % BN
    assert ratio not in (0, 1, BN - 1)
    off = [s for s in r1 if r2[s] != r1[s] * ratio % BN]
    assert off == {"empty": [], "const": [0], "partial": [pair["survivor"]]}[kind]
    tr = ds.elimination_trace(list(b.rows), b.forb, BN, False)
    assert tr["merges"] == [(9, 8)]
    assert tr["results"] == [(9, 8) + {"empty": (0, "empty"), "const": (1, "const"), "partial": (1, "forbidden")}[kind]]


def test_trace_results_kinds():
    """A conflict whose merge goes on is "live"; pops, merges and the holder keep their meaning."""
    b = ds.Builder(4, BN)
    glue = b.forbid(1)[0]
    ds.merge_pair(b, glue, 5, 6)
    tr = ds.elimination_trace(list(b.rows), b.forb, BN, False)
    assert tr["pops"] == [6, 5] and tr["merges"] == [(5, 6)] and len(tr["holder"]) == 1
    assert [r[:2] for r in tr["results"]] == tr["merges"] and {r[3] for r in tr["results"]} == {"forbidden"}
    b = ds.Builder(5, BN)
    ds.chain(b, 12)
    cl = R.build_clusters(b.rows, b.nxt)[0]
    tr = ds.elimination_trace(cl, b.forb, BN, False)
    assert tr["results"] and {r[3] for r in tr["results"]} == {"live"}
    assert [r[:2] for r in tr["results"]] == tr["merges"]


def test_dep_sub_defaults_are_the_plain_rows():
    """cancel = 0 and inherit = False consume nothing: the rows of the existing composition cases."""
    def rows(**kw):
        b = ds.Builder(11, BN)
        ds.dep_sub(b, 5, 6, 4, 3, **kw)
        return [r.c for r in b.rows], b.nxt, b.rng.random()
    assert rows() == rows(cancel=0, inherit=False)
    plain, zero = rows()[0], rows(cancel=2, inherit=True)[0]
    assert len(zero) == len(plain) + 1 and [len(r) for r in zero[:-1]] == [len(r) for r in plain]


def test_twin_stars_cancel():
    b = ds.Builder(6, BN)
    x1, x2, ratio = ds.twin_stars(b, 5)
    a = 12345
    b.nonlin({x1: a, x2: a * ratio % BN}, {b.forbid(1)[0]: 1}, {b.forbid(1)[0]: 1})
    res = R.simplification(b.system(), R.Flags(no_rounds=1), want_log=True)
    by = dict(rsio.pyref_log(res.log))
    assert len(by[x1]) == len(by[x2]) == 5 and set(by[x1]) == set(by[x2])
    assert [c for c in res.constraints if c.a] == []          # A vanished: the row turned linear


# ---------------------------------------------------------------------------- the table
def test_case_table_is_complete():
    names = [c.name for c in cc.CANCEL_CASES]
    assert len(set(names)) == len(names)
    want = {f"cancel_{kind}_{where}" for kind in ("empty", "const", "partial") for where in ds.PLACEMENTS + ("giant",)}
    assert len(want) == 15
    for t in ("head", "tail"):
        want |= {f"zero_{t}_{b}" for b in ("len64", "len65", "E+1", "kMergeD+1", "kMergeO+1", "kMergeK+1")}
    want |= {"zero_lane", "zero_p4_head", "zero_giant", "zero_round2", "zero_all_lane", "zero_all_head", "zero_all_tail"}
    want |= set(cc.FRAME_CASE_NAMES)
    assert set(names) == want
    by = {c.name: c for c in ds.CASES}
    for c in cc.CANCEL_CASES:
        assert c.primes == ("bn128", "goldilocks")
        if getattr(c, "twin_of", None):
            assert c.twin_of in by


# ---------------------------------------------------------------------------- certificates
_SHAPES = [(c, pr) for c in cc.CANCEL_CASES for pr in c.primes]


@pytest.mark.parametrize("case,prime", _SHAPES, ids=[f"{c.name}-{pr}" for c, pr in _SHAPES])
def test_certificate(case, prime):
    assert case.olds == (False,)
    sys_, info = case.build(R.PRIMES[prime])
    checks = case.certify(sys_, info, False)
    assert checks
    for rd, want in (case.n_rounds or {}).items():
        checks.append((f"linear rounds at rounds={rd}", ds.linear_rounds(sys_, rd, False), want))
    bad = [(what, got, want) for what, got, want in checks if got != want or type(got) is not type(want)]
    assert not bad, f"{case.name}: (quantity, certificate, intended) {bad}"


# ---------------------------------------------------------------------------- the reference's licence
_RUNS = [(c, pr, old, rd) for c in cc.CANCEL_CASES for pr, old, rd in ds.variants(c)]


@pytest.mark.parametrize("run", _RUNS, ids=[cc.run_id(r) for r in _RUNS])
def test_refcpu_log_is_pyrefs(run):
    case, prime, old, rounds = run
    sys_, _ = case.build(R.PRIMES[prime])
    h = rsio.InputHolder(sys_)
    fl = rsio.flags("O2", rounds, old, log=True)
    res = R.simplification(sys_, rsio.py_flags(fl), want_log=True)
    cons, sm, npiw, log = rsio.oracle_run_log(h.inp, fl, threads=8)
    d = ds.log_diff(log, rsio.pyref_log(res.log))
    assert d is None, f"refcpu's log differs from pyref's: {d}"
    assert rsio.same_result(res, (cons, sm, len(sm), npiw)) is None
