"""GPU parity for rounds 3 and later: the cases of round_cases.py -- whose shapes, list positions and turn
ranks tests/test_round_cases.py proves on the CPU, together with the wrong orders each case would expose
-- run through one engine and compared, array for array and bit for bit, with the CPU oracle
(oracle/refcpu.cpp, equal to pyref on every variant: proved there); then again with the substitution
log on, against refcpu's log.

  pos_*             the order of the rows a round turns linear, by the first position in map[from]: in the
                    initial lists, in lists appended one to five rounds deep (csrc/maplists.hpp), in both,
                    twice, and by cluster before `from`
  turn_*            the rank at which a row turns (d_round_turn), at bn128 and goldilocks, on both sides
                    of the k_frames_wave<1> batch limit
  empty_*, stale_*  rows that come out empty and visits of rows emptied earlier

Every variant (--O2, and --O2round N with N the round in which the rows turn, so that the list order is
the order of the last output rows; both heuristics) goes through load / run / fetch and through
rs_engine_simplify, the streamed result whose rows are rewritten in rounds after the first snapshot went
out.  rs_stats.rounds is round_cases.rounds_model on every run: pyref's count of linear rounds less the
trailing iteration over nothing but stale visits.  pos_appended_depth5 runs twice and the two results are
equal; an ordinary gen_system case runs after every tenth case; the whole list runs once more on an
in-process group of two engines, every rank against the oracle.

That the turn_limit_* rows take both sides of the batch limit is read from the library's own RS_PROF
line of round_apply (`round: N rows, B over a wave batch, T turn`: T rows turned in k_frames_wave<1>,
whose turn k_round_turn computes from turn_list; a row over the batch turns in k_round_fill's
pre-expanded path), in a child process, which is this file run as a program:

    python tests/test_gpu_rounds.py NAME [NAME ...]
"""
import json
import os
import re
import subprocess
import sys

import pytest

import dispatch_shapes as ds
import round_cases as rc
import rsio
import test_gpu_shard_cases as GS
import test_gpu_sharded as SH

R = rsio.R
pytestmark = pytest.mark.gpu
_ENG = None
_COUNT = [0]
_REF = {}


def engine():
    global _ENG
    if _ENG is None:
        import circom_cvm_amd as M
        _ENG = M.Engine(0)
    return _ENG


@pytest.fixture(scope="module", autouse=True)
def _release():
    """The module's engine and the group go when its tests are done (later modules need the device memory)."""
    yield
    global _ENG
    if _ENG is not None:
        _ENG.close()
        _ENG = None
    SH.release_groups()


_RUNS = [(c, pr, old, rd) for c in rc.CASES for pr, old, rd in rc.variants(c)]


def _id(run):
    c, pr, old, rd = run
    return c.name + ("" if pr == "bn128" else "-" + pr) + ("-old" if old else "") + (f"-round{rd}" if rd else "")


def _load_run(inp, fl):
    """-> (arrays, log, rs_stats.rounds) of one load / run / fetch on the module's engine."""
    e = engine()
    e.load(inp)
    e.run(fl)
    out = e.fetch()  # keep the owner alive while the arrays are copied
    return rsio.output_arrays(out.c), rsio.output_log(out.c), int(e.stats().rounds)


def _simplify(inp, fl):
    e = engine()
    out = e.simplify(inp, fl)
    return rsio.output_arrays(out), rsio.output_log(out), int(e.stats().rounds)


def _reference(run, log):
    """(input holder, flags, oracle arrays, oracle log, rounds_model) of a run, computed once."""
    key = (_id(run), log)
    if key not in _REF:
        case, prime, old, rounds = run
        sys_, _ = rc.built(case, prime)
        h = rsio.InputHolder(sys_, prime)
        fl = rsio.flags("O2", rounds, old, log=log)
        ref, _ = rsio.oracle_arrays(h.inp, fl, threads=8)
        ref_log = rsio.oracle_run_log(h.inp, fl, threads=8)[3] if log else []
        _REF[key] = (h, fl, ref, ref_log, rc.rounds_model(sys_, rounds, old))
    return _REF[key]


def _ordinary():
    """After every tenth case: an ordinary random system on the same engine."""
    _COUNT[0] += 1
    if _COUNT[0] % 10:
        return
    h = rsio.InputHolder(rsio.gen_system(300 + _COUNT[0], R.PRIMES["bn128"], n_sig=120, n_rows=200, big_cluster=400 if _COUNT[0] % 20 else 0))
    fl = rsio.flags("O2")
    got, _, _ = _load_run(h.inp, fl)
    assert rsio.diff_output_arrays(got, rsio.oracle_arrays(h.inp, fl)[0]) is None, "the ordinary case after a rounds case"


def _check(run, log):
    case = run[0]
    h, fl, ref, ref_log, want_rounds = _reference(run, log)

    def same(res, what):
        arrays, lg, n_rounds = res
        d = rsio.diff_output_arrays(arrays, ref)
        assert d is None, f"{what}: {d}"
        if log:
            d = ds.log_diff(lg, ref_log)
            assert d is None, f"{what}: log differs: {d}"
        assert n_rounds == want_rounds, f"{what}: rs_stats.rounds"
    first = _load_run(h.inp, fl)
    same(first, "load")
    same(_simplify(h.inp, fl), "rs_engine_simplify")
    if case.name == "pos_appended_depth5":      # the memo of the row lists is per run: the same lists again
        again = _load_run(h.inp, fl)
        same(again, "the second run")
        assert rsio.diff_output_arrays(again[0], first[0]) is None and again[1] == first[1]
    _ordinary()


@pytest.mark.parametrize("run", _RUNS, ids=[_id(r) for r in _RUNS])
def test_rounds(run):
    _check(run, log=False)


@pytest.mark.parametrize("run", _RUNS, ids=[_id(r) for r in _RUNS])
def test_rounds_log(run):
    _check(run, log=True)


@pytest.mark.parametrize("run", _RUNS, ids=[_id(r) for r in _RUNS])
def test_rounds_world2(run):
    """The same runs on a group of two engines, log off and on, both entry points: every rank's arrays,
    log and round count against the single-engine oracle."""
    for log in (False, True):
        h, fl, ref, ref_log, want_rounds = _reference(run, log)
        for path in ("load", "simplify"):
            outs = GS.run_ranks(h.inp, fl, 2, path)
            what = f"{_id(run)} via {path}, log {'on' if log else 'off'}"
            GS.check_ranks(outs, ref, ref_log, what)
            assert [int(st.rounds) for _, _, st in outs] == [want_rounds] * 2, what


def test_limit_rows_take_both_paths():
    """Round 2 of each turn_limit_* case touches its three storage rows; the long row is over the wave
    batch exactly in the +1 cases, and then only the short row turns in k_frames_wave<1>."""
    want = {f"turn_limit_terms{d:+d}": (3, int(d > 0), 2 - int(d > 0)) for d in (-1, 0, 1)}
    want.update({f"turn_limit_entries{d:+d}": (3, d, 2 - d) for d in (0, 1)})
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(want), capture_output=True, text=True, timeout=300,
                       env={**os.environ, "RS_PROF": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    res = {d["case"]: d for d in map(json.loads, r.stdout.strip().splitlines())}
    parts = r.stderr.split("[child] case ")[1:]
    assert [q.split("\n", 1)[0] for q in parts] == list(want)
    for q in parts:
        nm = q.split("\n", 1)[0]
        got = [tuple(map(int, m)) for m in re.findall(r"\[rs-prof\] round: (\d+) rows, (\d+) over a wave batch, (\d+) turn", q)]
        assert got[:1] == [want[nm]], (nm, got)
        assert res[nm]["diff"] is None and res[nm]["rounds"] == 3, res[nm]


def _child(names) -> int:
    import circom_cvm_amd as M
    eng = M.Engine(0)
    try:
        for nm in names:
            sys_, _ = rc.built(rc.BY[nm])
            h = rsio.InputHolder(sys_, "bn128")
            fl = rsio.flags("O2")
            ref, _ = rsio.oracle_arrays(h.inp, fl, threads=8)
            sys.stderr.write(f"[child] case {nm}\n")
            sys.stderr.flush()
            eng.load(h.inp)
            eng.run(fl)
            out = eng.fetch()
            print(json.dumps({"case": nm, "diff": rsio.diff_output_arrays(rsio.output_arrays(out.c), ref), "rounds": int(eng.stats().rounds)}))
    finally:
        eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(_child(sys.argv[1:]))
