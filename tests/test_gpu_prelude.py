"""GPU parity for everything a run does before its first elimination kernel: the cases of
prelude_cases.py -- whose shapes tests/test_prelude_cases.py proves on the CPU -- run through one engine
and compared, array for array and bit for bit, with the CPU oracle (oracle/refcpu.cpp); then again with
the substitution log on, against refcpu's log (equal to pyref's on every case: proved there).

  eq_*              the equality classes; the unions of 8,200 rows run twice and the two runs agree too
  const_*, border   the constant equalities and what both frames leave of a row
  order_*           the list order inside a cluster on each replay path (lane, wave, host, lane in global
                    memory), on topologies whose result follows the order (proved: order_sensitivity)

The cases marked `simplify` also go through rs_engine_simplify -- the keys-first load settles uncertain
rows and takes the kept eq rows' values from the host input -- as given and with the keys of every eq
row reversed.  rs_stats: rounds, n_clusters, max_cluster are pyref's (proved); cluster_host_ms is
positive on every run that replays a cluster on the host and zero on a run without a linear row.  It
cannot tell the host replay apart on the other runs: by its definition in include/rs_simplify.h it also
holds the time blocked in the clustering's read-backs, which every clustering has.  So that a cluster
is replayed on the host exactly when it is host class and not order-free is read from the library's
own RS_PROF lines, in a child process (test_host_replay_exactly_when_expected).  An ordinary gen_system
case runs after every tenth case."""
import json
import os
import re
import subprocess
import sys

import pytest

import dispatch_shapes as ds
import input_contract as ic
import prelude_cases as pc
import rsio

R = rsio.R
pytestmark = pytest.mark.gpu
_ENG = None
_COUNT = [0]


def engine():
    global _ENG
    if _ENG is None:
        import circom_cvm_amd as M
        _ENG = M.Engine(0)
    return _ENG


@pytest.fixture(scope="module", autouse=True)
def _release_engine():
    """The module's engine goes when its tests are done (later modules need the device memory)."""
    yield
    global _ENG
    if _ENG is not None:
        _ENG.close()
        _ENG = None


_RUNS = [(c, pr, old, rd) for c in pc.CASES for pr, old, rd in pc.variants(c) if (c.name, old) not in pc.DROPPED]


def _id(run):
    c, pr, old, rd = run
    return c.name + ("" if pr == "bn128" else "-" + pr) + ("-old" if old else "") + (f"-round{rd}" if rd else "")


def _load_run(inp, fl):
    """-> (arrays, log, stats) of one load / run / fetch on the module's engine."""
    e = engine()
    e.load(inp)
    e.run(fl)
    out = e.fetch()  # keep the owner alive while the arrays are copied
    return rsio.output_arrays(out.c), rsio.output_log(out.c), e.stats()


def _simplify(inp, fl):
    out = engine().simplify(inp, fl)
    return rsio.output_arrays(out), rsio.output_log(out)


def _ordinary():
    """After every tenth case: an ordinary random system on the same engine."""
    _COUNT[0] += 1
    if _COUNT[0] % 10:
        return
    h = rsio.InputHolder(rsio.gen_system(100 + _COUNT[0], R.PRIMES["bn128"], n_sig=120, n_rows=200, big_cluster=400 if _COUNT[0] % 20 else 0))
    fl = rsio.flags("O2")
    got, _, _ = _load_run(h.inp, fl)
    assert rsio.diff_output_arrays(got, rsio.oracle_arrays(h.inp, fl)[0]) is None, "the ordinary case after a prelude case"


def _check(run, log):
    case, prime, old, rounds = run
    sys_, info = pc.built(case, prime)
    h = rsio.InputHolder(sys_, prime)
    fl = rsio.flags("O2", rounds, old, log=log)
    ref, _ = rsio.oracle_arrays(h.inp, fl, threads=8)
    ref_log = rsio.oracle_run_log(h.inp, fl, threads=8)[3] if log else []
    got, got_log, st = _load_run(h.inp, fl)

    def same(arrays, lg, what):
        d = rsio.diff_output_arrays(arrays, ref)
        assert d is None, f"{what}: {d}"
        if log:
            d = ds.log_diff(lg, ref_log)
            assert d is None, f"{what}: log differs: {d}"
    same(got, got_log, "load")
    want = pc.expected_stats(case, sys_, info, old)
    assert {f: int(getattr(st, f)) for f in want} == want
    if pc.has_host_replay(case, old):
        assert st.cluster_host_ms > 0
    if want["n_clusters"] == 0:
        assert st.cluster_host_ms == 0
    if case.twice:      # the unions of one launch raced differently, if at all: the same arrays again
        again, again_log, _ = _load_run(h.inp, fl)
        same(again, again_log, "the second run")
        assert rsio.diff_output_arrays(again, got) is None and again_log == got_log
    if case.simplify:
        same(*_simplify(h.inp, fl), "rs_engine_simplify")
        g, cnt = ic.permute(h, "reversed", [ic.EQ])
        assert cnt[ic.EQ] == int(h.inp.eq.n_rows) > 0
        same(*_simplify(g.inp, fl), "rs_engine_simplify, eq keys reversed")
        a, lg, _ = _load_run(g.inp, fl)
        same(a, lg, "load, eq keys reversed")
    _ordinary()


@pytest.mark.parametrize("run", _RUNS, ids=[_id(r) for r in _RUNS])
def test_prelude(run):
    _check(run, log=False)


@pytest.mark.parametrize("run", _RUNS, ids=[_id(r) for r in _RUNS])
def test_prelude_log(run):
    _check(run, log=True)


def test_smaller_case_after_the_round2_replay():
    """Round 2 of order_round2 replays a host-class tournament from the staging block round 1's larger
    cluster used; a smaller host-class case on the same engine right after it still equals the oracle."""
    by = {c.name: c for c in pc.CASES}
    for nm in ("order_round2", f"order_tournament_{pc.k.kClMid + 1}", "order_tournament_63"):
        sys_, _ = pc.built(by[nm])
        h = rsio.InputHolder(sys_, "bn128")
        fl = rsio.flags("O2", None, False, log=True)
        got, got_log, _ = _load_run(h.inp, fl)
        assert rsio.diff_output_arrays(got, rsio.oracle_arrays(h.inp, fl, threads=8)[0]) is None, nm
        assert ds.log_diff(got_log, rsio.oracle_run_log(h.inp, fl, threads=8)[3]) is None, nm


def test_host_replay_exactly_when_expected():
    """One case of every replay path, the run with a cluster of each, the round-2 case and an order-free
    host-class cluster, in a child process under RS_PROF: per clustering, the clusters the host
    replayed are exactly the host-class ones that are not order-free, and cluster_host_ms is positive
    whenever there is one."""
    mid = pc.k.kClMid
    want = {"order_tournament_63": [], "order_late_star64_701": [], f"order_tournament_{mid + 1}": [(1, 0)],
            "order_interleaved64_5003": [(1, 0)], f"order_tournament_{pc.k.kClLds + 1}": [], "order_multi": [(1, 0)],
            "order_round2": [(1, 0), (1, 0)], "kClMid_order_free+1": [(1, 1)], "kClMid_ordered+1": [(1, 0)]}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "prelude_child.py")] + list(want), capture_output=True, text=True,
                       timeout=300, env={**os.environ, "RS_PROF": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    res = {d["case"]: d for d in map(json.loads, r.stdout.strip().splitlines())}
    parts = r.stderr.split("[child] case ")[1:]
    assert [q.split("\n", 1)[0] for q in parts] == list(want)
    for q in parts:
        nm = q.split("\n", 1)[0]
        got = [(int(a), int(b)) for a, b in re.findall(r"\[rs-prof\] host replay: (\d+) clusters \((\d+) order-free\)", q)]
        assert got == want[nm], (nm, got)
        assert res[nm]["diff"] is None, res[nm]
        if any(a > b for a, b in want[nm]):
            assert res[nm]["cluster_host_ms"] > 0
