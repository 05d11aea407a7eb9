"""The certified cancellations of cancel_cases.py -- whose shapes tests/test_cancel_cases.py proves on
the CPU -- on the GPU: every variant through load / run / fetch and through rs_engine_simplify, each
with the substitution log on and off.  The arrays equal the CPU oracle's bit for bit, the log equals
the oracle's entry for entry (explicit zero keys included: the only output that shows how the
elimination pool stores a right-hand side) and, for inputs under 2,000 rows, pyref's literal log
computed here; the counters are asserted as in tests/test_gpu_dispatch.py."""
import pytest

import cancel_cases as cc
import dispatch_shapes as ds
import rsio

R = rsio.R
pytestmark = pytest.mark.gpu
_ENG = None
PYREF_BELOW = 2000


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


_RUNS = [(c, pr, old, rd) for c in cc.CANCEL_CASES for pr, old, rd in ds.variants(c)]


def _counters(case, st, old, rounds):
    if case.n_rounds is not None:
        assert int(st.rounds) == case.n_rounds[rounds]
    if case.stats is not None:
        assert rounds is None
        want = case.stats(old)
        have = {f: int(getattr(st, f)) for f in want}
        assert have == want


@pytest.mark.parametrize("run", _RUNS, ids=[cc.run_id(r) for r in _RUNS])
def test_cancellation(run):
    case, prime, old, rounds = run
    sys_, _ = case.build(R.PRIMES[prime])
    h = rsio.InputHolder(sys_)
    off, on = rsio.flags("O2", rounds, old), rsio.flags("O2", rounds, old, log=True)
    ref, _ = rsio.oracle_arrays(h.inp, off, threads=8)
    ref_log = rsio.oracle_run_log(h.inp, on, threads=8)[3]
    if len(sys_.rows) < PYREF_BELOW:
        d = ds.log_diff(ref_log, rsio.pyref_log(R.simplification(sys_, rsio.py_flags(on), want_log=True).log))
        assert d is None, f"the oracle's log differs from pyref's: {d}"
    e = engine()
    for fl, want_log in ((on, ref_log), (off, [])):
        e.load(h.inp)
        e.run(fl)
        out = e.fetch()  # keep the owner alive while the arrays are copied
        assert rsio.diff_output_arrays(rsio.output_arrays(out.c), ref) is None
        d = ds.log_diff(rsio.output_log(out.c), want_log)
        assert d is None, f"load / run / fetch, log {'on' if want_log else 'off'}: {d}"
        _counters(case, e.stats(), old, rounds)
        o = e.simplify(h.inp, fl)  # views the engine's buffers until the next call on it
        assert rsio.diff_output_arrays(rsio.output_arrays(o), ref) is None
        d = ds.log_diff(rsio.output_log(o), want_log)
        assert d is None, f"rs_engine_simplify, log {'on' if want_log else 'off'}: {d}"
        _counters(case, e.stats(), old, rounds)
