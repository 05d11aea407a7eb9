"""The substitution log at every kernel dispatch boundary: each case of dispatch_shapes.py at its first
variant, run with the log on and compared entry for entry -- `from`, keys, values (the explicit
zeros the elimination pool keeps, algebra.rs:1279-1294) and order -- with the CPU oracle's log.
tests/test_dispatch_shapes.py licenses that reference: refcpu's log equals pyref's literal log on
each of these (case, variant) pairs, and every family holds a zero-valued non-constant key.  The
arrays must still equal the oracle's (the log flag perturbs nothing) and the counters are the ones
tests/test_gpu_dispatch.py asserts, so the path is still the one the case names."""
import pytest

import dispatch_shapes as ds
import rsio

R = rsio.R
pytestmark = pytest.mark.gpu
_ENG = None


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


@pytest.mark.parametrize("case", ds.CASES, ids=[c.name for c in ds.CASES])
def test_boundary_log(case):
    prime, old, rounds = ds.variants(case)[0]
    sys_, _ = case.build(R.PRIMES[prime])
    h = rsio.InputHolder(sys_)
    fl = rsio.flags("O2", rounds, old, log=True)
    e = engine()
    e.load(h.inp)
    e.run(fl)
    out = e.fetch()  # keep the owner alive while the arrays are copied
    got = rsio.output_arrays(out.c)
    got_log = rsio.output_log(out.c)
    ref_log = rsio.oracle_run_log(h.inp, fl, threads=8)[3]
    d = ds.log_diff(got_log, ref_log)
    assert d is None, f"log differs: {d}"
    ref, _ = rsio.oracle_arrays(h.inp, fl, threads=8)
    assert rsio.diff_output_arrays(got, ref) is None
    st = e.stats()
    if case.n_rounds is not None:
        assert int(st.rounds) == case.n_rounds[rounds]
    if case.stats is not None:
        assert rounds is None
        want = case.stats(old)
        have = {f: int(getattr(st, f)) for f in want}
        assert have == want
