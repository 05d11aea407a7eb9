"""GPU parity at every kernel dispatch boundary: the cases of dispatch_shapes.py -- whose shapes
tests/test_dispatch_shapes.py proves on the CPU -- run through the engine and compared, array for
array and bit for bit, with the CPU oracle (oracle/refcpu.cpp).  Where rs_stats tells the paths
apart (engine.hip: small_/head_/tail_/giant_launches count the eliminations that had lane-class
clusters / a head / tail groups / giant head clusters; rounds the linear rounds; max_cluster and
n_clusters the clustering), the counters are asserted too.  The round2_* cases put a storage row at
the frames limits in round 2 (k_frames_wave<1>); rs_stats.rounds == 2 shows the round ran.

Three comparisons the cases sit on cannot be told apart by any input: the composition's "few
runs" switch (dead while compose_sort = 1), the giant path's `rl > kGhRhsMax` (dominated by the
row-capacity test beside it) and the fix queue's 64-row count flush (a wave sees one window)."""
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


_RUNS = [(c, pr, old, rd) for c in ds.CASES for pr, old, rd in ds.variants(c)]


def _id(run):
    c, pr, old, rd = run
    return c.name + ("" if pr == "bn128" else "-" + pr) + ("-old" if old else "") + (f"-round{rd}" if rd else "")


@pytest.mark.parametrize("run", _RUNS, ids=[_id(r) for r in _RUNS])
def test_boundary(run):
    case, prime, old, rounds = run
    sys_, _ = case.build(R.PRIMES[prime])
    h = rsio.InputHolder(sys_)
    fl = rsio.flags("O2", rounds, old)
    e = engine()
    e.load(h.inp)
    e.run(fl)
    out = e.fetch()  # keep the owner alive while the arrays are copied
    got = rsio.output_arrays(out.c)
    ref, _ = rsio.oracle_arrays(h.inp, fl, threads=8)
    assert rsio.diff_output_arrays(got, ref) is None
    st = e.stats()
    if case.n_rounds is not None:  # the linear rounds the CPU proof counted: a round-2 case reaches round 2
        assert int(st.rounds) == case.n_rounds[rounds]
    if case.stats is not None:
        assert rounds is None
        want = case.stats(old)
        have = {f: int(getattr(st, f)) for f in want}
        assert have == want
