"""The end of a streamed run (rs_engine_simplify on one engine): the fused final layout -- all three
parts per pass, totals read in two copies --, label_to_wire, the row lengths, the jump tables and the
late rows handed to the result stream's thread as each becomes final, and the compact CSR's row
pointers built only when rs_engine_fetch asks for them.  Every result is compared array for array
with the oracle's (label_to_wire included).

Row counts: the smallest of the 60-120 k range.  On the CPU the oracle runs 2 (kind 0), 6 / 4 (kind 5:
bn128 / goldilocks) and 9 (kind 2) rounds at 60 k rows and drops 156 / 177 (kind 5) and 21 (kind 2)
storage rows that a later round emptied; kind 0 empties none at any size up to 120 k (nor at the
benchmark's 10 M), so its empty-row path is covered by the other kinds and by test_tail_all_rows_emptied.
The generator's kind 2 has coefficients the oracle rejects on goldilocks ("invalid input block"):
there the engine must reject the input too and stay usable."""
import functools

import numpy as np
import pytest

import rsio
import circom_cvm_amd as M

pytestmark = pytest.mark.gpu
R = rsio.R
ROWS = 60_000
_ENG = None


def engine():
    global _ENG
    if _ENG is None:
        _ENG = M.Engine(0)
    return _ENG


@pytest.fixture(scope="module", autouse=True)
def _release_engine():
    yield
    global _ENG
    if _ENG is not None:
        _ENG.close()
        _ENG = None


@functools.lru_cache(maxsize=None)
def synth(kind, prime):
    return M.Input.synth(kind, ROWS, 5, prime)


@functools.lru_cache(maxsize=None)
def synth_ref(kind, prime, level, rounds):
    """The oracle's arrays (None: it rejects the input), computed once and only read."""
    try:
        return rsio.oracle_arrays(synth(kind, prime).c, rsio.flags(level, rounds), threads=16)[0]
    except RuntimeError as e:
        assert "invalid input" in str(e)
        return None


def check_layout(o):
    """ABI 8: lengths + jumps give extents inside nnz (tests/test_gpu_hosthost.py's invariants)."""
    n = int(o.n_constraints)
    for q in range(3):
        lc, lay = o.block(q)
        if lay is None:
            continue
        assert not lc.ptr
        lens = np.ctypeslib.as_array(lay[0], shape=(n,)) if n else np.zeros(0, np.uint32)
        jumps = np.ctypeslib.as_array(lay[1], shape=(lay[2],)) if lay[2] else np.zeros(0, np.uint64)
        b = M.abi.row_starts(lens, jumps)
        e = b + (lens & ~np.uint32(M.abi.ROW_JUMP)).astype(np.int64)
        assert (b >= 0).all() and (e <= int(lc.nnz)).all() and lay[2] <= n


def streamed_equals(inp, fl, ref):
    o = engine().simplify(inp, fl)
    check_layout(o)
    d = rsio.diff_output_arrays(rsio.output_arrays(o), ref)
    assert d is None, d


@pytest.mark.parametrize("level,rounds", [("O2", None), ("O2", 1), ("O1", None)])
@pytest.mark.parametrize("prime", ["bn128", "goldilocks"])
@pytest.mark.parametrize("kind", [0, 5, 2])
def test_tail_synth(kind, prime, level, rounds, monkeypatch):
    """Halves, late rows and every snapshot on a small circuit; --O2 round 1 leaves the linear rows as
    C-only extras, --O1 the lconst extras; three calls reuse the regions the first one sized; then
    rs_engine_fetch of the streamed result is the oracle's compact CSR."""
    monkeypatch.setenv("RS_HALVES_MIN", "2")
    inp = synth(kind, prime).c
    fl = rsio.flags(level, rounds)
    ref = synth_ref(kind, prime, level, rounds)
    if ref is None:
        with pytest.raises(M.RsError) as ei:
            engine().simplify(inp, fl)
        assert ei.value.code == -1
        return
    for _ in range(3):
        streamed_equals(inp, fl, ref)
        if level == "O2" and rounds is None:
            assert engine().stats().rounds >= 2
    out = engine().fetch()
    assert not out.c.a_len and not out.c.b_len and not out.c.c_len and out.c.a.ptr
    d = rsio.diff_output_arrays(rsio.output_arrays(out.c), ref)
    assert d is None, d


def _only(sys_, keep):
    return R.System(sys_.p, sys_.max_signal, sys_.n_pub_out, sys_.n_pub_in, sys_.n_priv_in, sys_.forbidden,
                    [c for c in sys_.rows if keep(c)])


def emptied_system(p, k=40):
    """k triples over their own signals: x = 3; x * y = z (linear after round 1: z = 3 y); (z - 3 y) * u = v, a
    storage row until round 2 substitutes z and leaves 0 = v -- every storage row ends empty."""
    rows, s = [], 4
    for _ in range(k):
        x, y, z, u, v = range(s, s + 5)
        s += 5
        rows.append(R.Con({}, {}, {x: 1, 0: p - 3}))
        rows.append(R.Con({x: 1}, {y: 1}, {z: 1}))
        rows.append(R.Con({z: 1, y: p - 3}, {u: 1}, {v: 1}))
    return R.System(p, s, 1, 1, 1, {0, 1, 2}, rows)


def _ab_rows(arrs):
    return int(((np.diff(arrs["a"][0].astype(np.int64)) + np.diff(arrs["b"][0].astype(np.int64))) > 0).sum())


@pytest.mark.parametrize("seed,prime", [(1, "bn128"), (3, "goldilocks")])
def test_tail_random_systems(seed, prime):
    """test_hosthost_random_systems' systems on this module's engine, whole and cut down to their linear
    rows (no non-linear rows: nothing streams) and to their quadratic rows (no linear rows: one round)."""
    p = R.PRIMES[prime]
    for k in range(4):
        whole = rsio.gen_system(100 * seed + k, p, n_sig=120, n_rows=200, big_cluster=400 if k % 2 else 0)
        for sys_ in (whole, _only(whole, lambda c: not c.a and not c.b), _only(whole, lambda c: bool(c.a) or bool(c.b))):
            h = rsio.InputHolder(sys_, prime)
            for fl in (rsio.flags("O2"), rsio.flags("O1"), rsio.flags("O2", rounds=1)):
                ref, _ = rsio.oracle_arrays(h.inp, fl)
                streamed_equals(h.inp, fl, ref)


@pytest.mark.parametrize("prime", ["bn128", "goldilocks"])
def test_tail_all_rows_emptied(prime):
    """Every storage row is emptied by round 2 (n_keep == 0): the reference keeps storage rows after
    round 1 and none at the end; the streamed result and the compact CSR fetched after it agree."""
    h = rsio.InputHolder(emptied_system(R.PRIMES[prime]), prime)
    ref1, _ = rsio.oracle_arrays(h.inp, rsio.flags("O2", rounds=1))
    ref, _ = rsio.oracle_arrays(h.inp, rsio.flags("O2"))
    assert _ab_rows(ref1) > 0 and _ab_rows(ref) == 0
    for _ in range(3):
        streamed_equals(h.inp, rsio.flags("O2"), ref)
    assert engine().stats().rounds >= 2
    d = rsio.diff_output_arrays(rsio.output_arrays(engine().fetch().c), ref)
    assert d is None, d
    streamed_equals(h.inp, rsio.flags("O2", rounds=1), ref1)


def test_tail_early_fetch_ordering(monkeypatch):
    """Calls A, B, A with inputs of different sizes on one engine: each result is right on return (its
    copies were queued before the run ended and are waited for), and a copy of A's taken before B's
    call -- the view is reused -- still equals the oracle's afterwards."""
    monkeypatch.setenv("RS_HALVES_MIN", "2")
    fl = rsio.flags("O2")
    a, ref_a = synth(5, "bn128").c, synth_ref(5, "bn128", "O2", None)
    small = M.Input.synth(0, 20_000, 9, "bn128")
    ref_b, _ = rsio.oracle_arrays(small.c, fl, threads=16)
    o = engine().simplify(a, fl)
    check_layout(o)
    got_a = rsio.output_arrays(o)
    assert rsio.diff_output_arrays(got_a, ref_a) is None
    streamed_equals(small.c, fl, ref_b)
    assert rsio.diff_output_arrays(got_a, ref_a) is None
    streamed_equals(a, fl, ref_a)
    streamed_equals(small.c, fl, ref_b)
    small.free()
