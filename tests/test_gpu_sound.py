"""Soundness of the engine's own output, oracle-free: tests/soundness.py's check (the output rows and
the substitution log say exactly what the input said; the wire map is the stable compaction) run on
what the kernels return with the log on.  No oracle is involved, so a kernel that is wrong shows
even where both oracles are wrong in the same way.  Valid small inputs through paths the suite
already runs; exact equality in F_p."""
import os
import tempfile
import threading

import pytest

import rsio
import soundness as S
import circom_cvm_amd as M
import test_gpu_sharded as SH

R = rsio.R
pytestmark = pytest.mark.gpu
_ENG = None


def engine():
    global _ENG
    if _ENG is None:
        _ENG = M.Engine(0)
    return _ENG


@pytest.fixture(scope="module", autouse=True)
def _release_engine():
    """The module's engine and groups go when its tests are done (later modules need the memory)."""
    yield
    global _ENG
    if _ENG is not None:
        _ENG.close()
        _ENG = None
    SH.release_groups()


def _flags(key):
    lvl, rd, old = S.FLAG_SETS[key]
    return rsio.flags(lvl, rd, old, log=True)


def _result(out):
    cons, sm, nw, npiw = rsio.output_to_py(out)
    assert nw == len(sm)
    return cons, sm, npiw, rsio.output_log(out)


def run_resident(inp, fl):
    e = engine()
    e.load(inp)
    e.run(fl)
    out = e.fetch()  # owns the rs_output while it is read
    return _result(out.c), e.stats()


@pytest.mark.parametrize("prime", sorted(S.PRIMES))
def test_sound_small(prime):
    for seed in range(10):
        sys_, wit = S.small_circuit(prime, seed)
        h = rsio.InputHolder(sys_, prime if prime in R.PRIMES else None)
        for key in S.FLAG_SETS:
            res, _ = run_resident(h.inp, _flags(key))
            S.check(sys_, res, wit)


@pytest.mark.parametrize("key", ["O2", "old"])
def test_sound_process4(key):
    """The large cluster takes the workgroup path (rs_stats: an elimination with a head, its largest
    cluster past the process_4 threshold) under the new and the old heuristics."""
    for prime in ("bn128", "f257"):
        for i in range(2):
            sys_, wit = S.large_circuit(prime, i)
            h = rsio.InputHolder(sys_, prime if prime in R.PRIMES else None)
            res, st = run_resident(h.inp, _flags(key))
            assert int(st.head_launches) >= 1 and int(st.max_cluster) >= S.p4_threshold()
            S.check(sys_, res, wit)


def test_sound_round2():
    prime, seed = S.ROUND2
    sys_, wit = S.small_circuit(prime, seed)
    h = rsio.InputHolder(sys_, prime)
    res, st = run_resident(h.inp, _flags("O2round2"))
    assert int(st.rounds) == 2
    S.check(sys_, res, wit)


@pytest.mark.parametrize("prime", ["bn128", "goldilocks", "secq256r1", "f257"])
def test_sound_hosthost(prime):
    """rs_engine_simplify (host -> host, the streamed ABI 8 layout): its result copy is not fetch's."""
    for seed in range(10):
        sys_, wit = S.small_circuit(prime, seed)
        h = rsio.InputHolder(sys_, prime if prime in R.PRIMES else None)
        for key in S.FLAG_SETS:
            out = engine().simplify(h.inp, _flags(key))
            S.check(sys_, _result(out), wit)


@pytest.mark.parametrize("world", [2, 3])
def test_sound_sharded(world):
    """W engines joined in process: every rank's result is sound."""
    engs = SH.group(world)
    for prime, seed in (("bn128", 1), ("f257", 2), ("goldilocks", 3)):
        sys_, wit = S.small_circuit(prime, seed)
        h = rsio.InputHolder(sys_)
        for key in ("O2", "O2round2", "old"):
            fl = _flags(key)
            got, errs = [None] * world, [None] * world

            def work(r):
                try:
                    engs[r].load(h.inp)
                    engs[r].run(fl)
                    out = engs[r].fetch()
                    got[r] = _result(out.c)
                except Exception as ex:  # noqa: BLE001 -- reported below
                    errs[r] = ex

            th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(world)]
            for t in th:
                t.start()
            for t in th:
                t.join(timeout=240)
                assert not t.is_alive(), "sharded run hung"
            for e in errs:
                if e is not None:
                    raise e
            for r in range(world):
                S.check(sys_, got[r], wit)


def test_sound_written_r1cs():
    """rs_engine_write_r1cs, read back: every row of the file holds on the wire-ordered witness
    w_wire[signal_map[s]] = w[s], and the header's counts are the result's -- the device writer and
    the wire renumbering with no oracle writer involved.  The header's private-input count is the
    input's: the reference writes list.no_private_inputs there (constraint_list/src/r1cs_porting.rs:41),
    not no_private_inputs_witness, which only its log gets (:15) -- so that is what is asserted,
    also on the cases here in which a private input loses its wire."""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.r1cs")
        for prime, seed in (("bn128", 4), ("goldilocks", 5), ("secq256r1", 6)):
            sys_, wit = S.small_circuit(prime, seed)
            h = rsio.InputHolder(sys_, prime)
            for key in ("O1", "O2"):
                (cons, sm, npiw, log), _ = run_resident(h.inp, _flags(key))
                engine().write_r1cs(path)
                with open(path, "rb") as f:
                    data = f.read()
                got, hdr = R.read_r1cs_bytes(data)
                assert got.p == sys_.p and hdr["n_wires"] == len(sm) and hdr["n_cons"] == len(cons)
                assert (got.n_pub_out, got.n_pub_in) == (sys_.n_pub_out, sys_.n_pub_in)
                assert got.n_priv_in == sys_.n_priv_in  # r1cs_porting.rs:41 (see the docstring)
                assert hdr["n_labels"] == sys_.max_signal
                assert len(cons) > 0
                for w in wit:
                    ww = [0] * len(sm)
                    for s, wire in sm.items():
                        ww[wire] = w[s]
                    assert all(S.holds(row, ww, sys_.p) for row in got.rows)
