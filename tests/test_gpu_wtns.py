"""The witness on the device (ABI 13; csrc/witness.hpp): rs_engine_load_witness / rs_engine_load_wtns,
rs_engine_check_witness and rs_engine_write_wtns against the host twins and the Python evaluator of
tests/wtnsio.py.  Exact arithmetic in F_p: every comparison is an equality.  Small inputs: the shapes are
the smallest at which the evaluator takes another path (rows around a chunk of 64 entries and around the
default chunk, rows of many chunks, empty rows and blocks, limb and carry edges)."""
import dataclasses
import os
import random
import subprocess
import threading

import pytest

import rsio
import soundness as S
import wtnsio as W
import circom_cvm_amd as M
import test_gpu_sharded as SH
from circom_cvm_amd import abi

R = rsio.R
pytestmark = pytest.mark.gpu
_ENG = None
PRIMES4 = ["bn128", "goldilocks", "secq256r1", "f257"]
SEEDS = (0, 7, 19)


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


def _holder(sys_, prime):
    return rsio.InputHolder(sys_, prime if prime in R.PRIMES else None)


def _run(h, key, eng=None):
    """Loads and runs; -> (fetched output owner, rows, signal map, log)."""
    e = eng or engine()
    e.load(h.inp)
    e.run(_flags(key))
    out = e.fetch()
    cons, sm, nw, _ = rsio.output_to_py(out.c)
    assert nw == len(sm)
    return out, cons, sm, rsio.output_log(out.c)


def _device(w, p, what, inp=None, eng=None):
    e = eng or engine()
    e.load_witness(W.to_witness(w, p))
    return W.triples(e.check_witness(what, inp))


# --------------------------------------------------------------------------- 1. sound runs hold
@pytest.mark.parametrize("prime", PRIMES4)
def test_sound_runs_hold(prime):
    p = S.PRIMES[prime]
    for seed in SEEDS:
        sys_, wit = S.small_circuit(prime, seed)
        h = _holder(sys_, prime)
        sizes = [len(x) for x in R.classify(sys_)]
        for key in S.FLAG_SETS:
            out, cons, sm, log = _run(h, key)
            for w in wit:
                got = _device(w, p, W.ALL, h.inp)
                assert [got[c][0] for c in W.CLASSES] == sizes + [len(cons), len(log)] == sizes + [int(out.c.n_constraints), int(out.c.n_log)]
                assert all(f == 0 and first == W.NONE for _, f, first in got.values()), (seed, key, got)
                assert got == W.triples(abi.check_witness(W.to_witness(w, p), W.ALL, h.inp, out.c))


def test_sound_process4_holds():
    sys_, wit = S.large_circuit("bn128", 0)
    h = _holder(sys_, "bn128")
    out, cons, sm, log = _run(h, "O2")
    st = engine().stats()
    assert int(st.head_launches) >= 1 and int(st.max_cluster) >= S.p4_threshold()
    for w in wit:
        got = _device(w, sys_.p, W.ALL, h.inp)
        assert all(f == 0 for _, f, _ in got.values()) and got["output"][0] == len(cons) and got["log"][0] == len(log) > 0
        assert got == W.triples(abi.check_witness(W.to_witness(w, sys_.p), W.ALL, h.inp, out.c))


# --------------------------------------------------------------------------- 2. failing sets are exact
@pytest.mark.parametrize("prime", PRIMES4)
def test_failing_sets_are_exact(prime):
    p = S.PRIMES[prime]
    rng = random.Random(23)
    sys_, wit = S.small_circuit(prime, SEEDS[1])
    h = _holder(sys_, prime)
    classes = R.classify(sys_)
    for key in S.FLAG_SETS:
        out, cons, sm, log = _run(h, key)
        for _ in range(2):
            w = W.random_vector(rng, sys_.max_signal, p)
            want = W.evaluate(p, w, classes, cons, log)
            assert sum(f for _, f, _ in want.values()) > 0
            assert _device(w, p, W.ALL, h.inp) == want
        used = set().union(*(S._signals(c, p) for c in cons)) if cons else set()
        only_log = sorted({frm for frm, _ in log} - used)   # eliminated: the log mentions them, no output row does
        picks = [rng.randrange(1, sys_.max_signal)] + ([rng.choice(only_log)] if only_log else [])
        for s in picks:
            w = list(wit[0])
            w[s] = (w[s] + 1 + rng.randrange(p - 1)) % p
            want = W.evaluate(p, w, classes, cons, log)
            if s in only_log:
                assert want["output"][1] == 0 and want["log"][1] > 0
            assert _device(w, p, W.ALL, h.inp) == want
            # each class set on its own
            assert _device(w, p, abi.WIT_LOG)["log"] == want["log"]
            assert _device(w, p, abi.WIT_OUTPUT)["output"] == want["output"]


# --------------------------------------------------------------------------- 3. chunk borders
@pytest.mark.parametrize("chunk", ["64", None])
def test_chunk_borders(monkeypatch, chunk):
    """RS_WIT_INPUT only, on an engine with no result: rows of 0, 1, 63 .. 129 and 5,000 entries in every
    part, rows that begin and end on a chunk border, empty rows and blocks, the constant alone."""
    if chunk is None:
        monkeypatch.delenv("RS_WIT_CHUNK", raising=False)
    else:
        monkeypatch.setenv("RS_WIT_CHUNK", chunk)
    eng = M.Engine(0)
    try:
        for prime in ("bn128", "goldilocks"):
            p = S.PRIMES[prime]
            cases = [W.border_input(p, chunk=64, prime_name=prime)] + W.degenerate_inputs(p)
            if chunk is None and prime == "bn128":
                cases.append(W.border_input(p, seed=4, chunk=1024, prime_name=prime))
            for raw, w in cases:
                want = W.evaluate(p, w, raw.classes)
                assert _device(w, p, abi.WIT_INPUT, raw.inp, eng) == want
            want = W.evaluate(p, cases[0][1], cases[0][0].classes)
            for c in ("linear", "nonlinear"):
                assert 0 < want[c][1] < want[c][0]
    finally:
        eng.close()


# --------------------------------------------------------------------------- 4. limb and carry edges
@pytest.mark.parametrize("prime", ["bn128", "secq256r1", "goldilocks"])
def test_limb_and_carry_edges(monkeypatch, prime):
    p = S.PRIMES[prime]
    raw, w = W.edge_input(p, prime_name=prime)
    want = W.evaluate(p, w, raw.classes)
    assert 0 < want["linear"][1] < want["linear"][0] and 0 < want["nonlinear"][1] < want["nonlinear"][0]
    for chunk in ("64", None):
        if chunk is None:
            monkeypatch.delenv("RS_WIT_CHUNK", raising=False)
        else:
            monkeypatch.setenv("RS_WIT_CHUNK", chunk)
        assert _device(w, p, abi.WIT_INPUT, raw.inp) == want
    assert W.triples(abi.check_witness(W.to_witness(w, p), abi.WIT_INPUT, raw.inp)) == want


# --------------------------------------------------------------------------- 5. projection
def _written_files_agree(tmp_path, sys_, w, sm, n8):
    """write_wtns beside write_r1cs: the .wtns is the Python projection, and every row of the .r1cs holds
    on its values."""
    e = engine()
    p = sys_.p
    wt, r1 = str(tmp_path / "o.wtns"), str(tmp_path / "o.r1cs")
    e.load_witness(W.to_witness(w, p))
    e.write_wtns(wt)
    data = open(wt, "rb").read()
    assert data == W.wtns_bytes(W.project(w, sm), p)
    gp, gn8, vals = W.parse_wtns(data)
    assert (gp, gn8, len(vals)) == (p, n8, len(sm))
    e.write_r1cs(r1)
    got, hdr = R.read_r1cs_bytes(open(r1, "rb").read())
    assert hdr["n_wires"] == len(vals) and got.p == p
    assert all(S.holds(row, vals, p) for row in got.rows)
    return data


@pytest.mark.parametrize("prime", PRIMES4)
def test_projection_files(tmp_path, prime):
    n8 = 8 if prime in ("goldilocks", "f257") else 32
    for seed in SEEDS[:2]:
        sys_, wit = S.small_circuit(prime, seed)
        h = _holder(sys_, prime)
        for key in ("O1", "O2"):
            out, cons, sm, log = _run(h, key)
            assert len(cons) > 0 and len(sm) < sys_.max_signal
            data = _written_files_agree(tmp_path, sys_, wit[0], sm, n8)
            # the host twin writes the same bytes from the fetched result
            host = str(tmp_path / "h.wtns")
            W.to_witness(wit[0], sys_.p).write(host, out.c)
            assert open(host, "rb").read() == data


def test_projection_degenerate_results(tmp_path):
    p = R.PRIMES["bn128"]
    # a zero-row result: the one equality is eliminated
    zero = R.System(p, 5, 1, 1, 2, {0, 1, 2}, [R.Con({}, {}, {3: 5, 4: p - 5})])
    h = _holder(zero, "bn128")
    out, cons, sm, log = _run(h, "O2")
    assert cons == [] and len(log) == 1
    w = [1, 11, 12, 13, 13]
    _written_files_agree(tmp_path, zero, w, sm, 32)
    assert _device(w, p, W.ALL, h.inp) == W.evaluate(p, w, R.classify(zero), cons, log)
    # every signal forbidden: every label is kept, the projection is the witness itself
    sys_, wit = S.small_circuit("bn128", 3)
    allf = dataclasses.replace(sys_, forbidden=set(range(sys_.max_signal)))
    h = _holder(allf, "bn128")
    out, cons, sm, log = _run(h, "O2")
    assert len(sm) == allf.max_signal and log == []
    data = _written_files_agree(tmp_path, allf, wit[0], sm, 32)
    assert data == W.wtns_bytes(wit[0], p)


def test_load_wtns_file(tmp_path):
    """rs_engine_load_wtns of a Python-built file (either section order, an unknown section between) gives
    the reports rs_engine_load_witness gives; n8 = 32 and 8."""
    for prime in ("bn128", "goldilocks", "f257"):
        p = S.PRIMES[prime]
        sys_, wit = S.small_circuit(prime, 5)
        h = _holder(sys_, prime)
        out, cons, sm, log = _run(h, "O2")
        e = engine()
        bad = list(wit[1])
        bad[len(bad) // 2] = (bad[len(bad) // 2] + 1) % p
        for i, w in enumerate((wit[0], bad)):
            want = _device(w, p, W.ALL, h.inp)
            path = str(tmp_path / f"{prime}{i}.wtns")
            open(path, "wb").write(W.wtns_bytes(w, p, order=(2, 1) if i else (1, 2), between=(5, b"xyz") if i else None))
            e.load_wtns(path)
            assert W.triples(e.check_witness(W.ALL, h.inp)) == want == W.evaluate(p, w, R.classify(sys_), cons, log)
            e.write_wtns(str(tmp_path / "o.wtns"))
            assert open(str(tmp_path / "o.wtns"), "rb").read() == W.wtns_bytes(W.project(w, sm), p)


# --------------------------------------------------------------------------- 6. contract
def _small_case_runs(eng):
    sys_, wit = S.small_circuit("f257", 1)
    h = _holder(sys_, "f257")
    out, cons, sm, log = _run(h, "O2", eng)
    S.check(sys_, (cons, sm, int(out.c.no_private_inputs_witness), log), wit)
    assert all(f == 0 for _, f, _ in _device(wit[0], sys_.p, W.ALL, h.inp, eng).values())


def test_contract_refusals(tmp_path):
    p = R.PRIMES["bn128"]
    sys_, wit = S.small_circuit("bn128", 2)
    h = _holder(sys_, "bn128")
    w = wit[0]

    def refused(eng, f, word, after=True):
        with pytest.raises(abi.RsError) as ex:
            f()
        assert ex.value.code == -1 and word in str(ex.value), str(ex.value)
        if after:   # the engine that refused runs a small case correctly
            _small_case_runs(eng)

    fresh = M.Engine(0)   # no input, no result, no witness
    try:
        refused(fresh, lambda: fresh.check_witness(abi.WIT_INPUT, h.inp), "no witness", after=False)
        fresh.load_witness(W.to_witness(w, p))
        refused(fresh, lambda: fresh.check_witness(abi.WIT_OUTPUT), "no result", after=False)
        refused(fresh, lambda: fresh.check_witness(abi.WIT_LOG), "no result", after=False)
        refused(fresh, lambda: fresh.write_wtns(str(tmp_path / "x.wtns")), "no result", after=False)
        assert not (tmp_path / "x.wtns").exists()
        refused(fresh, lambda: fresh.check_witness(abi.WIT_INPUT), "without an input", after=False)
        assert W.triples(fresh.check_witness(abi.WIT_INPUT, h.inp)) == W.evaluate(p, w, R.classify(sys_))
        _small_case_runs(fresh)
    finally:
        fresh.close()
    e = engine()
    # a refused load leaves no witness resident
    refused(e, lambda: e.load_witness(W.to_witness([2] + w[1:], p)), "w[0]", after=False)
    refused(e, lambda: e.check_witness(abi.WIT_INPUT, h.inp), "no witness")
    refused(e, lambda: e.load_witness(W.to_witness(w[:9] + [p] + w[10:], p)), "not below the prime")
    bad = str(tmp_path / "bad.wtns")
    open(bad, "wb").write(W.malformed()["nvars_one_more"][0])
    refused(e, lambda: e.load_wtns(bad), "n8 * nVars")
    open(bad, "wb").write(W.wtns_bytes([1, 2, p], p))
    refused(e, lambda: e.load_wtns(bad), "not below the prime")
    # the log is off
    e.load(h.inp)
    e.run(rsio.flags("O2"))
    e.load_witness(W.to_witness(w, p))
    refused(e, lambda: e.check_witness(abi.WIT_LOG), "log")
    # n one short, one long; another prime
    e.load(h.inp)
    e.run(_flags("O2"))
    for vals in (w[:-1], w + [1]):
        e.load_witness(W.to_witness(vals, p))
        for what in (abi.WIT_INPUT, abi.WIT_OUTPUT, abi.WIT_LOG):
            with pytest.raises(abi.RsError) as ex:
                e.check_witness(what, h.inp)
            assert ex.value.code == -1 and "labels" in str(ex.value)
        with pytest.raises(abi.RsError) as ex:
            e.write_wtns(bad)
        assert ex.value.code == -1 and "labels" in str(ex.value)
    q = R.PRIMES["bls12381"]
    e.load_witness(W.to_witness([v % q for v in w], q))
    for what in (abi.WIT_INPUT, abi.WIT_OUTPUT):
        with pytest.raises(abi.RsError) as ex:
            e.check_witness(what, h.inp)
        assert ex.value.code == -1 and "prime" in str(ex.value)
    _small_case_runs(e)
    # a key at or past the labels; row pointers that decrease
    e.load_witness(W.to_witness([1, 2, 3], p))
    raw = W.RawInput(p, 3, linear=[{1: 1}, {5: 1}], prime_name="bn128")
    refused(e, lambda: e.check_witness(abi.WIT_INPUT, raw.inp), "key")
    e.load_witness(W.to_witness([1, 2, 3], p))
    raw = W.RawInput(p, 3, linear=[{1: 1, 2: 1}, {1: 1}], prime_name="bn128")
    raw.blocks[2].ptr[1] = 4   # [0, 4, 3]: decreasing
    refused(e, lambda: e.check_witness(abi.WIT_INPUT, raw.inp), "row pointers")


def test_result_buffers_do_not_move(tmp_path):
    """A fetch before and after a check and a projection returns identical arrays."""
    sys_, wit = S.small_circuit("bn128", 6)
    h = _holder(sys_, "bn128")
    e = engine()
    for key in ("O2", "O1"):
        out = e.simplify(h.inp, _flags(key))   # the streamed result: the compact rows are built on demand
        before = e.fetch()
        a = rsio.output_arrays(before.c)
        e.load_witness(W.to_witness(wit[0], sys_.p))
        rep = W.triples(e.check_witness(W.ALL, h.inp))
        assert all(f == 0 for _, f, _ in rep.values())
        e.write_wtns(str(tmp_path / "o.wtns"))
        after = e.fetch()
        assert rsio.diff_output_arrays(a, rsio.output_arrays(after.c)) is None
        assert rsio.output_log(before.c) == rsio.output_log(after.c)


def test_report_is_deterministic():
    sys_, wit = S.small_circuit("secq256r1", 8)
    p = sys_.p
    h = _holder(sys_, "secq256r1")
    _run(h, "O2")
    w = W.random_vector(random.Random(1), sys_.max_signal, p)
    first = _device(w, p, W.ALL, h.inp)
    for _ in range(3):
        assert _device(w, p, W.ALL, h.inp) == first


def test_sharded_rank_checks_its_own_copy(tmp_path):
    """Two engines joined in process: after a sharded run each rank checks and projects from its own
    complete copy, with no collective (one rank at a time, from this thread)."""
    engs = SH.group(2)
    sys_, wit = S.small_circuit("bn128", 1)
    p = sys_.p
    h = _holder(sys_, "bn128")
    fl = _flags("O2")
    errs, outs = [None, None], [None, None]

    def work(r):
        try:
            engs[r].load(h.inp)
            engs[r].run(fl)
            outs[r] = engs[r].fetch()
        except Exception as ex:  # noqa: BLE001 -- reported below
            errs[r] = ex

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=240)
        assert not t.is_alive(), "sharded run hung"
    for ex in errs:
        if ex is not None:
            raise ex
    bad = list(wit[1])
    bad[-1] = (bad[-1] + 1) % p
    for r in range(2):
        cons, sm, _, _ = rsio.output_to_py(outs[r].c)
        log = rsio.output_log(outs[r].c)
        for w in (wit[0], bad):
            assert _device(w, p, W.ALL, h.inp, engs[r]) == W.evaluate(p, w, R.classify(sys_), cons, log)
        path = str(tmp_path / f"r{r}.wtns")
        engs[r].write_wtns(path)
        assert open(path, "rb").read() == W.wtns_bytes(W.project(bad, sm), p)


# --------------------------------------------------------------------------- 7. the command-line tool
def test_cli_wtns(tmp_path):
    """circom-simplify --wtns: the engine path and --host-reader write the same .wtns (the Python
    projection) and the same summary line; a witness of another circuit is exit status 3 and no file."""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "circom_cvm_amd", "circom-simplify")
    sys_, wit = S.small_circuit("goldilocks", 4)
    p = sys_.p
    ident = R.Result(sys_.rows, {i: i for i in range(sys_.max_signal)}, sys_.n_priv_in)
    o0 = str(tmp_path / "in.r1cs")
    open(o0, "wb").write(R.result_to_r1cs(sys_, ident))
    good, bad = str(tmp_path / "good.wtns"), str(tmp_path / "bad.wtns")
    open(good, "wb").write(W.wtns_bytes(wit[0], p))
    w = list(wit[0])
    w[-1] = (w[-1] + 1) % p
    open(bad, "wb").write(W.wtns_bytes(w, p))
    res = R.simplification(sys_, rsio.py_flags(_flags("O2")), want_log=True)
    lines = []
    for tag, extra in (("dev", []), ("host", ["--host-reader"])):
        pre = str(tmp_path / tag)
        r = subprocess.run([exe, o0, "--O2", "--simplification_substitution", "--wtns", good, "-o", pre] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines.append([ln for ln in r.stderr.splitlines() if ln.startswith("witness:")])
        assert open(pre + ".wtns", "rb").read() == W.wtns_bytes(W.project(wit[0], res.signal_map), p)
        got, hdr = R.read_r1cs_bytes(open(pre + ".r1cs", "rb").read())
        vals = W.parse_wtns(open(pre + ".wtns", "rb").read())[2]
        assert hdr["n_wires"] == len(vals) and all(S.holds(row, vals, p) for row in got.rows)
    n_in = sum(len(x) for x in R.classify(sys_))
    assert lines[0] == lines[1] == [f"witness: {n_in} input rows, {len(res.constraints)} output rows, {len(res.log)} substitutions hold"]
    for tag, extra in (("dev_bad", []), ("host_bad", ["--host-reader"])):
        pre = str(tmp_path / tag)
        r = subprocess.run([exe, o0, "--O2", "--wtns", bad, "-o", pre] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 3, r.stderr
        assert "not one of this circuit" in r.stderr and not os.path.exists(pre + ".wtns")
