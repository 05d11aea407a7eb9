"""CPU tests of the witness entry points (ABI 13): the .wtns reader and writer against bytes built with
struct, the host projection against the Python one, and the host evaluation rs_check_witness against the
Python evaluator (tests/wtnsio.py: soundness.holds and the log rule of soundness.check_witnesses) -- on
each circuit's own witnesses, on random vectors and on single-value corruptions.  Exact arithmetic in
F_p: no tolerances.  The reader also runs stand-alone under the address and undefined-behaviour
sanitizers on every malformed file and every truncation of a good one."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import rsio
import soundness as S
import wtnsio as W
from circom_cvm_amd import abi

R = rsio.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "rs_simplify.h")


def _flags(key):
    lvl, rd, old = S.FLAG_SETS[key]
    return rsio.flags(lvl, rd, old, log=True)


def _simplified(prime, seed, key):
    """(system, witnesses, pyref result, log, an rs_output holder over it)"""
    sys_, wit = S.small_circuit(prime, seed)
    res = R.simplification(sys_, rsio.py_flags(_flags(key)), want_log=True)
    log = rsio.pyref_log(res.log)
    return sys_, wit, res, log, rsio.OutputHolder(res, sys_.max_signal, log)


def _holder(sys_, prime):
    return rsio.InputHolder(sys_, prime if prime in R.PRIMES else None)


def test_abi_version_and_struct_sizes(tmp_path):
    assert abi.lib().rs_abi_version() >= 13
    assert int(re.search(r"#define RS_ABI_VERSION (\d+)", open(HDR).read()).group(1)) >= 13
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rs_simplify.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(rs_witness), sizeof(rs_witness_report),\n'
                   '  offsetof(rs_witness, n8), offsetof(rs_witness, val), offsetof(rs_witness_report, first_failed),\n'
                   '  offsetof(rs_witness_report, total_ms), (int)RS_WIT_INPUT, (int)RS_WIT_OUTPUT, (int)RS_WIT_LOG, (int)RS_WITC_LOG); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(abi.RsWitness), C.sizeof(abi.RsWitnessReport), abi.RsWitness.n8.offset, abi.RsWitness.val.offset,
                   abi.RsWitnessReport.first_failed.offset, abi.RsWitnessReport.total_ms.offset,
                   abi.WIT_INPUT, abi.WIT_OUTPUT, abi.WIT_LOG, len(abi.WIT_CLASSES) - 1]


@pytest.mark.parametrize("prime", ["bn128", "secq256r1", "goldilocks", "f257"])
def test_write_and_read_roundtrip(tmp_path, prime):
    p = S.PRIMES[prime]
    n8 = 8 if prime in ("goldilocks", "f257") else 32
    assert W.n8_of(p) == n8
    rng = random.Random(3)
    vals = [1, 0, p - 1, p // 2] + [rng.randrange(p) for _ in range(40)]
    want = W.wtns_bytes(vals, p)
    assert len(want) == 12 + 12 + 8 + n8 + 12 + n8 * len(vals)
    path = str(tmp_path / "w.wtns")
    w = W.to_witness(vals, p)
    w.write(path)
    assert open(path, "rb").read() == want
    assert W.parse_wtns(want) == (p, n8, vals)
    for i, data in enumerate((want, W.wtns_bytes(vals, p, order=(2, 1)), W.wtns_bytes(vals, p, between=(7, b"unknown section")),
                              W.wtns_bytes(vals, p, order=(2, 1), between=(0, b"")))):
        q = str(tmp_path / f"r{i}.wtns")
        open(q, "wb").write(data)
        back = abi.Witness.read(q)
        assert back.values() == vals and back.prime() == p and int(back.c.n8) == n8 and int(back.c.n) == len(vals)
        assert int(back.c.prime_id) == (abi.PRIME_IDS[prime] if prime in abi.PRIME_IDS else abi.RS_PRIME_CUSTOM)
        back.write(path)   # what was read, written: the canonical file again
        assert open(path, "rb").read() == want
        back.free()


def test_empty_witness_file(tmp_path):
    p = R.PRIMES["bn128"]
    path = str(tmp_path / "e.wtns")
    open(path, "wb").write(W.wtns_bytes([], p))
    back = abi.Witness.read(path)
    assert back.values() == [] and back.prime() == p


@pytest.mark.parametrize("name", sorted(W.malformed()))
def test_reader_refuses_malformed(tmp_path, name):
    data, word = W.malformed()[name]
    path = str(tmp_path / "bad.wtns")
    open(path, "wb").write(data)
    with pytest.raises(abi.RsError) as e:
        abi.Witness.read(path)
    assert e.value.code == -1
    assert word in str(e.value), str(e.value)


def test_reader_refuses_a_missing_file(tmp_path):
    with pytest.raises(abi.RsError) as e:
        abi.Witness.read(str(tmp_path / "none.wtns"))
    assert e.value.code == -1 and "cannot read" in str(e.value)


@pytest.mark.parametrize("prime", sorted(S.PRIMES))
def test_host_projection(tmp_path, prime):
    """rs_write_wtns(w, out) == the Python projection; nVars of the file is n_wires."""
    p = S.PRIMES[prime]
    path = str(tmp_path / "p.wtns")
    for key in S.FLAG_SETS:
        sys_, wit, res, log, h = _simplified(prime, 1, key)
        assert len(res.signal_map) < sys_.max_signal
        for w in wit[:2]:
            W.to_witness(w, p).write(path, h.out)
            data = open(path, "rb").read()
            assert data == W.wtns_bytes(W.project(w, res.signal_map), p)
            assert W.parse_wtns(data)[2].__len__() == len(res.signal_map) == int(h.out.n_wires)
        # the projected witness satisfies the simplified rows, renumbered by wire
        ww = W.project(wit[0], res.signal_map)
        for c in res.constraints:
            row = R.Con(*({res.signal_map[k]: v for k, v in m.items()} for m in (c.a, c.b, c.c)))
            assert S.holds(row, ww, p)


def test_projection_refusals(tmp_path):
    sys_, wit, res, log, h = _simplified("bn128", 0, "O2")
    p = sys_.p
    path = str(tmp_path / "p.wtns")
    for bad in (wit[0][:-1], wit[0] + [0]):
        with pytest.raises(abi.RsError) as e:
            W.to_witness(bad, p).write(path, h.out)
        assert e.value.code == -1 and "labels" in str(e.value)
    w = W.to_witness(wit[0][:3] + [p] + wit[0][4:], p)
    with pytest.raises(abi.RsError) as e:
        w.write(path)
    assert e.value.code == -1 and "not below the prime" in str(e.value)
    with pytest.raises(abi.RsError):
        W.to_witness(wit[0], p, n8=12).write(path)


@pytest.mark.parametrize("prime", sorted(S.PRIMES))
def test_host_check_against_python(prime):
    p = S.PRIMES[prime]
    rng = random.Random(11)
    for key in S.FLAG_SETS:
        sys_, wit, res, log, h = _simplified(prime, 2, key)
        hin = _holder(sys_, prime)
        classes = R.classify(sys_)

        def both(w):
            want = W.evaluate(p, w, classes, res.constraints, log)
            got = W.triples(abi.check_witness(W.to_witness(w, p), W.ALL, hin.inp, h.out))
            assert got == want, (key, got, want)
            return want

        for w in wit:          # the circuit's own witnesses: nothing fails, every class is counted
            rep = both(w)
            assert all(f == 0 and first == W.NONE for _, f, first in rep.values())
            assert [rep[c][0] for c in W.CLASSES] == [len(x) for x in classes] + [len(res.constraints), len(log)]
        for _ in range(3):     # random vectors: the exact failing sets
            rep = both(W.random_vector(rng, sys_.max_signal, p))
            assert sum(f for _, f, _ in rep.values()) > 0
        if log:                # one eliminated intermediate changed: an input row and a log entry fail
            s = W.eliminated_intermediate(sys_, log, rng)
            for w in wit[:2]:
                bad = list(w)
                bad[s] = (bad[s] + 1 + rng.randrange(p - 1)) % p
                want = W.evaluate(p, bad, classes, res.constraints, log)
                assert sum(want[c][1] for c in W.CLASSES[:4]) > 0 and want["log"][1] > 0   # (the evaluator first)
                assert both(bad) == want


def test_host_check_class_selection():
    sys_, wit, res, log, h = _simplified("bn128", 3, "O2")
    p = sys_.p
    hin = _holder(sys_, "bn128")
    w = W.to_witness(W.random_vector(random.Random(5), sys_.max_signal, p), p)
    full = W.triples(abi.check_witness(w, W.ALL, hin.inp, h.out))
    only_in = W.triples(abi.check_witness(w, abi.WIT_INPUT, hin.inp, None))
    only_out = W.triples(abi.check_witness(w, abi.WIT_OUTPUT, None, h.out))
    only_log = W.triples(abi.check_witness(w, abi.WIT_LOG, None, h.out))
    zero = (0, 0, W.NONE)
    assert [only_in[c] for c in W.CLASSES] == [full[c] for c in W.CLASSES[:4]] + [zero, zero]
    assert [only_out[c] for c in W.CLASSES] == [zero] * 4 + [full["output"], zero]
    assert [only_log[c] for c in W.CLASSES] == [zero] * 5 + [full["log"]]
    d = abi.check_witness(w, W.ALL, hin.inp, h.out).as_dict()
    assert d["output"]["checked"] == len(res.constraints) and d["log"]["checked"] == len(log)
    assert d["nonlinear"]["first_failed"] in (None, full["nonlinear"][2])


@pytest.mark.parametrize("prime", ["bn128", "secq256r1", "goldilocks", "f257"])
def test_host_check_borders_and_edges(prime):
    """The hand-built inputs of the device tests (rows around a chunk border, limb and carry edges): the
    host twin equals the Python evaluator on them too, and about half of the rows fail."""
    p = S.PRIMES[prime]
    cases = [W.border_input(p), W.edge_input(p)] + W.degenerate_inputs(p)
    for raw, w in cases:
        want = W.evaluate(p, w, raw.classes)
        got = W.triples(abi.check_witness(W.to_witness(w, p), abi.WIT_INPUT, raw.inp))
        assert got == want
    raw, w = cases[0]
    want = W.evaluate(p, w, raw.classes)
    for c in ("linear", "nonlinear"):
        assert 0 < want[c][1] < want[c][0]


def test_host_check_refusals():
    sys_, wit, res, log, h = _simplified("bn128", 4, "O2")
    p = sys_.p
    hin = _holder(sys_, "bn128")
    w = wit[0]

    def refused(vals, what=W.ALL, inp=hin.inp, out=h.out, prime=p):
        with pytest.raises(abi.RsError) as e:
            abi.check_witness(W.to_witness(vals, prime), what, inp, out)
        assert e.value.code == -1
        return str(e.value)

    assert "w[0]" in refused([0] + w[1:])
    assert "w[0]" in refused([2] + w[1:])
    assert "not below the prime" in refused(w[:5] + [p] + w[6:])
    assert "labels" in refused(w[:-1])
    assert "labels" in refused(w + [1])
    assert "labels" in refused(w[:-1], abi.WIT_OUTPUT, None)
    assert "prime" in refused([v % R.PRIMES["bls12381"] for v in w], prime=R.PRIMES["bls12381"])
    assert "input" in refused(w, abi.WIT_INPUT, None, None)
    assert "output" in refused(w, abi.WIT_LOG, hin.inp, None)
    raw = W.RawInput(p, 3, linear=[{5: 1}])
    assert "key" in refused([1, 2, 3], abi.WIT_INPUT, raw.inp, None)
    # a refused call leaves the next one intact
    assert W.triples(abi.check_witness(W.to_witness(w, p), W.ALL, hin.inp, h.out)) == W.evaluate(p, w, R.classify(sys_), res.constraints, log)


def test_reader_and_evaluation_under_sanitizers(tmp_path):
    """csrc/wtns_io.hpp in a stand-alone program (tests/wtns_host_check.cpp) under the address and
    undefined-behaviour sanitizers: every malformed file and every truncation of a good file is refused."""
    exe = str(tmp_path / "wtns_host_check")
    csrc = os.path.join(ROOT, "circom_cvm_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, os.path.join(ROOT, "tests", "wtns_host_check.cpp"), os.path.join(csrc, "host_common.cpp"),
                           "-o", exe])
    bad = []
    for name, (data, _) in sorted(W.malformed().items()):
        path = str(tmp_path / (name + ".wtns"))
        open(path, "wb").write(data)
        bad.append(path)
    for prime in ("bn128", "goldilocks"):
        p = S.PRIMES[prime]
        good = str(tmp_path / f"good_{prime}.wtns")
        open(good, "wb").write(W.wtns_bytes([1, p - 1, 0, 12345, p // 3], p))
        r = subprocess.run([exe, str(tmp_path / "scratch.wtns"), good] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
