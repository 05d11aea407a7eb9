"""CPU tests of the lift (ABI 14): rs_lift_witness, the host twin, against the Python statement of the
definition (tests/lift.py lift_model) -- on each circuit's own witnesses projected onto the wires, on random
wire vectors, on circuits whose log has a chosen depth, on hand-built logs around the device evaluator's
chunk borders, on the degenerate logs and on every refusal the host can see.  Exact arithmetic in F_p: no
tolerances.  The lift also runs stand-alone under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import lift as LF
import rsio
import soundness as S
import wtnsio as W
from circom_cvm_amd import abi

R = rsio.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "rs_simplify.h")
SEEDS = (0, 7, 19)


def _flags(key):
    lvl, rd, old = S.FLAG_SETS[key]
    return rsio.flags(lvl, rd, old, log=True)


def _simplified(sys_, key):
    """(pyref result, log, an rs_output holder over it)"""
    res = R.simplification(sys_, rsio.py_flags(_flags(key)), want_log=True)
    log = rsio.pyref_log(res.log)
    return res, log, rsio.OutputHolder(res, sys_.max_signal, log)


def _host(v, p, out):
    """rs_lift_witness -> (values, counts)"""
    w, rep = abi.lift_witness(W.to_witness(v, p), out)
    assert int(w.c.n) == int(out.n_labels) and w.prime() == p and int(w.c.n8) == W.n8_of(p)
    assert rep.in_ms == 0 and rep.kernel_ms == 0
    return w.values(), rep.counts()


# --------------------------------------------------------------------------- 1. the ABI
def test_abi_version_and_struct_size(tmp_path):
    assert abi.lib().rs_abi_version() >= 14
    assert int(re.search(r"#define RS_ABI_VERSION (\d+)", open(HDR).read()).group(1)) >= 14
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rs_simplify.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(rs_lift_report), offsetof(rs_lift_report, levels),\n'
                   '  offsetof(rs_lift_report, entries), offsetof(rs_lift_report, total_ms)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(abi.RsLiftReport), abi.RsLiftReport.levels.offset, abi.RsLiftReport.entries.offset,
                   abi.RsLiftReport.total_ms.offset]


# --------------------------------------------------------------------------- 2. lift(project(w)) == w
@pytest.mark.parametrize("prime", ["bn128", "goldilocks", "f257"])
def test_lift_of_the_projection_is_the_witness(prime):
    p = S.PRIMES[prime]
    for seed in SEEDS:
        sys_, wit = S.small_circuit(prime, seed)
        hin = rsio.InputHolder(sys_, prime if prime in R.PRIMES else None)
        for key in S.FLAG_SETS:
            res, log, h = _simplified(sys_, key)
            for w in wit:
                v = W.project(w, res.signal_map)
                m = LF.lift_model(v, res.signal_map, log, sys_.max_signal, p)
                vals, counts = _host(v, p, h.out)
                assert vals == w == m["values"], (seed, key)
                assert counts == LF.model_counts(m, sys_.max_signal, len(res.signal_map))
                assert m["free"] == 0
                rep = W.triples(abi.check_witness(W.to_witness(vals, p), W.ALL, hin.inp, h.out))
                assert all(f == 0 for _, f, _ in rep.values()), (seed, key, rep)


def test_the_last_wins_rule_is_exercised():
    """Over all the runs above rs_lift_witness reports a shadowed entry at least once, and wherever it does
    the log holds that many entries whose `from` a later one has too."""
    total = 0
    for prime in ("bn128", "goldilocks", "f257"):
        p = S.PRIMES[prime]
        for seed in SEEDS:
            sys_, wit = S.small_circuit(prime, seed)
            for key in S.FLAG_SETS:
                res, log, h = _simplified(sys_, key)
                shadowed = _host(W.project(wit[0], res.signal_map), p, h.out)[1][4]
                assert shadowed == len(log) - len({f for f, _ in log})
                total += shadowed
    assert total > 0


def test_rust_structs_match_the_header():
    """integration/rust/src/lib.rs: rs_lift_report and rs_witness_report field for field as the header has
    them (names, types, order), with tests/test_integration.py's parsers."""
    import test_integration as TI
    cs, rs = TI.c_structs(), TI.rust_structs()
    for name in ("rs_lift_report", "rs_witness_report", "rs_witness"):
        assert cs[name] == rs[name], (name, cs[name], rs[name])
    assert [n for n, _ in rs["rs_lift_report"]] == [n for n, _ in abi.RsLiftReport._fields_]


# --------------------------------------------------------------------------- 3. random wire vectors
@pytest.mark.parametrize("prime", ["bn128", "goldilocks", "f257"])
def test_random_wire_vectors(prime):
    p = S.PRIMES[prime]
    rng = random.Random(31)
    for seed in SEEDS:
        sys_, wit = S.small_circuit(prime, seed)
        for key in S.FLAG_SETS:
            res, log, h = _simplified(sys_, key)
            for _ in range(2):
                v = W.random_vector(rng, len(res.signal_map), p)
                m = LF.lift_model(v, res.signal_map, log, sys_.max_signal, p)
                vals, counts = _host(v, p, h.out)
                assert vals == m["values"] and counts == LF.model_counts(m, sys_.max_signal, len(res.signal_map))
                # every owner entry holds on the lift: what fails is shadowed
                failing = {i for i, (frm, to) in enumerate(log) if (vals[frm] - S._dot(to, vals, p)) % p}
                assert failing <= {i for i, lv in enumerate(m["level"]) if lv is None}
                rep = abi.check_witness(W.to_witness(vals, p), abi.WIT_LOG, None, h.out)
                assert int(rep.failed[5]) == len(failing) and int(rep.first_failed[5]) == (min(failing) if failing else W.NONE)


# --------------------------------------------------------------------------- 4. K levels through the simplifier
@pytest.mark.parametrize("K", [1, 2, 3, 10, 40])
def test_tower_has_k_levels(K):
    p = S.PRIMES["bn128"]
    sys_ = LF.tower(p, K)
    res, log, h = _simplified(sys_, "O2")
    assert len(res.constraints) == 1
    v = LF.tower_wire_witness(p, K, 1, res.signal_map, res.constraints, random.Random(K))
    assert all(S.holds(c, [v[res.signal_map[s]] if s in res.signal_map else 0 for s in range(sys_.max_signal)], p) for c in res.constraints)
    m = LF.lift_model(v, res.signal_map, log, sys_.max_signal, p)
    vals, counts = _host(v, p, h.out)
    assert vals == m["values"] and counts == LF.model_counts(m, sys_.max_signal, len(res.signal_map))
    t, c, s, u = LF.tower_ids(K)
    assert m["levels"] == K and counts[5] == K
    assert counts[3] == 2 and m["free_set"] == {u, u + 2}
    assert all(S.holds(row, vals, p) for row in sys_.rows)


# --------------------------------------------------------------------------- 5. hand-built logs
@pytest.mark.parametrize("prime", ["bn128", "secq256r1", "goldilocks"])
def test_hand_built_logs(prime):
    p = S.PRIMES[prime]
    for l2w, log, v in (LF.border_log(p, 64), LF.chain_log(p, 300), LF.wide_log(p, 1000)):
        h = LF.LogHolder(l2w, log)
        m = LF.lift_model(v, h.signal_map, log, len(l2w), p)
        vals, counts = _host(v, p, h.out)
        assert vals == m["values"] and counts == LF.model_counts(m, len(l2w), len(v))
    l2w, log, v = LF.border_log(p, 64)
    m = LF.lift_model(v, LF.LogHolder(l2w, log).signal_map, log, len(l2w), p)
    assert (m["levels"], m["shadowed"], m["free"]) == (3, 2, 3)
    assert LF.lift_model(*_model_args(LF.chain_log(p, 300)), p)["levels"] == 300
    assert LF.lift_model(*_model_args(LF.wide_log(p, 1000)), p)["levels"] == 2


def _model_args(case):
    l2w, log, v = case
    return v, {s: x for s, x in enumerate(l2w) if x >= 0}, log, len(l2w)


# --------------------------------------------------------------------------- 6. degenerate logs
def test_degenerate_logs():
    p = S.PRIMES["bn128"]
    want_counts = [(3, 3, 0, 0, 0, 0, 0), (4, 2, 0, 2, 0, 0, 0), (1, 1, 0, 0, 0, 0, 0), (3, 2, 1, 0, 2, 1, 2), (3, 1, 2, 0, 0, 2, 1)]
    for (l2w, log, v), want in zip(LF.degenerate_logs(p), want_counts):
        h = LF.LogHolder(l2w, log)
        m = LF.lift_model(v, h.signal_map, log, len(l2w), p)
        vals, counts = _host(v, p, h.out)
        assert vals == m["values"] and counts == LF.model_counts(m, len(l2w), len(v)) == want
    # the last entry of a label owns it
    l2w, log, v = LF.degenerate_logs(p)[3]
    assert _host(v, p, LF.LogHolder(l2w, log).out)[0] == [1, 9, (1 - 9) % p]


# --------------------------------------------------------------------------- 7. refusals
def test_host_refusals():
    p = S.PRIMES["f257"]
    cases = LF.refusal_cases(p)
    good = LF.LogHolder(cases["one_long"][0], cases["one_long"][1])
    good_v = [1, 10, 20]
    want = [1, 10, 20, 25, 95, 95, 0]
    for name, (l2w, log, v, word) in cases.items():
        h = LF.LogHolder(l2w, log)
        with pytest.raises(LF.Refused) as e:
            LF.lift_model(v, h.signal_map, log, len(l2w), p)
        assert str(e.value) == word, name
        wp, rep = C.POINTER(abi.RsWitness)(), abi.RsLiftReport()
        vw = W.to_witness(v, p)
        rc = abi.lib().rs_lift_witness(C.byref(h.out), C.byref(vw.c), C.byref(wp), C.byref(rep))
        assert rc == -1 and not wp, name
        assert word in abi.lib().rs_last_error().decode(), (name, abi.lib().rs_last_error())
        assert _host(good_v, p, good.out)[0] == want      # a good call afterwards is intact
    # malformed row pointers
    for i, val in ((0, 1), (1, 5), (4, 6), (4, 1 << 40)):
        h = LF.LogHolder(cases["one_long"][0], cases["one_long"][1])
        h.blk.ptr[i] = val
        LF.expect_refusal(lambda: abi.lift_witness(W.to_witness(good_v, p), h.out), LF.WORDS["ptr"])
    # null arguments
    L = abi.lib()
    wp, rep, vw = C.POINTER(abi.RsWitness)(), abi.RsLiftReport(), W.to_witness(good_v, p)
    for args in ((None, C.byref(vw.c), C.byref(wp), C.byref(rep)), (C.byref(good.out), None, C.byref(wp), C.byref(rep)),
                 (C.byref(good.out), C.byref(vw.c), None, C.byref(rep)), (C.byref(good.out), C.byref(vw.c), C.byref(wp), None)):
        assert L.rs_lift_witness(*args) == -1 and LF.WORDS["null"] in L.rs_last_error().decode() and not wp
    bad = LF.LogHolder(cases["one_long"][0], cases["one_long"][1])
    bad.out.log_from = None
    LF.expect_refusal(lambda: abi.lift_witness(vw, bad.out), LF.WORDS["null"])
    assert _host(good_v, p, good.out)[0] == want


# --------------------------------------------------------------------------- 8. under the sanitizers
def test_lift_under_sanitizers(tmp_path):
    """csrc/wtns_io.hpp's lift in a stand-alone program (tests/lift_host_check.cpp) under the address and
    undefined-behaviour sanitizers: hand-built logs, the 5,000-key row and every refusal."""
    exe = str(tmp_path / "lift_host_check")
    csrc = os.path.join(ROOT, "circom_cvm_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", csrc, os.path.join(ROOT, "tests", "lift_host_check.cpp"), os.path.join(csrc, "host_common.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
