"""The lift on the device (ABI 14; csrc/lift.hpp): rs_engine_lift_witness, rs_lift_witness_device,
rs_engine_fetch_witness and rs_engine_write_wtns_resident against the host twin rs_lift_witness and the
Python statement of the definition (tests/lift.py).  Exact arithmetic in F_p: every comparison is an
equality.  Small inputs: the shapes are the smallest at which the device path takes another way (rows around
a chunk of 64 entries and around the default chunk, rows of many chunks at levels 0, 1 and 2, more rows in
a level than one 256-lane pass, thousands of levels, the empty log)."""
import ctypes as C
import random
import threading

import pytest

import lift as LF
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
    """Loads and runs with the log on; -> (fetched output owner, signal map, log)."""
    e = eng or engine()
    e.load(h.inp)
    e.run(_flags(key))
    out = e.fetch()
    cons, sm, nw, _ = rsio.output_to_py(out.c)
    assert nw == len(sm)
    return out, sm, rsio.output_log(out.c)


def _lift(v, p, eng=None):
    """Loads the wire witness, lifts it on the engine; -> (values, counts)."""
    e = eng or engine()
    e.load_witness(W.to_witness(v, p))
    rep = e.lift_witness()
    assert rep.total_ms > 0
    return e.fetch_witness().values(), rep.counts()


def _host(v, p, out):
    w, rep = abi.lift_witness(W.to_witness(v, p), out)
    return w.values(), rep.counts()


def _one_shot(v, p, out):
    w, rep = abi.lift_witness_device(W.to_witness(v, p), out)
    assert int(w.c.n) == int(out.n_labels) and w.prime() == p and int(w.c.n8) == W.n8_of(p)
    return w.values(), rep.counts()


# --------------------------------------------------------------------------- 1. real runs
def _real_run(tmp_path, sys_, wit, h, key):
    p = sys_.p
    e = engine()
    out, sm, log = _run(h, key)
    wires, o0 = str(tmp_path / "wires.wtns"), str(tmp_path / "o0.wtns")
    for w in wit:
        v = W.project(w, sm)
        vals, counts = _lift(v, p)
        assert vals == w
        assert (vals, counts) == _host(v, p, out.c)
        rep = W.triples(e.check_witness(W.ALL, h.inp))
        assert all(f == 0 for _, f, _ in rep.values()), (key, rep)
        e.write_wtns(wires)                 # the projection of the lifted witness: the wire file again
        assert open(wires, "rb").read() == W.wtns_bytes(v, p)
        e.write_wtns_resident(o0)
        host = str(tmp_path / "host.wtns")
        W.to_witness(w, p).write(host)
        assert open(o0, "rb").read() == open(host, "rb").read() == W.wtns_bytes(w, p)
    return log


@pytest.mark.parametrize("prime", PRIMES4)
def test_real_runs(tmp_path, prime):
    for seed in SEEDS:
        sys_, wit = S.small_circuit(prime, seed)
        h = _holder(sys_, prime)
        for key in S.FLAG_SETS:
            _real_run(tmp_path, sys_, wit, h, key)


def test_real_run_process4(tmp_path):
    sys_, wit = S.large_circuit("bn128", 0)
    h = _holder(sys_, "bn128")
    log = _real_run(tmp_path, sys_, wit, h, "O2")
    st = engine().stats()
    assert int(st.head_launches) >= 1 and int(st.max_cluster) >= S.p4_threshold() and len(log) > 0


# --------------------------------------------------------------------------- 2. levels through the simplifier
@pytest.mark.parametrize("prime,K,copies", [("bn128", 40, 1), ("goldilocks", 40, 1), ("bn128", 6, 300)])
def test_levels_through_the_simplifier(prime, K, copies):
    p = S.PRIMES[prime]
    sys_ = LF.tower(p, K, copies)
    h = _holder(sys_, prime)
    out, sm, log = _run(h, "O2")
    v = W.random_vector(random.Random(K + copies), len(sm), p)
    m = LF.lift_model(v, sm, log, sys_.max_signal, p)
    assert m["levels"] == K                         # from the fetched log
    per_level = [sum(1 for lv in m["level"] if lv == l) for l in range(K)]
    assert min(per_level) >= copies
    vals, counts = _lift(v, p)
    assert vals == m["values"] and counts == LF.model_counts(m, sys_.max_signal, len(sm))
    assert (vals, counts) == _host(v, p, out.c)
    assert counts[5] == K and counts[3] == 2 * copies


# --------------------------------------------------------------------------- 3. hand-built logs, one-shot
def _check_case(case, p):
    l2w, log, v = case
    h = LF.LogHolder(l2w, log)
    want = _host(v, p, h.out)
    assert _one_shot(v, p, h.out) == want
    return want


def _border_shape(log, sm, L, v, p, chunk):
    """What the border log must really hold for a chunk of `chunk` entries."""
    m = LF.lift_model(v, sm, log, L, p)
    lens = {(lv, len(to)) for (f, to), lv in zip(log, m["level"]) if lv is not None}
    assert any(lv >= 1 and n > 2 * chunk for lv, n in lens)
    for lv in (0, 1, 2):
        assert {(lv, chunk - 1), (lv, chunk), (lv, chunk + 1), (lv, 5000)} <= lens
    assert m["levels"] == 3 and m["shadowed"] == 2 and m["free"] == 3
    assert any(c == 0 for (f, to), lv in zip(log, m["level"]) if lv for k, c in to.items() if k >= 5200)   # a zero coefficient on an owned key


@pytest.mark.parametrize("chunk", ["64", None])
@pytest.mark.parametrize("prime", ["bn128", "secq256r1", "goldilocks"])
def test_border_logs(monkeypatch, prime, chunk):
    if chunk is None:
        monkeypatch.delenv("RS_WIT_CHUNK", raising=False)
    else:
        monkeypatch.setenv("RS_WIT_CHUNK", chunk)
    p = S.PRIMES[prime]
    sizes = [64] if chunk else [64, 1024]
    for size in sizes:
        l2w, log, v = LF.border_log(p, size)
        _border_shape(log, {s: x for s, x in enumerate(l2w) if x >= 0}, len(l2w), v, p, size)
        vals, counts = _check_case((l2w, log, v), p)
        assert counts[5] == 3


def test_chain_of_3000_levels():
    p = S.PRIMES["bn128"]
    vals, counts = _check_case(LF.chain_log(p, 3000), p)
    assert counts[5] == 3000 and counts[2] == 3000


def test_wide_levels():
    p = S.PRIMES["goldilocks"]
    vals, counts = _check_case(LF.wide_log(p, 70000), p)
    assert counts[2:] == (140000, 0, 0, 2, 420000)


@pytest.mark.parametrize("prime", ["bn128", "secq256r1", "goldilocks"])
def test_degenerate_logs(prime):
    p = S.PRIMES[prime]
    for case in LF.degenerate_logs(p):
        _check_case(case, p)


# --------------------------------------------------------------------------- 4. refusals
def test_one_shot_refusals():
    p = S.PRIMES["f257"]
    cases = LF.refusal_cases(p)
    good = LF.LogHolder(cases["one_long"][0], cases["one_long"][1])
    for name, (l2w, log, v, word) in cases.items():
        h = LF.LogHolder(l2w, log)
        wp, rep = C.POINTER(abi.RsWitness)(), abi.RsLiftReport()
        rc = abi.lib().rs_lift_witness_device(0, C.byref(h.out), C.byref(W.to_witness(v, p).c), C.byref(wp), C.byref(rep))
        assert rc == -1 and not wp, name
        msg = abi.lib().rs_last_error().decode()
        assert word in msg, (name, msg)
        if name not in ("w0_is_2", "w0_is_0", "value_is_p"):      # (those two causes are the load's: "witness: ...")
            assert msg.startswith("rs_lift_witness_device:"), (name, msg)   # the entry point the caller used
    for i, val in ((0, 1), (1, 5), (4, 6), (4, 1 << 40)):   # (the verdict is read before any kernel reads a row)
        h = LF.LogHolder(cases["one_long"][0], cases["one_long"][1])
        h.blk.ptr[i] = val
        LF.expect_refusal(lambda: abi.lift_witness_device(W.to_witness([1, 10, 20], p), h.out), LF.WORDS["ptr"])
    LF.expect_refusal(lambda: abi.check(abi.lib().rs_lift_witness_device(0, None, None, None, None)), LF.WORDS["null"])
    assert _one_shot([1, 10, 20], p, good.out)[0] == [1, 10, 20, 25, 95, 95, 0]


def test_engine_refusals():
    prime = "bn128"
    p = S.PRIMES[prime]
    sys_, wit = S.small_circuit(prime, 2)
    h = _holder(sys_, prime)
    fresh = M.Engine(0)
    try:
        LF.expect_refusal(fresh.lift_witness, "no result")
        LF.expect_refusal(fresh.fetch_witness, "no witness")
        fresh.load(h.inp)
        fresh.run(_flags("O2"))
        LF.expect_refusal(fresh.lift_witness, "no witness")
    finally:
        fresh.close()
    e = engine()
    out, sm, log = _run(h, "O2")
    v = W.project(wit[0], sm)
    assert len(sm) < sys_.max_signal
    # another size; the resident witness stays
    for bad in (v[:-1], v + [1]):
        e.load_witness(W.to_witness(bad, p))
        LF.expect_refusal(e.lift_witness, LF.WORDS["wires"])
        assert e.fetch_witness().values() == bad
    # another prime
    q = R.PRIMES["bls12381"]
    e.load_witness(W.to_witness([x % q for x in v], q))
    LF.expect_refusal(e.lift_witness, "prime")
    # a refused load leaves nothing to lift
    LF.expect_refusal(lambda: e.load_witness(W.to_witness([2] + v[1:], p)), "w[0]")
    LF.expect_refusal(e.lift_witness, "no witness")
    LF.expect_refusal(lambda: e.load_witness(W.to_witness(v[:1] + [p] + v[2:], p)), "not below the prime")
    # the log is off: refused, the wire witness stays resident, and after a run with the log a lift
    # succeeds without a reload
    e.load(h.inp)
    e.run(rsio.flags("O2"))
    e.load_witness(W.to_witness(v, p))
    LF.expect_refusal(e.lift_witness, "log")
    e.load(h.inp)
    e.run(_flags("O2"))
    rep = e.lift_witness()
    assert e.fetch_witness().values() == wit[0] and rep.counts() == _host(v, p, out.c)[1]
    # a second lift finds a witness of L values, not n_wires: refused, and the lifted one stays
    LF.expect_refusal(e.lift_witness, LF.WORDS["wires"])
    assert e.fetch_witness().values() == wit[0]
    assert all(f == 0 for _, f, _ in W.triples(e.check_witness(W.ALL, h.inp)).values())
    # null arguments
    assert abi.lib().rs_engine_lift_witness(e._h, None) == -1 and LF.WORDS["null"] in abi.lib().rs_last_error().decode()
    assert abi.lib().rs_engine_fetch_witness(e._h, None) == -1
    assert abi.lib().rs_engine_write_wtns_resident(e._h, None) == -1


# --------------------------------------------------------------------------- 5. the result does not move
def test_result_buffers_do_not_move(tmp_path):
    """The views rs_engine_simplify returned stay valid and equal after a lift."""
    sys_, wit = S.small_circuit("bn128", 6)
    h = _holder(sys_, "bn128")
    e = engine()
    for key in ("O2", "O1"):
        view = e.simplify(h.inp, _flags(key))
        a = rsio.output_arrays(view)
        log = rsio.output_log(view)
        sm = rsio.output_to_py(view)[1]
        before = e.fetch()
        e.load_witness(W.to_witness(W.project(wit[0], sm), sys_.p))
        e.lift_witness()
        e.write_wtns_resident(str(tmp_path / "o.wtns"))
        assert e.fetch_witness().values() == wit[0]
        assert rsio.diff_output_arrays(a, rsio.output_arrays(view)) is None and rsio.output_log(view) == log
        after = e.fetch()
        assert rsio.diff_output_arrays(rsio.output_arrays(before.c), rsio.output_arrays(after.c)) is None
        assert rsio.output_log(before.c) == rsio.output_log(after.c)


# --------------------------------------------------------------------------- 6. determinism
def test_lift_is_deterministic(monkeypatch, tmp_path):
    prime = "secq256r1"
    p = S.PRIMES[prime]
    sys_, wit = S.small_circuit(prime, 8)
    h = _holder(sys_, prime)
    out, sm, log = _run(h, "O2")
    v = W.random_vector(random.Random(1), len(sm), p)
    e = engine()
    seen = []
    for chunk in (None, None, "64"):
        if chunk is None:
            monkeypatch.delenv("RS_WIT_CHUNK", raising=False)
        else:
            monkeypatch.setenv("RS_WIT_CHUNK", chunk)
        vals, counts = _lift(v, p)
        path = str(tmp_path / "d.wtns")
        e.write_wtns_resident(path)
        seen.append((vals, counts, open(path, "rb").read()))
    assert seen[0] == seen[1] == seen[2]
    l2w, blog, bv = LF.border_log(p, 64)
    hb = LF.LogHolder(l2w, blog)
    monkeypatch.delenv("RS_WIT_CHUNK", raising=False)
    first = _one_shot(bv, p, hb.out)
    monkeypatch.setenv("RS_WIT_CHUNK", "64")
    assert _one_shot(bv, p, hb.out) == first


# --------------------------------------------------------------------------- 7. sharded
def test_sharded_rank_lifts_its_own_copy():
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
    for r in range(2):
        sm = rsio.output_to_py(outs[r].c)[1]
        for w in wit[:2]:
            v = W.project(w, sm)
            vals, counts = _lift(v, p, engs[r])
            assert vals == w and (vals, counts) == _host(v, p, outs[r].c)
