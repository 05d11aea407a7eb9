"""The device JSON writers (rs_engine_write_constraints_json / rs_engine_write_substitution_json and their
one-shots, csrc/json_write.hpp) against the host writers rs_write_constraints_json /
rs_write_substitution_json and the text models (rsio.py), byte for byte, at the default chunk size and at
RS_JSON_CHUNK=64 (the knob is read on every call), where one entry covers up to three chunks and some
chunks lie wholly inside one value."""
import os
import subprocess
import threading

import pytest

import degenerate
import jsonio
import rsio
import circom_cvm_amd as M
from circom_cvm_amd import abi

pytestmark = pytest.mark.gpu
R = rsio.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "circom_cvm_amd", "circom-simplify")
KINDS = ("constraints", "substitutions")
get = jsonio.get


@pytest.fixture(params=["default", "64"])
def chunk(request, monkeypatch):
    if request.param == "64":
        monkeypatch.setenv("RS_JSON_CHUNK", "64")
    else:
        monkeypatch.delenv("RS_JSON_CHUNK", raising=False)
    return request.param


def engine_write(eng, kind, path) -> int:
    L = abi.lib()
    f = L.rs_engine_write_constraints_json if kind == "constraints" else L.rs_engine_write_substitution_json
    return f(eng._h, path.encode())


def system():
    return rsio.gen_system(131, R.PRIMES["bn128"], n_sig=300, n_rows=300, big_cluster=400)


def models(res):
    return {"constraints": rsio.constraints_json_text(res.constraints, res.signal_map).encode(),
            "substitutions": rsio.substitutions_json_text(rsio.pyref_log(res.log)).encode()}


_MODELS = {}


def system_models(level="O2", prime="bn128"):
    """The model texts of system()'s result and log (computed once a level and prime)."""
    if (level, prime) not in _MODELS:
        sys_ = system() if prime == "bn128" else rsio.gen_system(131, R.PRIMES[prime], n_sig=300, n_rows=300, big_cluster=400)
        res = R.simplification(sys_, rsio.py_flags(rsio.flags(level)), want_log=True)
        _MODELS[(level, prime)] = (sys_, res, models(res))
    return _MODELS[(level, prime)]


@pytest.fixture(scope="module")
def run_engine():
    """An engine that holds the --O2 result and log of system()."""
    sys_, _res, _m = system_models()
    h = rsio.InputHolder(sys_)
    e = M.Engine(0)
    e.load(h.inp)
    e.run(rsio.flags("O2", log=True))
    yield e
    e.close()


def check_files_of(eng, tmp_path, want=None, tag="e"):
    """Both engine writers against the host writers over fetch() (and `want`, the models)."""
    out = eng.fetch()
    for kind in KINDS:
        dev, host = str(tmp_path / f"{tag}_dev_{kind}.json"), str(tmp_path / f"{tag}_host_{kind}.json")
        assert engine_write(eng, kind, dev) == 0, abi.lib().rs_last_error()
        assert jsonio.host_write(kind, host, out.c) == 0
        got, ref = get(dev), get(host)
        assert len(got) == len(ref) and got == ref, kind
        if want is not None:
            assert got == want[kind], kind
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_digit_output_through_the_one_shots(tmp_path, chunk, kind):
    h = jsonio.digit_output()
    dev, host = str(tmp_path / "dev.json"), str(tmp_path / "host.json")
    assert jsonio.host_write(kind, host, h.out) == 0
    assert jsonio.device_write(kind, dev, h.out) == 0, abi.lib().rs_last_error()
    got, want = get(dev), get(host)
    assert len(got) == len(want)
    assert got == want, next(i for i in range(len(want)) if got[i] != want[i])


def test_bad_outputs_are_refused(tmp_path, chunk, run_engine):
    """The one-shots refuse them with the contract's codes and leave no file -- with an engine that holds a
    result alive beside them, which then writes its own two files again unchanged."""
    eng = run_engine
    _sys, _res, want = system_models()
    before = {}
    for kind in KINDS:
        path = str(tmp_path / f"before_{kind}.json")
        assert engine_write(eng, kind, path) == 0
        before[kind] = get(path)
        assert before[kind] == want[kind]
    for name, (h, code) in jsonio.bad_outputs().items():
        kind = "substitutions" if name.startswith("log_") else "constraints"
        out = str(tmp_path / (name.replace("/", "_") + ".json"))
        assert jsonio.device_write(kind, out, h.out) == code, (name, abi.lib().rs_last_error())
        assert not os.path.exists(out), name
        f = abi.Output.write_substitution_json_device if kind == "substitutions" else abi.Output.write_constraints_json_device
        with pytest.raises(abi.RsError) as e:
            f(out, h.out)
        assert e.value.code == code and not os.path.exists(out), name
    for kind in KINDS:
        path = str(tmp_path / f"after_{kind}.json")
        assert engine_write(eng, kind, path) == 0
        assert get(path) == before[kind]


@pytest.mark.parametrize("level,prime", [("O1", "bn128"), ("O2", "bn128"), ("O2", "goldilocks")])
def test_engine_path(tmp_path, chunk, level, prime):
    sys_, _res, want = system_models(level, prime)
    h = rsio.InputHolder(sys_)
    e = M.Engine(0)
    try:
        e.load(h.inp)
        e.run(rsio.flags(level, log=True))
        check_files_of(e, tmp_path, want)
        for kind in KINDS:
            path = str(tmp_path / f"stats_{kind}.json")
            ms = e.write_constraints_json(path) if kind == "constraints" else e.write_substitution_json(path)
            st = e.json_stats()
            assert ms > 0 and st.write_ms == ms and st.kernel_ms > 0 and st.out_ms > 0
            if kind == "constraints":
                assert st.in_ms == 0
            elif len(want[kind]) > 3:
                assert st.in_ms > 0
            assert abs(st.in_ms + st.kernel_ms + st.out_ms - st.write_ms) < 1e-6 * max(1.0, st.write_ms)
            assert st.bytes == os.path.getsize(path) - len(jsonio.HEAD[kind]) - len(jsonio.TAIL[kind])
        # a run with the log off: the log file is `{\n}`, as the host writer's over the fetched output
        e.run(rsio.flags(level))
        path = str(tmp_path / "no_log.json")
        assert engine_write(e, "substitutions", path) == 0
        assert get(path) == b"{\n}"
        assert e.json_stats().bytes == 0
        out = e.fetch()
        assert jsonio.host_write("substitutions", str(tmp_path / "no_log_host.json"), out.c) == 0
        assert get(str(tmp_path / "no_log_host.json")) == b"{\n}"
    finally:
        e.close()


def test_writer_host_routes_to_the_host_writers(tmp_path, run_engine, monkeypatch):
    _sys, _res, want = system_models()
    monkeypatch.setenv("RS_WRITER_HOST", "1")
    for kind in KINDS:
        path = str(tmp_path / f"via_host_{kind}.json")
        assert engine_write(run_engine, kind, path) == 0
        assert get(path) == want[kind]
        st = run_engine.json_stats()
        assert st.write_ms > 0 and st.in_ms == 0 and st.kernel_ms == 0 and st.out_ms == 0
        assert st.bytes == len(want[kind]) - len(jsonio.HEAD[kind]) - len(jsonio.TAIL[kind])


def test_after_a_streamed_result(tmp_path, chunk):
    """rs_engine_simplify gives ABI 8's streamed layout: both engine writers and the one-shots over that
    rs_output as it is are right, and fetch, write_r1cs and write_sym still are afterwards (the writers'
    device buffers leave the result's views alone)."""
    sys_, res, want = system_models()
    h = rsio.InputHolder(sys_)
    sym_lines = [(i, i, i % 3, f"main.s[{i}]") for i in range(1, sys_.max_signal)]
    src = str(tmp_path / "in.sym")
    with open(src, "wb") as f:
        f.write("".join(f"{a},{b},{c},{d}\n" for a, b, c, d in sym_lines).encode())
    e = M.Engine(0)
    try:
        view = e.simplify(h.inp, rsio.flags("O2", log=True))
        for kind in KINDS:
            path = str(tmp_path / f"one_shot_{kind}.json")
            assert jsonio.device_write(kind, path, view) == 0, abi.lib().rs_last_error()
            assert get(path) == want[kind], kind
        for kind in KINDS:
            path = str(tmp_path / f"engine_{kind}.json")
            assert engine_write(e, kind, path) == 0, abi.lib().rs_last_error()
            assert get(path) == want[kind], kind
        out = e.fetch()
        assert rsio.same_result(res, rsio.output_to_py(out.c)) is None
        e.write_r1cs(str(tmp_path / "o.r1cs"))
        assert get(str(tmp_path / "o.r1cs")) == R.result_to_r1cs(sys_, res)
        e.write_sym(src, str(tmp_path / "o.sym"))
        assert get(str(tmp_path / "o.sym")) == R.result_to_sym(sym_lines, res).encode()
    finally:
        e.close()


def test_engine_without_a_result_is_invalid(tmp_path):
    e = M.Engine(0)
    try:
        for kind in KINDS:
            out = str(tmp_path / f"{kind}.json")
            assert engine_write(e, kind, out) == -1
            assert not os.path.exists(out)
        with pytest.raises(abi.RsError) as err:
            e.write_constraints_json(str(tmp_path / "o.json"))
        assert err.value.code == -1 and not os.path.exists(str(tmp_path / "o.json"))
    finally:
        e.close()


@pytest.mark.parametrize("name,n_rows", [("max_signal_1", 0), ("x_eq_0", 0), ("ab_eq_c", 1)])
def test_zero_and_one_row_results(tmp_path, chunk, name, n_rows):
    sys_ = degenerate.singletons(R.PRIMES["bn128"])[name]
    res = R.simplification(sys_, R.Flags(), want_log=True)
    assert len(res.constraints) == n_rows
    want = models(res)
    h = rsio.InputHolder(sys_)
    e = M.Engine(0)
    try:
        e.load(h.inp)
        e.run(rsio.flags("O2", log=True))
        out = check_files_of(e, tmp_path, want)
        for kind in KINDS:
            path = str(tmp_path / f"one_shot_{kind}.json")
            assert jsonio.device_write(kind, path, out.c) == 0, abi.lib().rs_last_error()
            assert get(path) == want[kind]
    finally:
        e.close()
    # the hand-built empty output: no rows, no log
    empty = jsonio.empty_output()
    for kind in KINDS:
        path = str(tmp_path / f"empty_{kind}.json")
        assert jsonio.device_write(kind, path, empty.out) == 0
        assert get(path) == jsonio.HEAD[kind] + jsonio.TAIL[kind]


def test_rank_1_of_a_group_writes_the_whole_files(tmp_path):
    """World 2 in one process: every rank holds the whole result and the whole log, the writers are no
    collectives, and rank 1 alone writes both files -- the host writers' bytes over its own fetch()."""
    world = 2
    inp = M.Input.synth(0, 300_000, 42)
    g = M.Group(world)
    engs = [M.Engine(0) for _ in range(world)]
    errs = [None] * world
    try:
        for r, e in enumerate(engs):
            e.join_group(g, r)

        def work(r):
            try:
                engs[r].load(inp.c)
                engs[r].run(rsio.flags("O2", log=True))
            except Exception as ex:  # noqa: BLE001 -- reported below
                errs[r] = ex

        th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=240)
            assert not t.is_alive(), "sharded run hung"
        for ex in errs:
            if ex is not None:
                raise ex
        out = check_files_of(engs[1], tmp_path)
        assert out.c.n_constraints > 1000 and out.c.n_log > 1000
    finally:
        for e in engs:
            e.close()
        g.close()


def test_cli_device_and_host_reader_write_the_same_files(tmp_path, chunk):
    sys_, res, want = system_models()
    ident = R.Result(sys_.rows, {i: i for i in range(sys_.max_signal)}, sys_.n_priv_in)
    r1 = str(tmp_path / "in.r1cs")
    with open(r1, "wb") as f:
        f.write(R.result_to_r1cs(sys_, ident))
    sym_lines = [(i, i, i % 3, f"main.s[{i}]") for i in range(1, sys_.max_signal)]
    sy = str(tmp_path / "in.sym")
    with open(sy, "wb") as f:
        f.write("".join(f"{a},{b},{c},{d}\n" for a, b, c, d in sym_lines).encode())
    outs = {}
    for tag, extra in (("dev", []), ("host", ["--host-reader"])):
        pre = str(tmp_path / tag)
        r = subprocess.run([EXE, r1, sy, "--O2", "--json", "--simplification_substitution", *extra, "-o", pre],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs[tag] = [get(pre + sfx) for sfx in (".r1cs", ".sym", "_constraints.json", "_substitutions.json")]
    assert outs["dev"] == outs["host"]
    assert outs["dev"][0] == R.result_to_r1cs(sys_, res)
    assert outs["dev"][1] == R.result_to_sym(sym_lines, res).encode()
    assert outs["dev"][2] == want["constraints"] and outs["dev"][3] == want["substitutions"]
