"""The device .sym writer (rs_engine_write_sym / rs_write_sym_device, csrc/sym_write.hpp) against the host
writer rs_write_sym and the split-on-newline model (symio.py), byte for byte, at the default chunk size
and at RS_SYM_CHUNK=64 (the knob is read on every call), where a file of a few thousand lines is cut
into a few thousand chunks and every field boundary meets every chunk offset.  The one-shot gets an
otherwise zeroed rs_output (only n_labels and label_to_wire are read)."""
import os
import subprocess

import numpy as np
import pytest

import rsio
import symio
import circom_cvm_amd as M
from circom_cvm_amd import abi

pytestmark = pytest.mark.gpu
R = rsio.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "circom_cvm_amd", "circom-simplify")


@pytest.fixture(params=["default", "64"])
def chunk(request, monkeypatch):
    if request.param == "64":
        monkeypatch.setenv("RS_SYM_CHUNK", "64")
    else:
        monkeypatch.delenv("RS_SYM_CHUNK", raising=False)
    return request.param


def put(tmp_path, name, data) -> str:
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    return path


def get(path) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def system_and_sym():
    sys_ = rsio.gen_system(131, R.PRIMES["bn128"], n_sig=300, n_rows=300, big_cluster=400)
    sym_lines = [(i, i, i % 3, f"main.s[{i}]") for i in range(1, sys_.max_signal)]
    text = "".join(f"{a},{b},{c},{d}\n" for a, b, c, d in sym_lines).encode()
    return sys_, sym_lines, text


@pytest.fixture(scope="module")
def run_engine():
    """An engine that holds the --O2 result of a random system: (engine, system, sym lines, sym text, oracle result)."""
    sys_, sym_lines, text = system_and_sym()
    h = rsio.InputHolder(sys_)
    e = M.Engine(0)
    e.load(h.inp)
    e.run(rsio.flags("O2"))
    res = R.simplification(sys_, R.Flags())
    yield e, sys_, sym_lines, text, res
    e.close()


@pytest.mark.parametrize("level", ["O1", "O2"])
def test_docs_basic(tmp_path, chunk, level):
    import sys
    sys.path.insert(0, GOLD)
    import make_golden as G
    sys_ = G.docs_system()
    res = R.simplification(sys_, G.flags_of(level))
    l2w = np.full(sys_.max_signal, -1, np.int32)
    for lab, w in res.signal_map.items():
        l2w[lab] = w
    out = str(tmp_path / "o.sym")
    assert symio.device_write(os.path.join(GOLD, "docs_basic_O0.sym"), out, l2w) == 0
    assert get(out) == get(os.path.join(GOLD, f"docs_basic_{level}.sym"))


@pytest.mark.parametrize("name", sorted(symio.valid_files()))
def test_valid_files_equal_the_host_writer(tmp_path, chunk, name):
    text, l2w = symio.valid_files()[name]
    src = put(tmp_path, "in.sym", text)
    host, dev = str(tmp_path / "host.sym"), str(tmp_path / "dev.sym")
    assert symio.host_write(src, host, l2w) == 0
    assert symio.device_write(src, dev, l2w) == 0, abi.lib().rs_last_error()
    want = get(host)
    assert want == symio.model(text, l2w)
    got = get(dev)
    assert len(got) == len(want) and got == want


def test_refused_files_leave_no_output_and_a_usable_engine(tmp_path, chunk, run_engine):
    eng, _sys, _lines, text, _res = run_engine
    good = put(tmp_path, "good.sym", text)
    want = str(tmp_path / "want.sym")
    eng.write_sym(good, want)
    L = abi.lib()
    for name, data in symio.bad_files().items():
        src = put(tmp_path, name.replace("/", "_") + ".sym", data)
        out = str(tmp_path / (name.replace("/", "_") + ".out"))
        assert L.rs_engine_write_sym(eng._h, src.encode(), out.encode()) == -1, name
        assert not os.path.exists(out), name
    # the one-shot refuses them too (one kind of each placement)
    for name in ("leading_zero_L/mid", "empty_W/straddle", "one_comma/last", "nul/mid"):
        src = put(tmp_path, "one_shot.sym", symio.bad_files()[name])
        out = str(tmp_path / "one_shot.out")
        assert symio.device_write(src, out, symio.small_l2w()) == -1, name
        assert not os.path.exists(out), name
    again = str(tmp_path / "again.sym")
    eng.write_sym(good, again)
    assert get(again) == get(want)


def test_engine_path(tmp_path, chunk, run_engine, monkeypatch):
    eng, sys_, sym_lines, text, res = run_engine
    src = put(tmp_path, "in.sym", text)
    dev, host, via_host = (str(tmp_path / n) for n in ("dev.sym", "host.sym", "via_host.sym"))
    ms = eng.write_sym(src, dev)
    st = eng.stats()
    assert ms > 0 and st.sym_in_ms > 0 and st.sym_kernel_ms > 0 and st.sym_out_ms > 0
    assert abs(st.sym_in_ms + st.sym_kernel_ms + st.sym_out_ms - st.sym_write_ms) < 1e-6 * max(1.0, st.sym_write_ms)
    assert get(dev) == R.result_to_sym(sym_lines, res).encode()
    out = eng.fetch()
    assert abi.lib().rs_write_sym(src.encode(), host.encode(), out.ptr) == 0
    assert get(dev) == get(host)
    monkeypatch.setenv("RS_WRITER_HOST", "1")
    eng.write_sym(src, via_host)
    assert get(via_host) == get(dev)


def test_engine_without_a_result_is_invalid(tmp_path):
    src = put(tmp_path, "in.sym", b"1,1,1,main.out\n")
    out = str(tmp_path / "o.sym")
    e = M.Engine(0)
    try:
        assert abi.lib().rs_engine_write_sym(e._h, src.encode(), out.encode()) == -1
        with pytest.raises(abi.RsError) as err:
            e.write_sym(src, out)
        assert err.value.code == -1 and not os.path.exists(out)
    finally:
        e.close()


def test_after_a_streamed_result_the_engine_still_fetches(tmp_path, chunk):
    """rs_engine_simplify (the CLI's path), then write_sym, then fetch and write_r1cs: the .sym writer's
    device buffers leave the result's views alone."""
    sys_, sym_lines, text = system_and_sym()
    h = rsio.InputHolder(sys_)
    src = put(tmp_path, "in.sym", text)
    e = M.Engine(0)
    try:
        e.simplify(h.inp, rsio.flags("O2"))
        e.write_sym(src, str(tmp_path / "o.sym"))
        res = R.simplification(sys_, R.Flags())
        assert get(str(tmp_path / "o.sym")) == R.result_to_sym(sym_lines, res).encode()
        out = e.fetch()
        assert rsio.same_result(res, rsio.output_to_py(out.c)) is None
        e.write_r1cs(str(tmp_path / "o.r1cs"))
        assert get(str(tmp_path / "o.r1cs")) == R.result_to_r1cs(sys_, res)
    finally:
        e.close()


def test_cli_device_and_host_reader_write_the_same_sym(tmp_path, chunk):
    sys_, sym_lines, text = system_and_sym()
    ident = R.Result(sys_.rows, {i: i for i in range(sys_.max_signal)}, sys_.n_priv_in)
    r1 = put(tmp_path, "in.r1cs", R.result_to_r1cs(sys_, ident))
    sy = put(tmp_path, "in.sym", text)
    outs = {}
    for tag, extra in (("dev", []), ("host", ["--host-reader"])):
        pre = str(tmp_path / tag)
        r = subprocess.run([EXE, r1, sy, "--O2", *extra, "-o", pre], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs[tag] = get(pre + ".sym")
    assert outs["dev"] == outs["host"]
    assert outs["dev"] == R.result_to_sym(sym_lines, R.simplification(sys_, R.Flags())).encode()
