"""The empty, single and widest shapes of tests/degenerate.py through the library, on ONE engine for the
file (a call that leaves stale state behind is seen by the next call): every result equals the oracle's
bit for bit, the satisfiable ones also pass tests/soundness.py's check on the engine's own output and
log.  An ordinary gen_system case runs after every tenth degenerate one, and the empty input right after
the largest case of the file.  Entry paths: load = rs_engine_load / run / fetch, simplify =
rs_engine_simplify (streamed, keys first), oneshot = rs_simplify, log = load with
emit_substitution_log against pyref's literal log.  The shapes are proved on the CPU by
tests/test_degenerate.py; every test asserts the set of (case, entry path) pairs it ran."""
import ctypes as C
import dataclasses
import os
import struct
import subprocess
import sys
import threading

import numpy as np
import pytest

import degenerate as D
import readerio
import rsio
import soundness as S
import circom_cvm_amd as M
from circom_cvm_amd import abi
import test_flatten as TF
import test_gpu_sharded as SH
from test_gpu_writer import device_bytes, host_bytes

pytestmark = pytest.mark.gpu
R = rsio.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "circom_cvm_amd", "circom-simplify")
P_IDS = [nm for nm, _ in D.PRIMES3]
_ENG = None
_COUNT = [0]
_NORMAL = {}


def engine():
    global _ENG
    if _ENG is None:
        _ENG = M.Engine(0)
    return _ENG


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    global _ENG
    if _ENG is not None:
        _ENG.close()
        _ENG = None
    SH.release_groups()


# ---------------------------------------------------------------------------- the entry paths
def check_csr(o):
    """A fetched result is compact CSR with n_rows + 1 offsets per block, also for zero rows (where
    rsio's readers never look at them): ptr[0] = 0 and ptr[n] = nnz."""
    n = int(o.n_constraints)
    for q in range(3):
        lc, lay = o.block(q)
        assert lay is None and lc.ptr and int(lc.n_rows) == n
        assert int(lc.ptr[0]) == 0 and int(lc.ptr[n]) == int(lc.nnz), (q, n, int(lc.ptr[0]), int(lc.ptr[n]), int(lc.nnz))
    if int(o.n_log):
        assert int(o.log_to.ptr[0]) == 0 and int(o.log_to.ptr[int(o.n_log)]) == int(o.log_to.nnz)


def run_path(path, inp, fl):
    """-> (result arrays, log or None) of `inp` through one entry path on the file's engine."""
    e = engine()
    if path == "load":
        e.load(inp)
        e.run(fl)
        out = e.fetch()
        check_csr(out.c)
        return rsio.output_arrays(out.c), None
    if path == "simplify":
        return rsio.output_arrays(e.simplify(inp, fl)), None
    if path == "oneshot":
        out = C.POINTER(abi.RsOutput)()
        abi.check(abi.lib().rs_simplify(C.byref(inp), C.byref(fl), C.byref(out)))
        try:
            check_csr(out.contents)
            return rsio.output_arrays(out.contents), None
        finally:
            abi.lib().rs_output_free(out)
    assert path == "log"
    fl2 = abi.RsFlags.from_buffer_copy(fl)
    fl2.emit_substitution_log = 1
    e.load(inp)
    e.run(fl2)
    out = e.fetch()
    check_csr(out.c)
    return rsio.output_arrays(out.c), (rsio.output_to_py(out.c), rsio.output_log(out.c))


def normal_case():
    if not _NORMAL:
        h = rsio.InputHolder(D.normal_system(), "bn128")
        _NORMAL["h"], _NORMAL["ref"] = h, rsio.oracle_arrays(h.inp, rsio.flags("O2"))[0]
    return _NORMAL["h"], _NORMAL["ref"]


def check_normal(after):
    h, ref = normal_case()
    for path in ("load", "simplify"):
        d = rsio.diff_output_arrays(run_path(path, h.inp, rsio.flags("O2"))[0], ref)
        assert d is None, f"the ordinary case via {path} after {after}: {d}"


def check_case(what, sys_, pname, key, paths, ran, wit=None, sound=False):
    """One case at one flag set through `paths`: bit for bit the oracle's; with `sound` the engine's own
    result and log through soundness.check; the log path against pyref's literal log."""
    h = D.holder(sys_, pname)
    fl = D.fl_of(key)
    ref, _ = rsio.oracle_arrays(h.inp, fl)
    for path in paths:
        got, logged = run_path(path, h.inp, fl)
        d = rsio.diff_output_arrays(got, ref)
        assert d is None, f"{what} {pname} {key} via {path}: {d}"
        if logged is not None:
            (cons, sm, nw, npiw), log = logged
            res = R.simplification(sys_, rsio.py_flags(fl), want_log=True)
            assert log == rsio.pyref_log(res.log), f"{what} {pname} {key}: the log differs from pyref's"
            assert rsio.same_result(res, (cons, sm, nw, npiw)) is None
            if sound:
                S.check(sys_, (cons, sm, npiw, log), wit)
        ran.add((what, key, path))
        _COUNT[0] += 1
        if _COUNT[0] % 10 == 0:
            check_normal(f"{what} {pname} {key} via {path}")


# ---------------------------------------------------------------------------- A. the block lattice
@pytest.mark.parametrize("pname", P_IDS)
@pytest.mark.parametrize("family", ["gen", "sat"])
def test_lattice(family, pname):
    """Each of the 16 class subsets at the five flag sets through load and simplify; the satisfiable
    family with the log on through soundness.check; four masks also through rs_simplify and against
    pyref's log."""
    _, wit = D.lattice_base(family, pname)
    ran, want = set(), set()
    for mask, sys_ in D.lattice_cases(family, pname):
        for key in D.FLAG_SETS:
            paths = ["load", "simplify"]
            if family == "sat" or mask in D.ONESHOT_MASKS:
                paths.append("log")
            if mask in D.ONESHOT_MASKS:
                paths.append("oneshot")
            want |= {(mask, key, pa) for pa in paths}
            check_case(mask, sys_, pname, key, paths, ran, wit, sound=family == "sat")
    assert ran == want and len({(m, k) for m, k, _ in ran}) == 80


# ---------------------------------------------------------------------------- B. singletons and headers
@pytest.mark.parametrize("pname,p", D.PRIMES3, ids=P_IDS)
def test_singletons(pname, p):
    ran, want = set(), set()
    for name, sys_ in D.singletons(p).items():
        for key in D.FLAG_SETS:
            paths = ["load", "simplify", "log", "oneshot"]
            want |= {(name, key, pa) for pa in paths}
            check_case(name, sys_, pname, key, paths, ran, sound=name in D.SOUND_SINGLETONS)
    assert ran == want and len({n for n, _, _ in ran}) == 14


@pytest.mark.parametrize("pname,p", D.PRIMES3, ids=P_IDS)
def test_dags(pname, p):
    """rs_flatten_dag and rs_engine_flatten_dag against pyref.flatten_dag block for block, then the
    engine's view through rs_engine_simplify against the oracle."""
    ran = set()
    e = engine()
    for name, (nodes, main, no, npb, npr, forb) in D.dags(p).items():
        sys_, b = R.flatten_dag(p, nodes, main, no, npb, npr, forb)
        d = M.Dag(p, nodes, main, no, npb, npr, forb, D.abi_name(pname))
        one = d.flatten(0)
        TF._eq_blocks(TF.blocks_of(one.c), b, sys_)
        ran.add((name, "rs_flatten_dag"))
        view = e.flatten_dag(d)
        TF._eq_blocks(TF.blocks_of(view), b, sys_)
        assert readerio.diff_inputs(readerio.input_arrays(one.c), readerio.input_arrays(view)) is None, name
        ran.add((name, "rs_engine_flatten_dag"))
        h = D.holder(sys_, pname)   # (kept: it owns the arrays behind h.inp)
        for key in ("O2", "O1", "O2round1"):
            fl = D.fl_of(key)
            ref, _ = rsio.oracle_arrays(h.inp, fl)
            diff =rsio.diff_output_arrays(rsio.output_arrays(e.simplify(view, fl)), ref)
            assert diff is None, (name, key, diff)
            ran.add((name, "simplify " + key))
        one.free()
        check_normal(f"the DAG {name}")
    assert ran == {(n, s) for n in D.dags(p) for s in ("rs_flatten_dag", "rs_engine_flatten_dag", "simplify O2", "simplify O1",
                                                       "simplify O2round1")}


# ---------------------------------------------------------------------------- C. every way in and out
def put(tmp_path, name, data) -> str:
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    return path


def get(path) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def o0_bytes(sys_) -> bytes:
    return R.result_to_r1cs(sys_, R.Result(sys_.rows, {i: i for i in range(sys_.max_signal)}, sys_.n_priv_in))


def sym_text(sys_) -> bytes:
    return "".join(f"{i},{i},{i % 2},main.s[{i}]\n" for i in range(sys_.max_signal)).encode()


def sym_lines(sys_):
    return [(i, i, i % 2, f"main.s[{i}]") for i in range(sys_.max_signal)]


def smallest_results():
    """name -> (System, rows of its --O2 result): zero rows with more than one wire, one row, the
    all-forbidden result, and zero rows with signal 0 the only wire."""
    s = D.singletons(D.BN)
    only0 = R.System(D.BN, 6, 0, 0, 2, {0}, [R.Con({}, {}, {3: 1, 0: 2})])
    return {"zero_rows": s["x_eq_c"], "one_row": s["ab_eq_c"], "all_forbidden": s["all_forbidden"], "only_wire_0": only0}


def test_writers_on_the_smallest_results(tmp_path, monkeypatch):
    ran = set()
    e = engine()
    for name, sys_ in smallest_results().items():
        h = D.holder(sys_, "bn128")
        fl = rsio.flags("O2", log=True)
        res = R.simplification(sys_, rsio.py_flags(fl), want_log=True)
        assert len(res.constraints) == {"zero_rows": 0, "one_row": 1, "only_wire_0": 0}.get(name, len(res.constraints))
        if name == "zero_rows":
            assert len(res.signal_map) > 1
        if name == "only_wire_0":
            assert res.signal_map == {0: 0}
        want = R.result_to_r1cs(sys_, res)
        src = put(tmp_path, name + "_in.sym", sym_text(sys_))
        want_sym = R.result_to_sym(sym_lines(sys_), res).encode()
        for path in ("simplify", "load"):
            if path == "simplify":
                out = e.simplify(h.inp, fl)
                keep = None
            else:
                e.load(h.inp)
                e.run(fl)
                keep = e.fetch()
                out = keep.c
            tag = f"{name}_{path}"
            a = host_bytes(str(tmp_path / (tag + "_h.r1cs")), h.inp, out)
            b = device_bytes(e, str(tmp_path / (tag + "_d.r1cs")))
            assert a == b == want, tag
            monkeypatch.setenv("RS_WRITER_HOST", "1")
            assert device_bytes(e, str(tmp_path / (tag + "_dh.r1cs"))) == want, tag
            e.write_sym(src, str(tmp_path / (tag + "_dh.sym")))
            monkeypatch.delenv("RS_WRITER_HOST")
            e.write_sym(src, str(tmp_path / (tag + "_d.sym")))
            assert abi.lib().rs_write_sym(src.encode(), str(tmp_path / (tag + "_h.sym")).encode(), C.byref(out)) == 0
            assert get(str(tmp_path / (tag + "_d.sym"))) == get(str(tmp_path / (tag + "_h.sym"))) == want_sym, tag
            assert get(str(tmp_path / (tag + "_dh.sym"))) == want_sym, tag
            empty = put(tmp_path, "empty.sym", b"")
            e.write_sym(empty, str(tmp_path / (tag + "_e.sym")))
            assert abi.lib().rs_write_sym(empty.encode(), str(tmp_path / (tag + "_eh.sym")).encode(), C.byref(out)) == 0
            assert get(str(tmp_path / (tag + "_e.sym"))) == get(str(tmp_path / (tag + "_eh.sym"))) == b"", tag
            cj, sj = str(tmp_path / (tag + "_c.json")), str(tmp_path / (tag + "_s.json"))
            abi.check(abi.lib().rs_write_constraints_json(cj.encode(), C.byref(out)))
            abi.check(abi.lib().rs_write_substitution_json(sj.encode(), C.byref(out)))
            assert open(cj).read() == rsio.constraints_json_text(res.constraints, res.signal_map), tag
            assert open(sj).read() == rsio.substitutions_json_text(rsio.pyref_log(res.log)), tag
            ran.add((name, path))
            del keep
    assert ran == {(n, pa) for n in ("zero_rows", "one_row", "all_forbidden", "only_wire_0") for pa in ("simplify", "load")}
    sym = R.result_to_sym(sym_lines(smallest_results()["only_wire_0"]), R.simplification(smallest_results()["only_wire_0"], R.Flags()))
    assert [ln.split(",")[1] for ln in sym.splitlines()] == ["0"] + ["-1"] * 5     # every witness -1 but signal 0's


def test_custom_gates_on_a_zero_row_result(tmp_path):
    used = struct.pack("<I", 1) + b"CMul\x00" + struct.pack("<I", 1) + (7).to_bytes(32, "little")
    apps = [(0, [3, 4, 6]), (0, [7, 4, 3])]
    gsig = {x for _, sig in apps for x in sig}
    base = D.singletons(D.BN)["x_eq_c"]
    sys_ = dataclasses.replace(base, forbidden=base.forbidden | gsig, gates=(used, apps))
    o0 = put(tmp_path, "in.r1cs", o0_bytes(sys_))
    e = engine()
    inp = M.Input.read_r1cs(o0)
    for key in ("O1", "O2"):
        fl = D.fl_of(key)
        res = R.simplification(sys_, rsio.py_flags(fl))
        assert not res.constraints and len(res.signal_map) == 7
        out = e.simplify(inp.c, fl)
        a = host_bytes(str(tmp_path / "h.r1cs"), inp.c, out, o0)
        b = device_bytes(e, str(tmp_path / "d.r1cs"), o0)
        assert a == b == R.result_to_r1cs(sys_, res), key
    inp.free()


def _files_systems():
    base = R.System(D.BN, 80, 1, 1, 2, {0, 1, 2}, [])
    return {"empty": base, "one_empty": dataclasses.replace(base, rows=[R.Con({}, {}, {})])}


@pytest.mark.parametrize("name", ["empty", "one_empty"])
def test_empty_files_end_to_end(tmp_path, name):
    """The file read on the device, its view simplified, the result written back with its .sym: pyref's
    files; and once through circom-simplify, with --host-reader and without."""
    sys_ = _files_systems()[name]
    src = put(tmp_path, name + ".r1cs", o0_bytes(sys_))
    sy = put(tmp_path, name + ".sym", sym_text(sys_)[len(b"0,0,0,main.s[0]\n"):])
    lines = sym_lines(sys_)[1:]
    e = engine()
    assert readerio.compare_readers(e, src) == {"host": 0, "dev": 0, "diff": None}
    h = D.holder(sys_, "bn128")
    for key in ("O2", "O1", "O2round1"):
        fl = D.fl_of(key)
        res = R.simplification(sys_, rsio.py_flags(fl))
        assert not res.constraints and len(res.signal_map) == 3
        view = e.read_r1cs(src)
        assert int(view.linear.n_rows) == len(sys_.rows) and int(view.max_signal) == 80
        ref, _ = rsio.oracle_arrays(h.inp, fl)
        assert rsio.diff_output_arrays(rsio.output_arrays(e.simplify(view, fl)), ref) is None, key
        assert device_bytes(e, str(tmp_path / "d.r1cs")) == R.result_to_r1cs(sys_, res), key
        e.write_sym(sy, str(tmp_path / "d.sym"))
        assert get(str(tmp_path / "d.sym")) == R.result_to_sym(lines, res).encode(), key
    res = R.simplification(sys_, R.Flags(), want_log=True)
    outs = {}
    for tag, extra in (("dev", []), ("host", ["--host-reader"])):
        pre = str(tmp_path / tag)
        r = subprocess.run([EXE, src, sy, "--O2", "--json", "--simplification_substitution", *extra, "-o", pre],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs[tag] = tuple(get(pre + s) for s in (".r1cs", ".sym", "_constraints.json", "_substitutions.json"))
    assert outs["dev"] == outs["host"]
    assert outs["dev"] == (R.result_to_r1cs(sys_, res), R.result_to_sym(lines, res).encode(),
                           rsio.constraints_json_text(res.constraints, res.signal_map).encode(),
                           rsio.substitutions_json_text(rsio.pyref_log(res.log)).encode())
    check_normal(f"the file {name}")


# ---------------------------------------------------------------------------- D. ranks with nothing to do
@pytest.mark.parametrize("world", D.WORLDS)
def test_ranks_with_nothing_to_do(world):
    """In-process groups: fewer clusters than ranks, none at all, no relevant set, empty record lists --
    load / run / fetch and rs_engine_simplify on every rank equal the single-GPU oracle."""
    ran = set()
    for name, (sys_, _want) in D.rank_cases(D.BN, world).items():
        h = D.holder(sys_, "bn128")
        for key in ("O2", "O2round2", "O1"):
            fl = D.fl_of(key)
            ref, _ = rsio.oracle_arrays(h.inp, fl)
            for r, (got, st) in enumerate(SH.sharded_run(h.inp, fl, world, arrays=True)):
                d = rsio.diff_output_arrays(got, ref)
                assert d is None, f"{name} {key} load: rank {r}/{world}: {d}"
                assert st.world == world
            ran.add((name, key, "load"))
            for r, (got, st) in enumerate(SH.sharded_simplify(h.inp, fl, world)):
                d = rsio.diff_output_arrays(got, ref)
                assert d is None, f"{name} {key} simplify: rank {r}/{world}: {d}"
            ran.add((name, key, "simplify"))
    assert ran == {(n, k, pa) for n in D.RANK_CASES for k in ("O2", "O2round2", "O1") for pa in ("load", "simplify")}
    h, ref = normal_case()      # the group's next call is an ordinary one
    for r, (got, _st) in enumerate(SH.sharded_simplify(h.inp, rsio.flags("O2"), world)):
        assert rsio.diff_output_arrays(got, ref) is None, f"rank {r}"


def test_one_cluster_over_the_host_transport():
    """One linear cluster, two processes joined by the host transport (rs_engine_join_host)."""
    name, world = D.HOST_TRANSPORT_CASE
    child = os.path.join(ROOT, "tests", "degenerate_child.py")
    tag = f"dg{os.getpid()}"
    procs = [subprocess.Popen([sys.executable, "-u", child, str(world), str(r), tag, name], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=120)
            outs.append(out)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} exited {p.returncode}:\n{out[-3000:]}"
        assert f"rank {r} ok" in out


# ---------------------------------------------------------------------------- E. four-byte wires
def test_four_byte_wires(tmp_path):
    """2^24 + 1024 forbidden signals: the identity wire map puts four-byte wires into the writers.  The
    device writer's file equals the host writer's; its constraint section equals one built in Python
    from the oracle's rows with int.to_bytes as the sort key; read back as an --O0 file, the device
    reader equals the host reader.  Then the empty input on the same engine."""
    h = D.WideHolder()
    fl = rsio.flags("O2")
    ref, _ = rsio.oracle_arrays(h.inp, fl)
    e = engine()
    out = e.simplify(h.inp, fl)
    assert rsio.diff_output_arrays(rsio.output_arrays(out), ref) is None
    cons, sm, nw, _ = rsio.output_to_py(out)
    assert nw == D.WIDE_S and all(sm[k] == k for c in cons for q in (c.a, c.b, c.c) for k in q)
    a = host_bytes(str(tmp_path / "h.r1cs"), h.inp, out)
    pd = str(tmp_path / "d.r1cs")
    b = device_bytes(e, pd)
    assert len(a) == len(b) and a == b
    _, body, size = readerio.sections(b)[2]
    want = D.constraint_section(cons, 32)
    assert size == len(want) and b[body:body + size] == want
    del a, b
    os.remove(str(tmp_path / "h.r1cs"))
    assert readerio.compare_readers(e, pd) == {"host": 0, "dev": 0, "diff": None}
    os.remove(pd)
    # the empty input directly after the largest case of the file, then an ordinary one
    ran = set()
    for pname, _ in D.PRIMES3:
        check_case("0000", D.lattice_cases("gen", pname)[0][1], pname, "O2", ["load", "simplify", "log"], ran)
    assert len(ran) == 3
    check_normal("the wide system")
