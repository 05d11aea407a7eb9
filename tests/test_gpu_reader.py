"""The device --O0 reader (rs_engine_read_r1cs_o0 / rs_read_r1cs_o0_device, csrc/r1cs_read.hpp) against
its oracle, the host reader rs_read_r1cs_o0, on the same file: every scalar, `forbidden` and the six
blocks' n_rows / nnz / ptr / col / val equal (readerio.diff_inputs, the one comparison), and the same
verdict on malformed files.  The small sizes RS_R1CS_CHUNK=64 RS_R1CS_GROUP=2 (set for a child
process) cut a section of a few thousand 4-byte slots into hundreds of chunks and several groups, so
every table of the boundary search is walked and random value bytes act as bogus counts in every chunk;
at the default sizes these files are one chunk."""
import dataclasses
import json
import os
import struct
import subprocess
import sys

import pytest

import dagio
import readerio
import rsio
import circom_cvm_amd as M

pytestmark = pytest.mark.gpu
R = rsio.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DOCS = os.path.join(GOLD, "docs_basic_O0.r1cs")
EXE = os.path.join(ROOT, "circom_cvm_amd", "circom-simplify")
SMALL = {"RS_R1CS_CHUNK": "64", "RS_R1CS_GROUP": "2"}


def o0_bytes(sys_) -> bytes:
    ident = R.Result(sys_.rows, {i: i for i in range(sys_.max_signal)}, sys_.n_priv_in)
    return R.result_to_r1cs(sys_, ident)


def write(tmp_path, name, data) -> str:
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    return path


def child(good, files, env=SMALL):
    """Both readers on `files` in a child process under `env`, on one engine (readerio.main)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "readerio.py"), good, *files],
                       capture_output=True, text=True, timeout=120, env={**os.environ, **env})
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def assert_equal_reads(res, files):
    for f, r in zip(files, res):
        assert r["host"] == 0 and r["dev"] == 0 and r["diff"] is None and r["good_after"], (os.path.basename(f), r)


@pytest.fixture(scope="module")
def eng():
    e = M.Engine(0)
    yield e
    e.close()


def random_systems():
    out = []
    for i, (prime, n_rows, density) in enumerate([("bn128", 120, 1.0), ("bn128", 300, 3.0), ("bls12381", 200, 2.0),
                                                   ("goldilocks", 250, 3.0), ("goldilocks", 130, 1.5)]):
        out.append((f"{prime}_{n_rows}", rsio.gen_system(500 + i, R.PRIMES[prime], n_sig=90 + 40 * i, n_rows=n_rows,
                                                        density=density)))
    return out


def test_docs_basic_default_sizes(eng):
    r = readerio.compare_readers(eng, DOCS)
    assert r == {"host": 0, "dev": 0, "diff": None}
    one = M.Input.read_r1cs_device(DOCS)  # the one-shot: malloc'ed arrays
    assert readerio.diff_inputs(readerio.host_read(DOCS)[1], readerio.input_arrays(one.c)) is None
    one.free()


def test_random_systems_default_and_small_sizes(eng, tmp_path):
    files = []
    for name, sys_ in random_systems():
        data = o0_bytes(sys_)
        fs = R.field_size_bytes(sys_.p)
        assert struct.unpack_from("<I", data, readerio.sections(data)[1][1])[0] == fs
        assert fs == (8 if name.startswith("goldilocks") else 32)  # goldilocks: 8-byte fields in the file
        files.append(write(tmp_path, name + ".r1cs", data))
    for f in files:  # the defaults: one chunk
        assert readerio.compare_readers(eng, f) == {"host": 0, "dev": 0, "diff": None}, f
    assert_equal_reads(child(DOCS, files), files)


def boundary_system():
    """LCs just under, at and over a chunk (64 slots) and a group (128 slots) at fs 32 -- a C row of k
    entries is 1 + 9 k slots -- one that jumps over whole groups, runs of one-slot LCs, an all-empty
    constraint and a non-linear row with an empty B."""
    p = R.PRIMES["bn128"]
    S = 80
    rows = []

    def crow(k, base):
        return R.Con({}, {}, {1 + (base + j) % (S - 1): 2 + j for j in range(k)})

    for i, k in enumerate((1, 6, 7, 8, 14, 15, 60)):
        rows.append(crow(k, 3 * i))
        rows += [R.Con({}, {}, {1 + (i + j) % (S - 1): 1}) for j in range(50)]
        rows.append(R.Con({}, {}, {}))
        rows.append(R.Con({1 + i: 1, 0: 5}, {}, {2 + i: p - 1}))
        rows.append(R.Con({3: 1}, {4: p - 2, 5: 1}, crow(k, 7).c))
    rows.append(crow(60, 11))  # the file ends in a long LC
    return R.System(p, S, 1, 1, 2, {0, 1, 2}, rows)


def test_boundary_shapes_small_sizes(tmp_path):
    sys_ = boundary_system()
    files = [write(tmp_path, "boundary.r1cs", o0_bytes(sys_)),
             write(tmp_path, "empty.r1cs", o0_bytes(dataclasses.replace(sys_, rows=[]))),
             write(tmp_path, "one_empty.r1cs", o0_bytes(dataclasses.replace(sys_, rows=[R.Con({}, {}, {})])))]
    assert_equal_reads(child(DOCS, files), files)
    assert_equal_reads(child(DOCS, files, env={}), files)  # and at the defaults


def gate_system(seed=57):
    """A random system with one custom gate (section 4) applied twice (section 5): the applied signals
    are forbidden (dag/src/map_to_constraint_list.rs:22-24)."""
    sys_ = rsio.gen_system(seed, R.PRIMES["bn128"], n_sig=80, n_rows=150)
    used = struct.pack("<I", 1) + b"CMul\x00" + struct.pack("<I", 1) + (7).to_bytes(32, "little")
    apps = [(0, [10, 11, 12]), (0, [40, 41, 12])]
    gsig = {x for _, sig in apps for x in sig}
    return dataclasses.replace(sys_, forbidden=sys_.forbidden | gsig, gates=(used, apps))


def test_custom_gate_sections(eng, tmp_path):
    sys_ = gate_system()
    path = write(tmp_path, "gates.r1cs", o0_bytes(sys_))
    assert readerio.compare_readers(eng, path) == {"host": 0, "dev": 0, "diff": None}
    rc, got = readerio.engine_read(eng, path)
    assert rc == 0 and got["forbidden"].tolist() == sorted(sys_.forbidden)
    assert {10, 11, 12, 40, 41} <= set(got["forbidden"].tolist())


@pytest.mark.parametrize("env", [{}, SMALL], ids=["default", "small"])
def test_malformed_constraint_section(tmp_path, env):
    sys_ = rsio.gen_system(77, R.PRIMES["bn128"], n_sig=70, n_rows=160, density=2.0)
    data = o0_bytes(sys_)
    good = write(tmp_path, "good.r1cs", data)
    lcs = readerio.lc_offsets(data)
    size_at, body, size = readerio.sections(data)[2]
    assert lcs[0] == body and lcs[-1] < body + size
    mid = next(o for o in lcs[len(lcs) // 2:] if struct.unpack_from("<I", data, o)[0] >= 2)

    def patched(off, value):
        b = bytearray(data)
        struct.pack_into("<I", b, off, value)
        return bytes(b)

    huge = write(tmp_path, "huge_count.r1cs", patched(mid, 0x7fffffff))
    key = write(tmp_path, "bad_key.r1cs", patched(mid + 4, sys_.max_signal + 5))
    lower = write(tmp_path, "count_minus_one.r1cs", patched(mid, struct.unpack_from("<I", data, mid)[0] - 1))
    # forty extra bytes inside an enlarged section 2, after the last constraint
    extra = bytearray(data[:body + size] + bytes(range(1, 41)) + data[body + size:])
    struct.pack_into("<Q", extra, size_at, size + 40)
    extra = write(tmp_path, "extra.r1cs", bytes(extra))
    files = [huge, key, lower, extra]
    res = dict(zip(("huge", "key", "lower", "extra"), child(good, files, env=env)))
    assert all(r["good_after"] for r in res.values()), res
    assert res["huge"]["host"] == -1 and res["huge"]["dev"] == -1, res["huge"]
    assert res["key"]["host"] == -1 and res["key"]["dev"] == -1, res["key"]
    assert res["lower"]["host"] == res["lower"]["dev"] and res["lower"]["diff"] is None, res["lower"]
    assert res["extra"] == {"host": 0, "dev": 0, "diff": None, "good_after": True}, res["extra"]
    # the extra bytes change nothing but the file: the blocks are the good file's
    assert readerio.diff_inputs(readerio.host_read(good)[1], readerio.host_read(extra)[1]) is None


def test_view_feeds_simplify(eng, tmp_path):
    """eng.read_r1cs(path) then eng.simplify(view, --O2): bit-identical to the result from the host
    reader's input, and the view is unchanged afterwards."""
    other = write(tmp_path, "r.r1cs", o0_bytes(rsio.gen_system(91, R.PRIMES["bn128"], n_sig=300, n_rows=280, density=2.0)))
    fl = rsio.flags("O2")
    for path in (DOCS, other):
        host = M.Input.read_r1cs(path)
        want = rsio.output_arrays(eng.simplify(host.c, fl))
        view = eng.read_r1cs(path)
        before = readerio.input_arrays(view)
        got = rsio.output_arrays(eng.simplify(view, fl))
        assert rsio.diff_output_arrays(want, got) is None, path
        assert readerio.diff_inputs(before, readerio.input_arrays(view)) is None
        assert readerio.diff_inputs(readerio.host_read(path)[1], before) is None
        host.free()


def test_engine_buffers_reused(tmp_path):
    """Two reads on one engine, the second of a smaller file; then a flatten_dag and a read in either
    order (they share the engine's page-locked result buffers): each view is right when it is used."""
    big = write(tmp_path, "big.r1cs", o0_bytes(rsio.gen_system(92, R.PRIMES["bn128"], n_sig=200, n_rows=300, density=3.0)))
    small = write(tmp_path, "small.r1cs", o0_bytes(rsio.gen_system(93, R.PRIMES["bn128"], n_sig=40, n_rows=120)))
    p = R.PRIMES["bn128"]
    nodes, main, no, npb, npr, forb = dagio.gen_dag(303, p, n_templates=5)
    d = M.Dag(p, nodes, main, no, npb, npr, forb, "bn128")
    flat = d.flatten(0)
    flat_want = readerio.input_arrays(flat.c)
    e = M.Engine(0)
    for path in (big, small, big):
        assert readerio.compare_readers(e, path) == {"host": 0, "dev": 0, "diff": None}, path
    assert readerio.diff_inputs(flat_want, readerio.input_arrays(e.flatten_dag(d))) is None
    assert readerio.compare_readers(e, small) == {"host": 0, "dev": 0, "diff": None}
    assert readerio.diff_inputs(flat_want, readerio.input_arrays(e.flatten_dag(d))) is None
    assert readerio.diff_inputs(readerio.host_read(big)[1], readerio.input_arrays(e.read_r1cs(big))) is None
    flat.free()
    e.close()


def test_cli_device_and_host_reader_agree(tmp_path):
    sym = os.path.join(GOLD, "docs_basic_O0.sym")
    outs = {}
    for tag, extra in (("dev", []), ("host", ["--host-reader"])):
        pre = str(tmp_path / tag)
        r = subprocess.run([EXE, DOCS, sym, "--O2", "--json", "--simplification_substitution", *extra, "-o", pre],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs[tag] = (r.stdout, *(open(pre + s, "rb").read() for s in (".r1cs", ".sym", "_constraints.json", "_substitutions.json")))
    assert outs["dev"] == outs["host"]
    assert outs["dev"][1] == open(os.path.join(GOLD, "docs_basic_O2.r1cs"), "rb").read()
