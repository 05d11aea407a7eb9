"""The staging rings of csrc/stage_io.hpp once they wrap: every case runs at RS_IO_STAGE=65536 (the knob is
read on every call), where the inbound ring (StageIn, 4 buffers) is back at its first buffer after 256 KiB
and the outbound one (ImageOut, 8 buffers) after 512 KiB, on inputs of more than two laps of each.  At the
default 32 MiB no file of the suite leaves its ring's first buffers.  Every result is compared byte for
byte, or field for field, with the host twin that is its oracle everywhere else."""
import os
import random

import pytest

import jsonio
import readerio
import rsio
import symio
import wtnsio as W
import circom_cvm_amd as M
from circom_cvm_amd import abi

pytestmark = pytest.mark.gpu
R = rsio.R
STAGE = 65536
IN_LAPS = 9 * STAGE      # more than two laps of the 4 inbound buffers
OUT_LAPS = 17 * STAGE    # more than two laps of the 8 outbound buffers
P = R.PRIMES["bn128"]
P192 = 2 ** 192 - 237    # a prime of three limbs: n8 = 24, and 65536 is no multiple of 24


@pytest.fixture(autouse=True)
def small_stage(monkeypatch):
    monkeypatch.setenv("RS_IO_STAGE", str(STAGE))


def put(tmp_path, name, data) -> str:
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    return path


def get(path) -> bytes:
    with open(path, "rb") as f:
        return f.read()


class Run:
    """One engine that holds the --O2 result and the log of a 100,000-row rs_synth circuit (115,588 labels,
    some 41,000 wires and 74,000 substitutions: a .wtns of 1.3 MB, JSON files of 10 MB and more), the result
    fetched once."""

    def __init__(self):
        self.inp = M.Input.synth(0, 100000, 7)
        self.eng = M.Engine(0)
        self.eng.load(self.inp.c)
        self.eng.run(rsio.flags("O2", log=True))
        self.out = self.eng.fetch()
        self.n = int(self.inp.c.max_signal)

    def close(self):
        self.eng.close()
        self.out.free()
        self.inp.free()


@pytest.fixture(scope="module")
def run():
    r = Run()
    yield r
    r.close()


def staged_bytes(lc) -> int:
    return 8 * (int(lc.n_rows) + 1) + 36 * int(lc.nnz)


# --------------------------------------------------------------------------- 1. the --O0 reader
def test_reader_section_of_many_buffers(tmp_path, run):
    sys_ = rsio.gen_system(77, P, n_sig=3000, n_rows=6000, density=2.0)
    ident = R.Result(sys_.rows, {i: i for i in range(sys_.max_signal)}, sys_.n_priv_in)
    data = R.result_to_r1cs(sys_, ident)
    assert readerio.sections(data)[2][2] > IN_LAPS
    path = put(tmp_path, "in.r1cs", data)
    assert readerio.compare_readers(run.eng, path) == {"host": 0, "dev": 0, "diff": None}


# --------------------------------------------------------------------------- 2. the .sym writer
def sym_both(run, tmp_path, text, tag):
    """`text` through rs_engine_write_sym and through rs_write_sym over the fetched result: (device, host) bytes."""
    src = put(tmp_path, tag + ".in.sym", text)
    dev, host = str(tmp_path / (tag + ".dev.sym")), str(tmp_path / (tag + ".host.sym"))
    run.eng.write_sym(src, dev)
    assert abi.lib().rs_write_sym(src.encode(), host.encode(), run.out.ptr) == 0
    return get(dev), get(host)


@pytest.mark.parametrize("chunk", ["4096", "64"])
def test_sym_of_many_buffers(tmp_path, monkeypatch, run, chunk):
    monkeypatch.setenv("RS_SYM_CHUNK", chunk)
    text, _ = symio.gen_valid(5, 30000)
    assert len(text) > OUT_LAPS
    for tag, t in (("whole", text), ("no_newline", text[:-1])):  # the last piece's last byte decides the size
        got, want = sym_both(run, tmp_path, t, tag)
        assert len(want) > OUT_LAPS and want.endswith(b"\n")
        assert len(got) == len(want) and got == want, tag


# --------------------------------------------------------------------------- 3. the witness on its way in
def linear_probe(p, w, bad):
    """A linear block with one row per witness value, w[i] - value = 0: row i holds iff value i arrived; the
    rows in `bad` are off by one."""
    rows = [{i: 1, 0: (-(v + (1 if i in bad else 0))) % p} for i, v in enumerate(w) if i]
    return W.RawInput(p, len(w), linear=rows)


@pytest.mark.parametrize("p,n", [(P, 20000), (P192, 30000)])
def test_witness_of_many_buffers_both_loaders(tmp_path, p, n):
    n8 = W.n8_of(p)
    assert n8 in (32, 24) and n * n8 > IN_LAPS and (STAGE % n8 == 0) == (n8 == 32)
    rng = random.Random(n)
    w = W.random_vector(rng, n, p)
    per = STAGE // n8  # values a buffer: a bad row in the first buffer, at both sides of a wrap, in the last one
    bad = {1, 4 * per - 1, 4 * per, 4 * per + 1, 8 * per, n - 1}
    raw = linear_probe(p, w, bad)
    wit = W.to_witness(w, p)
    want = W.triples(abi.check_witness(wit, abi.WIT_INPUT, raw.inp))
    assert want["linear"] == (n - 1, len(bad), 0)
    eng = M.Engine(0)
    try:
        eng.load_witness(wit)
        assert W.triples(eng.check_witness(abi.WIT_INPUT, raw.inp)) == want
        eng.load_witness(W.to_witness([1] * n, p))   # (another witness in between)
        eng.load_wtns(put(tmp_path, "w.wtns", W.wtns_bytes(w, p)))
        assert W.triples(eng.check_witness(abi.WIT_INPUT, raw.inp)) == want
    finally:
        eng.close()


def test_check_witness_stages_input_and_log(run):
    c = run.inp.c
    blocks = [c.cons_eq, c.eq, c.linear, c.nl_a, c.nl_b, c.nl_c]
    assert sum(staged_bytes(b) for b in blocks) > IN_LAPS and max(staged_bytes(b) for b in blocks) > 4 * STAGE
    o = run.out.c
    assert 12 * int(o.n_log) + 36 * int(o.log_to.nnz) > IN_LAPS
    rng = random.Random(3)
    sparse = [1] + [rng.randrange(P) if rng.random() < 0.02 else 0 for _ in range(run.n - 1)]
    for w in (W.random_vector(rng, run.n, P), sparse):
        wit = W.to_witness(w, P)
        want = W.triples(abi.check_witness(wit, W.ALL, c, o))
        run.eng.load_witness(wit)
        assert W.triples(run.eng.check_witness(W.ALL, c)) == want
        assert [want[k][0] for k in W.CLASSES] == [int(b.n_rows) for b in blocks[:4]] + [int(o.n_constraints), int(o.n_log)]
    assert all(0 < want[k][1] < want[k][0] for k in ("linear", "nonlinear", "output", "log"))  # the sparse one: a mix


# --------------------------------------------------------------------------- 4. the images on their way out
def test_wtns_image_of_many_buffers(tmp_path, run):
    w = W.random_vector(random.Random(4), run.n, P)
    wit = W.to_witness(w, P)
    run.eng.load_witness(wit)
    dev, host = str(tmp_path / "dev.wtns"), str(tmp_path / "host.wtns")
    run.eng.write_wtns(dev)
    wit.write(host, run.out.c)
    assert os.path.getsize(host) > OUT_LAPS and get(dev) == get(host)


@pytest.mark.parametrize("kind", ["constraints", "substitutions"])
def test_json_images_of_many_buffers(tmp_path, monkeypatch, run, kind):
    write = run.eng.write_constraints_json if kind == "constraints" else run.eng.write_substitution_json
    dev, host, via_host = (str(tmp_path / n) for n in ("dev.json", "host.json", "via_host.json"))
    write(dev)   # (the log goes up through StageIn first)
    assert int(run.eng.json_stats().bytes) > OUT_LAPS
    assert jsonio.host_write(kind, host, run.out.c) == 0
    monkeypatch.setenv("RS_WRITER_HOST", "1")
    write(via_host)
    assert get(dev) == get(host) == get(via_host)


def test_r1cs_image_of_many_buffers(tmp_path, monkeypatch, run):
    dev, via_host = str(tmp_path / "dev.r1cs"), str(tmp_path / "via_host.r1cs")
    run.eng.write_r1cs(dev)
    monkeypatch.setenv("RS_WRITER_HOST", "1")
    run.eng.write_r1cs(via_host)
    data = get(dev)
    assert readerio.sections(data)[2][2] > OUT_LAPS and data == get(via_host)


# --------------------------------------------------------------------------- 5. sizes at the borders
BORDERS = {"empty": 0, "less_than_a_buffer": 1000, "one_buffer": STAGE, "one_buffer_and_a_byte": STAGE + 1,
           "the_ring": 4 * STAGE, "the_ring_and_a_byte": 4 * STAGE + 1, "a_byte_short_of_five": 5 * STAGE - 1}


@pytest.mark.parametrize("name", list(BORDERS))
def test_sym_sizes_at_the_ring_borders(tmp_path, run, name):
    size = BORDERS[name]
    text = symio.line_at(size, b"") if size else symio.edge_files()["empty"][0]
    assert len(text) == size
    got, want = sym_both(run, tmp_path, text, name)
    assert got == want and (len(want) > 0) == (size > 0)


# --------------------------------------------------------------------------- 6. a refusal after the first wrap
def test_sym_refused_after_the_first_wrap(tmp_path, monkeypatch, run):
    good = symio.line_at(7 * STAGE, b"")
    at = good.index(b"\n", 5 * STAGE + 100) + 1   # a line start in the sixth piece: its buffer is on its second use
    bad = good[:at] + symio.BAD_LINES["nul"] + b"\n" + good[at:]
    src = put(tmp_path, "bad.sym", bad)
    L = abi.lib()
    codes = []
    for stage in (None, str(STAGE)):
        if stage is None:
            monkeypatch.delenv("RS_IO_STAGE")
        else:
            monkeypatch.setenv("RS_IO_STAGE", stage)
        out = str(tmp_path / f"bad.{stage}.out")
        codes.append(L.rs_engine_write_sym(run.eng._h, src.encode(), out.encode()))
        assert b"NUL" in L.rs_last_error() and not os.path.exists(out)
    assert codes == [-1, -1]
    got, want = sym_both(run, tmp_path, good, "after")
    assert got == want


def test_witness_refused_after_the_first_wrap(tmp_path, monkeypatch):
    n = 20000
    w = W.random_vector(random.Random(6), n, P)
    bad = list(w)
    bad[5 * (STAGE // 32) + 9] = P   # in the sixth piece
    raw = linear_probe(P, w, {n - 1})
    want = W.triples(abi.check_witness(W.to_witness(w, P), abi.WIT_INPUT, raw.inp))
    path = put(tmp_path, "bad.wtns", W.wtns_bytes(bad, P))
    eng = M.Engine(0)
    try:
        for stage in (None, str(STAGE)):
            if stage is None:
                monkeypatch.delenv("RS_IO_STAGE")
            else:
                monkeypatch.setenv("RS_IO_STAGE", stage)
            for load in (lambda: eng.load_wtns(path), lambda: eng.load_witness(W.to_witness(bad, P))):
                with pytest.raises(abi.RsError) as ex:
                    load()
                assert ex.value.code == -1 and "not below the prime" in str(ex.value)
                with pytest.raises(abi.RsError) as ex:   # a refused load leaves no witness resident
                    eng.check_witness(abi.WIT_INPUT, raw.inp)
                assert ex.value.code == -1 and "no witness" in str(ex.value)
        eng.load_wtns(put(tmp_path, "good.wtns", W.wtns_bytes(w, P)))
        assert W.triples(eng.check_witness(abi.WIT_INPUT, raw.inp)) == want
    finally:
        eng.close()
