"""CPU tests of the device JSON writers' boundary (rs_engine_write_constraints_json,
rs_engine_write_substitution_json, their one-shots and rs_engine_json_stats; ABI 12): the symbols exist
and are bound, null arguments are refused, without a gfx950 device the writers fail loudly and write
nothing -- there is no CPU fallback -- and the fixtures of the GPU tests (test_gpu_json.py) are pinned here
first: the host writers equal the text models on them, and the hand-built fixture covers what it says."""
import ctypes as C
import os
import random
import subprocess

import pytest

import jsonio
from circom_cvm_amd import abi

KINDS = ("constraints", "substitutions")


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_abi_binds_the_five_json_functions():
    names = {n for n, _, _ in abi.SYMBOLS}
    assert {"rs_engine_write_constraints_json", "rs_engine_write_substitution_json", "rs_write_constraints_json_device",
            "rs_write_substitution_json_device", "rs_engine_json_stats"} <= names
    L = abi.lib()
    assert L.rs_engine_write_constraints_json.argtypes[0] is C.c_void_p
    assert L.rs_engine_write_substitution_json.argtypes[0] is C.c_void_p
    assert L.rs_engine_json_stats.argtypes[0] is C.c_void_p
    assert L.rs_write_constraints_json_device.argtypes[0] is C.c_int
    assert L.rs_write_substitution_json_device.argtypes[0] is C.c_int
    for name in ("write_constraints_json", "write_substitution_json", "json_stats"):
        assert hasattr(abi.Engine, name)
    for name in ("write_constraints_json_device", "write_substitution_json_device"):
        assert hasattr(abi.Output, name)
    assert L.rs_abi_version() >= 12


def test_json_stats_fields():
    assert [k for k, _ in abi.RsJsonStats._fields_] == ["write_ms", "in_ms", "kernel_ms", "out_ms", "bytes"]
    assert [t for _, t in abi.RsJsonStats._fields_] == [C.c_double] * 4 + [C.c_uint64]
    assert C.sizeof(abi.RsJsonStats) == 40


def test_json_null_arguments_are_invalid(tmp_path):
    L = abi.lib()
    out = str(tmp_path / "o.json").encode()
    o = jsonio.random_output().out
    assert L.rs_write_constraints_json_device(0, None, C.byref(o)) == -1
    assert L.rs_write_constraints_json_device(0, out, None) == -1
    assert L.rs_write_substitution_json_device(0, None, C.byref(o)) == -1
    assert L.rs_write_substitution_json_device(0, out, None) == -1
    assert L.rs_engine_write_constraints_json(None, out) == -1
    assert L.rs_engine_write_substitution_json(None, out) == -1
    assert L.rs_engine_json_stats(None, C.byref(abi.RsJsonStats())) == -1
    assert not os.path.exists(out)


@pytest.mark.skipif(_gpu_present(), reason="checks the no-device path")
def test_device_json_writers_have_no_cpu_fallback(tmp_path):
    L = abi.lib()
    h = jsonio.random_output()
    for kind in KINDS:
        out = str(tmp_path / (kind + ".json"))
        assert jsonio.host_write(kind, str(tmp_path / ("host_" + kind)), h.out) == 0  # the host writer needs no device
        assert jsonio.device_write(kind, out, h.out) == -6
        assert b"gfx950" in L.rs_last_error() or b"device" in L.rs_last_error().lower()
        assert not os.path.exists(out)
    for f in (abi.Output.write_constraints_json_device, abi.Output.write_substitution_json_device):
        out = str(tmp_path / "wrapped.json")
        with pytest.raises(abi.RsError) as e:
            f(out, h.out)
        assert e.value.code == -6 and not os.path.exists(out)
    # the engine writers need an engine, and there is none to be had
    eng = C.c_void_p()
    assert L.rs_engine_create(0, C.byref(eng)) == -6


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["digit", "random_O1", "random_O2", "empty"])
def test_host_writers_equal_the_models(tmp_path, name, kind):
    h = {"digit": jsonio.digit_output, "empty": jsonio.empty_output,
         "random_O1": lambda: jsonio.random_output(level="O1"), "random_O2": jsonio.random_output}[name]()
    path = str(tmp_path / "host.json")
    assert jsonio.host_write(kind, path, h.out) == 0
    got, want = jsonio.get(path), jsonio.model(kind, h)
    assert len(got) == len(want) and got == want
    assert got.startswith(jsonio.HEAD[kind]) and got.endswith(jsonio.TAIL[kind])
    if name == "empty":
        assert got == jsonio.HEAD[kind] + jsonio.TAIL[kind]
    else:
        assert len(got) > 100


def test_fixture_covers_every_length():
    h = jsonio.digit_output()
    vals = {len(str(v)) for r in h.rows for part in r for _, v in part}
    assert vals == set(range(1, 79))
    assert {len(str(v)) for _, to in h.log for _, v in to} == set(range(1, 79))
    assert {len(str(k)) for r in h.rows for part in r for k, _ in part} == set(range(1, 9))
    assert {len(str(k)) for _, to in h.log for k, _ in to} == set(range(1, 11))
    assert {len(str(f)) for f, _ in h.log} == set(range(1, 11))
    assert set(jsonio.VALUES) <= {v for r in h.rows for part in r for _, v in part}
    sizes = {len(part) for r in h.rows for part in r}
    assert set(jsonio.PART_SIZES) | {jsonio.BIG_ROW} <= sizes
    assert {len(to) for _, to in h.log} >= set(jsonio.PART_SIZES) | {jsonio.BIG_ROW}
    assert h.rows[0] == ([], [], []) and h.rows[-1] == ([], [], [])
    # the long row is more than four chunks at the largest chunk size swept and at the default
    assert jsonio.DEFAULT_CHUNK in jsonio.SWEPT_CHUNKS
    assert jsonio.big_row_text_len(h) > 4 * max(max(jsonio.SWEPT_CHUNKS), jsonio.DEFAULT_CHUNK)


def test_fixture_puts_every_byte_class_on_every_offset_of_a_64_byte_chunk():
    """In the images (the files less their opening strings: chunks count from the image's first byte) of the
    two model texts together, every class of byte meets every offset 0..63."""
    h = jsonio.digit_output()
    seen = {c: set() for c in ("bracket", "brace", "comma", "quote", "colon", "key digit", "value digit", "newline")}
    simple = {ord("["): "bracket", ord("]"): "bracket", ord("{"): "brace", ord("}"): "brace", ord(","): "comma",
              ord('"'): "quote", ord(":"): "colon", ord("\n"): "newline"}
    for kind in KINDS:
        text = jsonio.model(kind, h)
        img = text[len(jsonio.HEAD[kind]):len(text) - len(jsonio.TAIL[kind])]
        for i, b in enumerate(img):
            if b in simple:
                seen[simple[b]].add(i % 64)
            elif 48 <= b <= 57:
                # a digit run that ends in `":` or `" :` is a key (or a log entry's `from`), else a value
                j = i
                while 48 <= img[j] <= 57:
                    j += 1
                seen["key digit" if img[j:j + 2] in (b'":', b'" ') else "value digit"].add(i % 64)
            else:
                assert b == ord(" "), (kind, i, b)
    for c, offs in seen.items():
        assert offs == set(range(64)), (c, sorted(set(range(64)) - offs))


def test_conversion_helpers_on_the_host(tmp_path):
    """json_dec / json_dig32 (csrc/json_write.hpp), the kernels' 256-bit binary -> decimal conversion,
    compiled for the host into a stand-alone program under the address and undefined-behaviour sanitizers:
    every fixture value, every 10^k - 1 / 10^k, and random values of every bit length."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "json_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wno-unknown-pragmas", "-I", os.path.join(root, "circom_cvm_amd", "csrc"),
                           os.path.join(root, "tests", "json_host_check.cpp"), "-o", exe])
    rng = random.Random(5)
    vals = list(jsonio.VALUES) + [10 ** k for k in range(78)] + [rng.getrandbits(b) for b in range(1, 257) for _ in range(8)]
    text = "".join(" ".join("%x" % ((v >> (64 * i)) & abi.U64_MAX) for i in range(4)) + "\n" for v in vals)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(vals)
    for v, line in zip(vals, got):
        assert line == f"{v} {len(str(v))}", v


def test_bad_outputs_are_what_they_say():
    bad = jsonio.bad_outputs()
    assert len(bad) == 3 * 4 + 3 * 2 + 1
    for name, (h, code) in bad.items():
        assert code in (-1, -5)
        if code == -5:  # the host writer refuses a removed or out-of-range signal too
            assert not name.startswith("log_")
    assert bad["removed_and_swapped"][1] == -5


@pytest.mark.parametrize("name", sorted(n for n, (_, code) in jsonio.bad_outputs().items() if code == -5))
def test_host_writer_refuses_removed_signals(tmp_path, name):
    h, _ = jsonio.bad_outputs()[name]
    assert jsonio.host_write("constraints", str(tmp_path / "o.json"), h.out) == -5
