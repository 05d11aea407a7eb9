"""CPU tests of the device .sym writer's boundary (rs_engine_write_sym, rs_write_sym_device; ABI 11):
the symbols exist and are bound, null arguments are refused, without a gfx950 device the writer fails
loudly and writes nothing -- there is no CPU fallback -- and the fixtures of its GPU tests
(test_gpu_sym.py) are pinned here first: the host writer rs_write_sym equals the split-on-newline model
on every generated valid file."""
import ctypes as C
import os

import pytest

import symio
from circom_cvm_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS = os.path.join(ROOT, "tests", "golden", "docs_basic_O0.sym")


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_abi_binds_both_sym_functions():
    names = {n for n, _, _ in abi.SYMBOLS}
    assert {"rs_engine_write_sym", "rs_write_sym_device"} <= names
    L = abi.lib()
    assert L.rs_engine_write_sym.argtypes[0] is C.c_void_p
    assert L.rs_write_sym_device.argtypes[0] is C.c_int
    assert hasattr(abi.Engine, "write_sym") and hasattr(abi.Output, "write_sym_device")
    assert L.rs_abi_version() >= 11
    fields = [k for k, _ in abi.RsStats._fields_]
    assert fields[-4:] == ["sym_write_ms", "sym_in_ms", "sym_kernel_ms", "sym_out_ms"]


def test_sym_null_arguments_are_invalid(tmp_path):
    L = abi.lib()
    out = str(tmp_path / "o.sym").encode()
    l2w = symio.small_l2w()
    o = symio.out_struct(l2w)
    assert L.rs_write_sym_device(0, None, out, C.byref(o)) == -1
    assert L.rs_write_sym_device(0, DOCS.encode(), None, C.byref(o)) == -1
    assert L.rs_write_sym_device(0, DOCS.encode(), out, None) == -1
    assert L.rs_engine_write_sym(None, DOCS.encode(), out) == -1
    assert not os.path.exists(out)


@pytest.mark.skipif(_gpu_present(), reason="checks the no-device path")
def test_device_sym_writer_has_no_cpu_fallback(tmp_path):
    L = abi.lib()
    out = str(tmp_path / "o.sym")
    l2w = symio.small_l2w()
    assert symio.host_write(DOCS, str(tmp_path / "h.sym"), l2w) == 0  # the host writer needs no device
    assert symio.device_write(DOCS, out, l2w) == -6
    assert b"gfx950" in L.rs_last_error() or b"device" in L.rs_last_error().lower()
    assert not os.path.exists(out)
    with pytest.raises(abi.RsError) as e:
        abi.Output.write_sym_device(DOCS, out, symio.out_struct(l2w))
    assert e.value.code == -6 and not os.path.exists(out)


@pytest.mark.parametrize("name", sorted(symio.valid_files()))
def test_host_writer_equals_the_model(tmp_path, name):
    text, l2w = symio.valid_files()[name]
    src, dst = str(tmp_path / "in.sym"), str(tmp_path / "out.sym")
    with open(src, "wb") as f:
        f.write(text)
    assert symio.host_write(src, dst, l2w) == 0
    with open(dst, "rb") as f:
        assert f.read() == symio.model(text, l2w)


def test_generated_files_cover_every_delta():
    text, l2w = symio.gen_valid(1)
    deltas = set()
    for line in text.split(b"\n"):
        if line:
            lab, w, _ = line.split(b",", 2)
            new = int(l2w[int(lab)]) if int(lab) < len(l2w) else -1
            deltas.add(len(str(new)) - len(w))
    assert deltas == set(range(-9, 10))
    assert any(int(line.split(b",")[0]) >= len(l2w) for line in text.split(b"\n") if line)


def test_host_writer_refuses_fewer_than_two_commas(tmp_path):
    for kind in ("no_comma", "one_comma"):
        src, dst = str(tmp_path / (kind + ".sym")), str(tmp_path / (kind + ".out"))
        with open(src, "wb") as f:
            f.write(symio.bad_files()[kind + "/mid"])
        assert symio.host_write(src, dst, symio.small_l2w()) == -1
