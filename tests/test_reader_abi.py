"""CPU tests of the device --O0 reader's boundary (rs_engine_read_r1cs_o0, rs_read_r1cs_o0_device;
ABI 10): the symbols exist and are bound, null arguments are refused, and without a gfx950 device the
reader fails loudly -- there is no CPU fallback.  Its results are checked on the GPU
(test_gpu_reader.py)."""
import ctypes as C
import os

import pytest

import readerio
from circom_cvm_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS = os.path.join(ROOT, "tests", "golden", "docs_basic_O0.r1cs")


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_abi_binds_both_reader_functions():
    names = {n for n, _, _ in abi.SYMBOLS}
    assert {"rs_engine_read_r1cs_o0", "rs_read_r1cs_o0_device"} <= names
    L = abi.lib()
    assert L.rs_engine_read_r1cs_o0.argtypes[0] is C.c_void_p
    assert L.rs_read_r1cs_o0_device.argtypes[0] is C.c_int
    assert hasattr(abi.Engine, "read_r1cs") and hasattr(abi.Input, "read_r1cs_device")
    assert L.rs_abi_version() >= 10


def test_reader_null_arguments_are_invalid():
    L = abi.lib()
    p = C.POINTER(abi.RsInput)()
    assert L.rs_read_r1cs_o0_device(0, None, C.byref(p)) == -1
    assert L.rs_read_r1cs_o0_device(0, DOCS.encode(), None) == -1
    assert L.rs_engine_read_r1cs_o0(None, DOCS.encode(), C.byref(p)) == -1
    assert not p


@pytest.mark.skipif(_gpu_present(), reason="checks the no-device path")
def test_device_reader_has_no_cpu_fallback():
    L = abi.lib()
    assert readerio.host_read(DOCS)[0] == 0  # the host reader needs no device
    p = C.POINTER(abi.RsInput)()
    rc = L.rs_read_r1cs_o0_device(0, DOCS.encode(), C.byref(p))
    assert rc == -6 and not p
    assert b"gfx950" in L.rs_last_error() or b"device" in L.rs_last_error().lower()
    with pytest.raises(abi.RsError) as e:
        abi.Input.read_r1cs_device(DOCS)
    assert e.value.code == -6
