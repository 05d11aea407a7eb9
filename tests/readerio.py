"""Helpers of the device --O0 reader's tests (test_reader_abi.py, test_gpu_reader.py): the one
comparison of two rs_input structs, field for field and array for array, and -- run as a script -- a
child process that reads files with both readers under the environment its parent gave it (the
RS_R1CS_CHUNK / RS_R1CS_GROUP sizes), on ONE engine:

    python readerio.py <good.r1cs> <file> [<file> ...]

prints one JSON line: per file the host reader's status, the device reader's status, their difference
(None: equal) and, after every file, whether the same engine still reads <good.r1cs> correctly."""
from __future__ import annotations

import ctypes as C
import json
import os
import struct
import sys

import numpy as np

BLOCKS = ("cons_eq", "eq", "linear", "nl_a", "nl_b", "nl_c")
SCALARS = ("prime_id", "max_signal", "n_pub_out", "n_pub_in", "n_priv_in", "n_forbidden")


def input_arrays(x) -> dict:
    """Every field of an rs_input, arrays copied (numpy)."""
    d = {k: int(getattr(x, k)) for k in SCALARS}
    d["prime"] = [int(v) for v in x.prime]
    nf = int(x.n_forbidden)
    d["forbidden"] = np.ctypeslib.as_array(x.forbidden, shape=(max(nf, 1),))[:nf].copy()
    for nm in BLOCKS:
        b = getattr(x, nm)
        n, nnz = int(b.n_rows), int(b.nnz)
        d[nm] = (n, nnz,
                 np.ctypeslib.as_array(b.ptr, shape=(n + 1,)).copy(),
                 np.ctypeslib.as_array(b.col, shape=(max(nnz, 1),))[:nnz].copy(),
                 np.ctypeslib.as_array(b.val, shape=(max(nnz, 1) * 4,))[:4 * nnz].copy())
    return d


def diff_inputs(x: dict, y: dict) -> str | None:
    """The first difference between two input_arrays() results (None: equal)."""
    for k in SCALARS + ("prime",):
        if x[k] != y[k]:
            return f"{k}: {x[k]} vs {y[k]}"
    if not np.array_equal(x["forbidden"], y["forbidden"]):
        return "forbidden differs"
    for nm in BLOCKS:
        if x[nm][0] != y[nm][0] or x[nm][1] != y[nm][1]:
            return f"{nm}: {x[nm][0]} rows / {x[nm][1]} entries vs {y[nm][0]} / {y[nm][1]}"
        for i, part in ((2, "ptr"), (3, "col"), (4, "val")):
            if not np.array_equal(x[nm][i], y[nm][i]):
                return f"{nm}.{part} differs at {int(np.argmax(x[nm][i] != y[nm][i]))}"
    return None


def host_read(path):
    """(status, input_arrays or None) of rs_read_r1cs_o0."""
    from circom_cvm_amd import abi
    p = C.POINTER(abi.RsInput)()
    rc = abi.lib().rs_read_r1cs_o0(path.encode(), C.byref(p))
    if rc:
        return rc, None
    try:
        return 0, input_arrays(p.contents)
    finally:
        abi.lib().rs_input_free(p)


def engine_read(eng, path):
    """(status, input_arrays or None) of rs_engine_read_r1cs_o0 on `eng`."""
    from circom_cvm_amd import abi
    p = C.POINTER(abi.RsInput)()
    rc = abi.lib().rs_engine_read_r1cs_o0(eng._h, path.encode(), C.byref(p))
    return rc, (input_arrays(p.contents) if rc == 0 else None)


def compare_readers(eng, path):
    """{"host": rc, "dev": rc, "diff": str | None} for one file."""
    hrc, h = host_read(path)
    drc, d = engine_read(eng, path)
    diff = None
    if hrc == 0 and drc == 0:
        diff = diff_inputs(h, d)
    return {"host": hrc, "dev": drc, "diff": diff}


# ---- locating the constraint section and its linear combinations in a file's bytes
def sections(data: bytes) -> dict:
    """type -> (offset of the section's size field, offset of its body, size), from the section table."""
    out = {}
    off = 12
    for _ in range(struct.unpack_from("<I", data, 8)[0]):
        t, sz = struct.unpack_from("<IQ", data, off)
        out.setdefault(t, (off + 4, off + 12, sz))
        off += 12 + sz
    return out


def lc_offsets(data: bytes) -> list:
    """File offsets of the count fields of the 3 * n_cons linear combinations, in order."""
    sec = sections(data)
    fs = struct.unpack_from("<I", data, sec[1][1])[0]
    n_cons = struct.unpack_from("<I", data, sec[1][1] + 4 + fs + 16 + 8)[0]
    off = sec[2][1]
    out = []
    for _ in range(3 * n_cons):
        out.append(off)
        off += 4 + struct.unpack_from("<I", data, off)[0] * (4 + fs)
    return out


def main(argv):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import circom_cvm_amd as M
    good, files = argv[0], argv[1:]
    eng = M.Engine(0)
    want = host_read(good)[1]
    res = []
    for f in files:
        r = compare_readers(eng, f)
        rc, got = engine_read(eng, good)
        r["good_after"] = rc == 0 and diff_inputs(want, got) is None
        res.append(r)
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1:])
