"""Helpers of the .sym writers' tests (test_sym_abi.py, test_gpu_sym.py): a seeded generator of --O0
.sym texts with their label_to_wire arrays, the files the device writer must refuse, and the
split-on-newline model of the rewrite (constraint_list/src/sym_porting.rs:5-37: column 2 of every
line becomes label_to_wire[column 1], -1 for a label the map does not hold)."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np

CHUNK = 4096  # the device writer's default RS_SYM_CHUNK; 64 is its minimum (both are tested)

# label_to_wire values of every decimal length, 1 .. 10 bytes (and "-1")
WIRES = [-1, 0] + [x for k in range(1, 10) for x in (10 ** k - 1, 10 ** k)] + [2147483646]


def model(data: bytes, l2w) -> bytes:
    """What every writer must produce for a file in the accepted grammar."""
    out = []
    for line in data.split(b"\n"):
        if not line:
            continue
        lab, _w, rest = line.split(b",", 2)
        w = int(l2w[int(lab)]) if int(lab) < len(l2w) else -1
        out.append(b"%d,%d,%s\n" % (int(lab), w, rest))
    return b"".join(out)


def old_w(k: int) -> bytes:
    """An old witness column: k + 1 digits for k = 0 .. 9, -1 for k = 10."""
    return b"-1" if k == 10 else (b"%d" % (k % 9 + 1)) + b"7" * k


def gen_valid(seed: int, n_lines: int = 3000):
    """(text, label_to_wire): labels shuffled, a few of them >= n_labels; old W of every width with new W of
    every width (210 = 10 * 21 lines hold every pair, so delta takes every value -9 .. +9); name lengths
    cycling 0 .. 66, so every field boundary meets every offset of a 64-byte chunk; some names of 300
    bytes (whole chunks inside one name), names made of digits and commas, an empty name, an empty rest."""
    rng = random.Random(seed)
    n_labels = n_lines + 1
    labels = list(range(1, n_labels + 40))  # the last 40 labels are past the map
    rng.shuffle(labels)
    labels = labels[:n_lines]
    l2w = np.full(n_labels, -1, np.int32)
    lines = []
    for k, lab in enumerate(labels):
        if lab < n_labels:
            l2w[lab] = WIRES[k % len(WIRES)]
        w = old_w(k % 10 if k % 23 else 10)
        n = k % 67
        if k % 97 == 5:
            name = b"main." + b"q" * 295
        elif k % 97 == 6:
            name = b"1,2,3,"
        elif k % 97 == 7:
            name = b",5,6,7"
        elif k % 97 == 8:
            name = b""
        else:
            name = (b"main.s[%d].x" % k + b"abcdefghij" * 7)[:n]
        if k % 97 == 9:
            lines.append(b"%d,%s," % (lab, w))  # an empty rest
        else:
            lines.append(b"%d,%s,%d,%s" % (lab, w, k % 3, name))
    return b"".join(x + b"\n" for x in lines), l2w


def line_at(target: int, text: bytes) -> bytes:
    """`text` (whole lines) extended by valid lines to exactly `target` bytes."""
    assert text == b"" or text.endswith(b"\n")
    k = 0
    while len(text) < target - 90:
        text += b"%d,%d,1,main.pad[%d]\n" % (k % 50, k, k)
        k += 1
    fill = target - len(text) - len(b"7,1,0,\n")
    assert fill >= 0
    return text + b"7,1,0," + b"p" * fill + b"\n"


def small_l2w():
    return np.array([WIRES[(3 * i) % len(WIRES)] for i in range(50)], np.int32)


def edge_files():
    """name -> (text, label_to_wire): the grammar's corners."""
    l2w = small_l2w()
    one = b"3,3,1,main.in[1]\n"
    body = b"1,1,1,main.out\n2,22,1,main.in[0]\n49,333,0,main.c.out\n50,4,0,main.past_the_map\n"
    return {
        "empty": (b"", l2w),
        "newlines_only": (b"\n\n", l2w),
        "one_line": (one, l2w),
        "no_trailing_newline": (body + one[:-1], l2w),
        "one_line_no_newline": (one[:-1], l2w),
        "second_comma_last": (body + b"9,12,", l2w),
        "empty_lines": (b"\n\n" + body + b"\n\n" + body + b"\n\n\n", l2w),
        "line_at_chunk_boundary": (line_at(CHUNK, b"") + body + one, l2w),
        "empty_line_at_chunk_boundary": (line_at(CHUNK, b"") + b"\n" + body, l2w),
        "w_across_chunk_boundary": (line_at(CHUNK - 4, b"") + b"12,1234567890,1,main.x\n" + body, l2w),
    }


def valid_files():
    out = {"random_%d" % s: gen_valid(s) for s in (1, 2)}
    out.update(edge_files())
    return out


# every kind of line the device writer refuses (the host writer refuses only the first two)
BAD_LINES = {
    "no_comma": b"main.x",
    "one_comma": b"5,3",
    "leading_zero_L": b"05,3,1,main.a",
    "blank_L": b" 5,3,1,main.a",
    "empty_L": b",3,1,main.a",
    "non_numeric_L": b"x5,3,1,main.a",
    "L_11_digits": b"12345678901,3,1,main.a",
    "empty_W": b"5,,1,main.a",
    "minus_only_W": b"5,-,1,main.a",
    "non_numeric_W": b"5,3x,1,main.a",
    "W_11_digits": b"5,12345678901,1,main.a",
    "nul": b"5,3,1,ma\x00in.a",
}


def bad_files():
    """name -> text: each refused kind mid-file, straddling a chunk boundary (of 4096 bytes, so of 64
    too), and as the last line without a newline."""
    good, _ = gen_valid(3, 200)
    half = good[:good.index(b"\n", len(good) // 2) + 1]
    out = {}
    for kind, bad in BAD_LINES.items():
        out[kind + "/mid"] = half + bad + b"\n" + good[len(half):]
        pre = line_at(CHUNK - 2, b"")
        assert len(pre) < CHUNK < len(pre) + len(bad)
        out[kind + "/straddle"] = pre + bad + b"\n" + good
        out[kind + "/last"] = good + bad
    return out


# ---- the library's writers on files
def out_struct(l2w):
    """An otherwise zeroed rs_output that holds n_labels and label_to_wire (the array must stay alive)."""
    from circom_cvm_amd import abi
    o = abi.RsOutput()
    o.n_labels = len(l2w)
    o.label_to_wire = l2w.ctypes.data_as(C.POINTER(C.c_int32))
    return o


def host_write(o0_sym: str, path: str, l2w) -> int:
    from circom_cvm_amd import abi
    l2w = np.ascontiguousarray(l2w, np.int32)
    return abi.lib().rs_write_sym(o0_sym.encode(), path.encode(), C.byref(out_struct(l2w)))


def device_write(o0_sym: str, path: str, l2w, device: int = 0) -> int:
    from circom_cvm_amd import abi
    l2w = np.ascontiguousarray(l2w, np.int32)
    return abi.lib().rs_write_sym_device(device, o0_sym.encode(), path.encode(), C.byref(out_struct(l2w)))
