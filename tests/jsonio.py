"""Helpers of the JSON writers' tests (test_json_abi.py, test_gpu_json.py): wrappers of the host and the
device writers of <prefix>_constraints.json and <prefix>_substitutions.json, the text models (rsio's
restatements of json_porting.rs / json_writer.rs), a hand-built rs_output whose values, wires and log
keys take every decimal length at every row-part size the formatter treats differently, and the outputs
the device writers must refuse."""
from __future__ import annotations

import ctypes as C

import numpy as np

import rsio
from circom_cvm_amd import abi

R = rsio.R

DEFAULT_CHUNK = 16384                        # the device writers' default RS_JSON_CHUNK
SWEPT_CHUNKS = (4096, 8192, 16384, 32768, 65536)
HEAD = {"constraints": b'{\n"constraints": [', "substitutions": b"{"}
TAIL = {"constraints": b"\n]\n}", "substitutions": b"\n}"}

VALUES = ([0, 1, 9]
          + [10 ** k + d for k in range(1, 78) for d in (-1, 0, 1)]
          + [10 ** 38 + 1, 10 ** 57 + 10 ** 19]                    # zero 9-digit chunks inside
          + [2 ** 32 - 1, 2 ** 32, 2 ** 64 - 1, 2 ** 64, 2 ** 128 - 1, 2 ** 128, 2 ** 192 - 1, 2 ** 192, 2 ** 256 - 1]
          + [p - 1 for p in R.PRIMES.values()])
LONG_VALUES = [v for v in VALUES if len(str(v)) >= 76]
N_LABELS = 10_000_001
WIRE_KEYS = sorted({0, 10_000_000} | {10 ** k - 1 for k in range(1, 8)} | {10 ** k for k in range(1, 8)})
LOG_KEYS = sorted({0, 2 ** 32 - 1} | {10 ** k - 1 for k in range(1, 10)} | {10 ** k for k in range(1, 10)})
PART_SIZES = (0, 1, 2, 63, 64, 65)
BIG_ROW = 3000


class Ident:
    """label_to_wire = the identity, as a mapping."""

    def __getitem__(self, k):
        return k


class Block:
    """A CSR rs_lc over numpy arrays from rows given as lists of (key, value), in the order given."""

    def __init__(self, rows):
        ptr = np.zeros(len(rows) + 1, np.uint64)
        np.cumsum([len(r) for r in rows], out=ptr[1:])
        keys = [k for r in rows for k, _ in r]
        vals = [(v >> (64 * i)) & abi.U64_MAX for r in rows for _, v in r for i in range(4)]
        self.ptr = ptr
        self.col = np.array(keys or [0], np.uint32)
        self.val = np.array(vals or [0, 0, 0, 0], np.uint64)
        self.lc = abi.RsLc(len(rows), len(keys), self.ptr.ctypes.data_as(C.POINTER(C.c_uint64)),
                           self.col.ctypes.data_as(C.POINTER(C.c_uint32)), self.val.ctypes.data_as(C.POINTER(C.c_uint64)))


class Holder:
    """An rs_output over numpy arrays (kept alive here): constraint rows as (a, b, c) lists of
    (key, value), label_to_wire, and the log as [(from, [(key, value)])]."""

    def __init__(self, rows, l2w, log=()):
        self.rows, self.log = list(rows), list(log)
        self.blocks = [Block([r[q] for r in self.rows]) for q in range(3)]
        self.l2w = np.ascontiguousarray(l2w, np.int32)
        self.log_blk = Block([to for _, to in self.log])
        self.log_from = np.array([f for f, _ in self.log] or [0], np.uint32)
        o = abi.RsOutput()
        o.n_constraints = len(self.rows)
        o.a, o.b, o.c = [b.lc for b in self.blocks]
        o.n_labels = len(self.l2w)
        o.label_to_wire = self.l2w.ctypes.data_as(C.POINTER(C.c_int32))
        o.n_wires = int((self.l2w >= 0).sum())
        o.n_log = len(self.log)
        o.log_from = self.log_from.ctypes.data_as(C.POINTER(C.c_uint32))
        o.log_to = self.log_blk.lc
        self.out = o

    def cons(self):
        return [R.Con(dict(a), dict(b), dict(c)) for a, b, c in self.rows]

    def wires(self):
        if np.array_equal(self.l2w, np.arange(len(self.l2w))):
            return Ident()
        return {i: int(w) for i, w in enumerate(self.l2w)}

    def constraints_text(self) -> bytes:
        return rsio.constraints_json_text(self.cons(), self.wires()).encode()

    def substitutions_text(self) -> bytes:
        return rsio.substitutions_json_text([(f, dict(to)) for f, to in self.log]).encode()


def _rows(special, n_small):
    """Row parts of every size in PART_SIZES over keys that hold `special`, the BIG_ROW row, n_small rows
    of 0 - 2 entries a part (so that every kind of byte meets every offset of a 64-byte chunk), an empty
    row first and last.  The values cycle through VALUES."""
    pool = sorted(set(special) | set(range(200, 260)))
    assert len(pool) >= 65
    nv = [0]

    def part(m, off):
        keys = sorted(pool[(off + i) % len(pool)] for i in range(m))
        out = []
        for k in keys:
            out.append((k, VALUES[nv[0] % len(VALUES)]))
            nv[0] += 1
        return out

    rows = [([], [], [])]
    for i in range(6):
        rows.append(tuple(part(PART_SIZES[(i + q) % 6], 7 * i + 3 * q) for q in range(3)))
    big = [(1_000_000 + 3 * i, LONG_VALUES[i % len(LONG_VALUES)]) for i in range(BIG_ROW)]
    rows.append((big, part(1, 0), []))
    for i in range(6):
        rows.append(tuple(part(PART_SIZES[(i + 2 * q + 1) % 6], 5 * i + q + 11) for q in range(3)))
    for i in range(n_small):
        rows.append(tuple(part((i + q + i // 3) % 3, i + 5 * q) for q in range(3)))
    rows.append(([], [], []))
    return rows


_DIGIT = None


def digit_output() -> Holder:
    """The fixture of the value, wire and log-key lengths (built once, never modified)."""
    global _DIGIT
    if _DIGIT is None:
        rows = _rows(WIRE_KEYS, 700)
        lrows = _rows(LOG_KEYS, 700)
        log = []
        for i, r in enumerate(lrows):
            for q in range(3):
                log.append((LOG_KEYS[(3 * i + q) % len(LOG_KEYS)], r[q]))
        _DIGIT = Holder(rows, np.arange(N_LABELS, dtype=np.int32), log)
    return _DIGIT


def big_row_text_len(h: Holder) -> int:
    a, b, c = next(r for r in h.rows if len(r[0]) == BIG_ROW)
    return len(",\n[" + ",".join(rsio.json_map(dict(m)) for m in (a, b, c)) + "]")


def empty_output() -> Holder:
    return Holder([], np.arange(4, dtype=np.int32), [])


def random_output(seed=131, level="O2") -> Holder:
    """The pyref result and log of a random system as a Holder."""
    sys_ = rsio.gen_system(seed, R.PRIMES["bn128"], n_sig=60, n_rows=80)
    res = R.simplification(sys_, R.Flags(flag_s=level == "O1", no_rounds=0 if level == "O1" else (1 << 64) - 1), want_log=True)
    l2w = np.array([res.signal_map.get(i, -1) for i in range(sys_.max_signal)], np.int32)
    rows = [tuple(sorted(m.items()) for m in (c.a, c.b, c.c)) for c in res.constraints]
    return Holder(rows, l2w, [(s.frm, sorted(s.to.items())) for s in res.log])


def _small_rows():
    return [tuple([(1 + j + 3 * q + 9 * r, 5 + r + j) for j in range(3)] for q in range(3)) for r in range(5)]


def bad_outputs():
    """name -> (Holder, the code both device writers' contract gives it).  Constraint outputs with a used
    key whose label_to_wire is -1, a key = n_labels, two keys of a part swapped, a key twice -- each in the
    first, a middle and the last row -- and one with a removed signal and a swapped pair; logs with a
    swapped pair and a key twice at the same places (a log has no removed signals)."""
    out = {}
    n_labels = 64
    for where, r in (("first", 0), ("mid", 2), ("last", 4)):
        for kind in ("removed", "past", "swapped", "twice"):
            rows, l2w = _small_rows(), np.arange(n_labels, dtype=np.int32)
            part = rows[r][1]
            if kind == "removed":
                l2w[part[1][0]] = -1
            elif kind == "past":
                part[2] = (n_labels, part[2][1])
            elif kind == "swapped":
                part[0], part[1] = part[1], part[0]
            else:
                part[2] = (part[1][0], part[2][1])
            out[f"{kind}/{where}"] = (Holder(rows, l2w), -5 if kind in ("removed", "past") else -1)
        for kind in ("swapped", "twice"):
            log = [(7 + i, list(rw[0])) for i, rw in enumerate(_small_rows())]
            to = log[r][1]
            if kind == "swapped":
                to[1], to[2] = to[2], to[1]
            else:
                to[1] = (to[0][0], to[1][1])
            out[f"log_{kind}/{where}"] = (Holder([], np.arange(4, dtype=np.int32), log), -1)
    rows, l2w = _small_rows(), np.arange(n_labels, dtype=np.int32)
    rows[1][0][0], rows[1][0][1] = rows[1][0][1], rows[1][0][0]
    l2w[rows[3][2][1][0]] = -1
    out["removed_and_swapped"] = (Holder(rows, l2w), -5)
    return out


# ---- the library's writers on files
def host_write(kind: str, path: str, out) -> int:
    f = abi.lib().rs_write_constraints_json if kind == "constraints" else abi.lib().rs_write_substitution_json
    return f(path.encode(), C.byref(out))


def device_write(kind: str, path: str, out, device: int = 0) -> int:
    L = abi.lib()
    f = L.rs_write_constraints_json_device if kind == "constraints" else L.rs_write_substitution_json_device
    return f(device, path.encode(), C.byref(out))


def model(kind: str, h: Holder) -> bytes:
    return h.constraints_text() if kind == "constraints" else h.substitutions_text()


def get(path) -> bytes:
    with open(path, "rb") as f:
        return f.read()
