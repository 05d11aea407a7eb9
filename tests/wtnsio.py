"""Helpers of the witness tests (test_wtns_abi.py, test_gpu_wtns.py): .wtns bytes built with struct,
independently of the library; witness <-> rs_witness; a Python evaluator of a witness that returns the
report triple per class (soundness.holds for rows, the log rule of soundness.check_witnesses); the table
of malformed files; and hand-built rs_inputs for the chunk-border and limb-edge cases."""
from __future__ import annotations

import ctypes as C
import random
import struct

import numpy as np

import rsio
import soundness as S
from circom_cvm_amd import abi

R = rsio.R
NONE = abi.U64_MAX
CLASSES = abi.WIT_CLASSES
ALL = abi.WIT_INPUT | abi.WIT_OUTPUT | abi.WIT_LOG


# --------------------------------------------------------------------------- the file format
def n8_of(p: int) -> int:
    bits = p.bit_length()
    return bits // 8 if bits % 64 == 0 else (bits // 64 + 1) * 8


def section(sid: int, body: bytes, length=None) -> bytes:
    return struct.pack("<IQ", sid, len(body) if length is None else length) + body


def sec1(p: int, n8: int, nvars: int) -> bytes:
    return struct.pack("<I", n8) + p.to_bytes(n8, "little") + struct.pack("<I", nvars)


def sec2(values, n8: int) -> bytes:
    return b"".join(v.to_bytes(n8, "little") for v in values)


def wtns_bytes(values, p: int, n8=None, order=(1, 2), between=None, version=2) -> bytes:
    """The .wtns of `values` over F_p; order: the sections' order; between: an unknown section
    (id, body) placed between them."""
    n8 = n8_of(p) if n8 is None else n8
    secs = {1: section(1, sec1(p, n8, len(values))), 2: section(2, sec2(values, n8))}
    parts = [secs[order[0]]] + ([section(*between)] if between else []) + [secs[order[1]]]
    return b"wtns" + struct.pack("<II", version, len(parts)) + b"".join(parts)


def parse_wtns(data: bytes):
    """-> (p, n8, values) of a well-formed file (sections 1 then 2)."""
    assert data[:4] == b"wtns" and struct.unpack_from("<II", data, 4) == (2, 2)
    sid, ln = struct.unpack_from("<IQ", data, 12)
    assert sid == 1
    n8 = struct.unpack_from("<I", data, 24)[0]
    assert ln == 8 + n8
    p = int.from_bytes(data[28:28 + n8], "little")
    nv = struct.unpack_from("<I", data, 28 + n8)[0]
    off = 32 + n8
    sid, ln = struct.unpack_from("<IQ", data, off)
    assert sid == 2 and ln == n8 * nv and len(data) == off + 12 + ln
    off += 12
    return p, n8, [int.from_bytes(data[off + n8 * i: off + n8 * (i + 1)], "little") for i in range(nv)]


def malformed(p: int = R.PRIMES["bn128"]):
    """{name: (bytes, a word of the message that names the cause)}"""
    n8 = n8_of(p)
    vals = [1, 5, p - 1, 7]
    good = wtns_bytes(vals, p)
    s1, s2 = section(1, sec1(p, n8, 4)), section(2, sec2(vals, n8))
    head = lambda n: b"wtns" + struct.pack("<II", 2, n)
    out = {
        "bad_magic": (b"wtnz" + good[4:], "magic"),
        "r1cs_magic": (b"r1cs" + good[4:], "magic"),
        "version_1": (wtns_bytes(vals, p, version=1), "version"),
        "version_3": (wtns_bytes(vals, p, version=3), "version"),
        "no_section_1": (head(1) + s2, "section 1 is missing"),
        "no_section_2": (head(1) + s1, "section 2 is missing"),
        "no_sections": (head(0), "missing"),
        "two_section_1": (head(3) + s1 + s1 + s2, "twice"),
        "two_section_2": (head(3) + s1 + s2 + s2, "twice"),
        "section_2_past_file": (head(2) + s1 + section(2, sec2(vals, n8), length=n8 * 4 + 1), "past the end"),
        "section_1_past_file": (head(2) + section(1, sec1(p, n8, 4), length=1 << 40) + s2, "past the end"),
        "unknown_past_file": (head(3) + s1 + section(9, b"xy", length=1 << 62) + s2, "past the end"),
        "table_past_file": (head(3) + s1 + s2, "past the end"),
        "table_cut": (head(3) + s1 + s2 + b"\x07\x00\x00", "past the end"),
        "n8_12": (head(2) + section(1, sec1(p % (1 << 96) | 1, 12, 4)) + section(2, sec2(vals[:2] + [3, 7], 12)), "n8"),
        "n8_0": (head(2) + section(1, struct.pack("<II", 0, 4)) + section(2, b""), "n8"),
        "n8_40": (head(2) + section(1, sec1(p, 40, 4)) + section(2, sec2(vals, 40)), "n8"),
        "n8_huge": (head(2) + section(1, struct.pack("<I", 0xfffffff8) + p.to_bytes(32, "little") + struct.pack("<I", 4)) + s2, "n8"),
        "section_1_long": (head(2) + section(1, sec1(p, n8, 4) + b"\x00") + s2, "8 + n8"),
        "section_1_short": (head(2) + section(1, sec1(p, n8, 4)[:-1]) + s2, "8 + n8"),
        "section_1_tiny": (head(2) + section(1, b"\x20\x00") + s2, "section 1"),
        "nvars_one_more": (head(2) + section(1, sec1(p, n8, 5)) + s2, "n8 * nVars"),
        "nvars_one_less": (head(2) + section(1, sec1(p, n8, 3)) + s2, "n8 * nVars"),
        "nvars_max": (head(2) + section(1, sec1(p, n8, 0xffffffff)) + s2, "n8 * nVars"),
        "value_is_p": (wtns_bytes([1, p, 2, 3], p), "not below the prime"),
        "value_all_ones": (wtns_bytes([1, 2, 3, (1 << 256) - 1], p), "not below the prime"),
        "even_prime": (wtns_bytes([1, 2], p - 1), "odd"),
        "prime_one": (wtns_bytes([0], 1, n8=8), "odd"),
    }
    g = R.PRIMES["goldilocks"]
    out["value_is_p_n8_8"] = (wtns_bytes([1, g], g), "not below the prime")
    out["value_257_n8_8"] = (wtns_bytes([1, 257], 257), "not below the prime")
    return out


# --------------------------------------------------------------------------- witness <-> rs_witness
def to_witness(values, p: int, n8=None) -> "abi.Witness":
    return abi.Witness.from_ints(list(values), p, n8)


def project(values, signal_map):
    """The wire-ordered witness: wire signal_map[s] <- values[s]."""
    out = [0] * len(signal_map)
    for s, wire in signal_map.items():
        out[wire] = values[s]
    return out


# --------------------------------------------------------------------------- the Python evaluator
def _triple(flags):
    bad = [i for i, ok in enumerate(flags) if not ok]
    return (len(flags), len(bad), bad[0] if bad else NONE)


def evaluate(p, w, classes=None, cons=None, log=None):
    """The report of witness w: {class name: (checked, failed, first_failed)}; a class not given has
    (0, 0, NONE).  classes: (cons_eq, eq, linear, nonlinear) lists of pyref Cons (R.classify's);
    cons: the result's rows; log: [(from, {signal: value})]."""
    rep = {c: (0, 0, NONE) for c in CLASSES}
    if classes is not None:
        for name, rows in zip(CLASSES[:4], classes):
            rep[name] = _triple([S.holds(c, w, p) for c in rows])
    if cons is not None:
        rep["output"] = _triple([S.holds(c, w, p) for c in cons])
    if log is not None:
        rep["log"] = _triple([(w[frm] - S._dot(to, w, p)) % p == 0 for frm, to in log])
    return rep


def triples(rep) -> dict:
    """An RsWitnessReport in evaluate's form."""
    return {c: (int(rep.checked[i]), int(rep.failed[i]), int(rep.first_failed[i])) for i, c in enumerate(CLASSES)}


def random_vector(rng, n, p):
    return [1] + [rng.randrange(p) for _ in range(n - 1)]


def eliminated_intermediate(sys_, log, rng):
    """A signal the log defines (an eliminated one) that an input row mentions."""
    used = set()
    for row in sys_.rows:
        used |= S._signals(row, sys_.p)
    cand = sorted({frm for frm, _ in log} & used)
    return rng.choice(cand)


# --------------------------------------------------------------------------- hand-built inputs
class RawInput:
    """An rs_input over given rows: cons_eq / eq / linear are lists of {signal: value} (their C parts),
    nl a list of (a, b, c).  Nothing is classified or cleaned: the evaluator takes rows as they are."""

    def __init__(self, p, max_signal, cons_eq=(), eq=(), linear=(), nl=(), prime_name=None):
        self.p, self.max_signal = p, max_signal
        self.classes = ([R.Con({}, {}, dict(m)) for m in cons_eq], [R.Con({}, {}, dict(m)) for m in eq],
                        [R.Con({}, {}, dict(m)) for m in linear], [R.Con(dict(a), dict(b), dict(c)) for a, b, c in nl])
        self.blocks = [rsio._Block([dict(m) for m in cons_eq]), rsio._Block([dict(m) for m in eq]),
                       rsio._Block([dict(m) for m in linear]), rsio._Block([dict(a) for a, _, _ in nl]),
                       rsio._Block([dict(b) for _, b, _ in nl]), rsio._Block([dict(c) for _, _, c in nl])]
        self.forb = np.array([0], dtype=np.uint32)
        inp = abi.RsInput()
        inp.prime_id = abi.PRIME_IDS[prime_name] if prime_name else 255
        for i in range(4):
            inp.prime[i] = (p >> (64 * i)) & abi.U64_MAX
        inp.max_signal = max_signal
        inp.n_forbidden = 1
        inp.forbidden = self.forb.ctypes.data_as(C.POINTER(C.c_uint32))
        inp.cons_eq, inp.eq, inp.linear, inp.nl_a, inp.nl_b, inp.nl_c = [b.lc for b in self.blocks]
        self.inp = inp


def _lc_with_value(rng, p, w, keys, target):
    """{key: coefficient} over `keys` (w[keys[-1]] != 0) whose dot product with w is `target`."""
    m = {k: rng.randrange(1, p) for k in keys[:-1]}
    rest = (target - sum(v * w[k] for k, v in m.items())) % p
    m[keys[-1]] = rest * pow(w[keys[-1]], -1, p) % p
    return m


def border_input(p, seed=1, chunk=64, prime_name=None):
    """(RawInput, witness) with rows of every length around a chunk of `chunk` entries and a 5,000-entry
    row, in C of the linear classes and in A, B and C of non-linear rows; empty rows between them; an empty
    A beside a non-empty B; a row that begins exactly on a chunk border and one that ends on one.  Every
    other row holds, the rest miss by one."""
    rng = random.Random(seed)
    n = 5200
    w = [1] + [rng.randrange(1, p) for _ in range(n - 1)]
    lens = [0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1, 5000]
    flip = [0]

    def target(t):
        flip[0] ^= 1
        return t if flip[0] else (t + 1) % p

    def keys(ln):
        return rng.sample(range(n), ln)

    def lc(ln, t):
        if ln == 0:
            return {}
        return _lc_with_value(rng, p, w, keys(ln), t)

    linear, nl = [], []
    for ln in lens:
        # (an empty linear row's dot is 0: it holds, and cannot be made to miss)
        linear.append(lc(ln, target(0) if ln else 0))
        linear.append({})
        for part in range(3):
            x, y = rng.randrange(1, p), rng.randrange(1, p)
            if part == 0:
                a, b = lc(ln, x if ln else 0), lc(3, y)
                c = lc(2, target((x if ln else 0) * y % p))
            elif part == 1:
                a, b = lc(2, x), lc(ln, y if ln else 0)
                c = lc(2, target(x * (y if ln else 0) % p))
            else:
                a, b = lc(1, x), lc(2, y)
                c = lc(ln, target(x * y % p)) if ln else {}
            nl.append((a, b, c))
    # an empty A with a non-empty B: the product is 0
    nl.append(({}, lc(4, 9), lc(3, 0)))
    nl.append(({}, lc(4, 9), lc(3, 1)))
    # the linear block so far holds sum(lens) entries; pad to a border, then a row that begins exactly on
    # it and ends exactly on the next one, then one that begins there
    used = sum(len(m) for m in linear)
    pad = (-used) % chunk
    if pad:
        linear.append(lc(pad, target(0)))
    linear.append(lc(chunk, target(0)))
    linear.append(lc(3, target(0)))
    cons_eq = [lc(1, 0), lc(2, target(0)), {}, lc(chunk + 3, target(0))]
    eq = [lc(2, target(0)) for _ in range(chunk + 2)]
    return RawInput(p, n, cons_eq, eq, linear, nl, prime_name), w


def degenerate_inputs(p):
    """[(RawInput, witness)]: a block of only empty rows; blocks with zero rows; max_signal = 1 (the
    witness is the constant alone, the rows are {0: c}); rows whose only key is 0."""
    out = []
    out.append((RawInput(p, 3, linear=[{}, {}, {}], nl=[({}, {}, {}), ({}, {}, {})]), [1, 2, 3]))
    out.append((RawInput(p, 3), [1, 2, 3]))
    out.append((RawInput(p, 3, cons_eq=[{1: 1, 0: p - 2}]), [1, 2, 3]))
    out.append((RawInput(p, 1, cons_eq=[{0: 0}, {0: 5}], linear=[{0: p - 1}, {}],
                         nl=[({0: 2}, {0: 3}, {0: 6}), ({0: 2}, {0: 3}, {0: 7}), ({0: p - 1}, {0: p - 1}, {0: 1})]), [1]))
    out.append((RawInput(p, 4, linear=[{0: 1}, {0: 0}], nl=[({0: 3}, {0: 4}, {0: 12}), ({0: 1}, {2: 1}, {0: 9})]), [1, 5, 9, 2]))
    return out


def edge_values(p):
    vals = [0, 1, 2, p - 1, p - 2, (1 << 64) - 1, 1 << 64, (1 << 128) - 1, 1 << 128, 1 << 192, p // 2, p // 2 + 1]
    return sorted({v for v in vals if v < p})


def edge_input(p, seed=2, prime_name=None):
    """(RawInput, witness): coefficients and witness values from edge_values; two-entry rows whose partial
    sums are exactly p; A.w = B.w = p - 1 with C.w = 1; a 5,000-entry row of (p - 1)(p - 1) terms."""
    rng = random.Random(seed)
    ev = edge_values(p)
    w = [1] + ev + [p - 1] * 5000
    n = len(w)
    ix = list(range(1, 1 + len(ev)))
    linear, nl = [], []
    for i in ix:            # every coefficient x every value, as one-entry rows and against the constant
        for c in ev:
            linear.append({i: c})
            linear.append({i: c, 0: (-c * w[i]) % p})
            nl.append(({i: c}, {rng.choice(ix): rng.choice(ev)}, {0: rng.choice(ev)}))
            j = rng.choice(ix)
            nl.append(({i: c}, {j: 1}, {0: c * w[i] * w[j] % p}))
    one = ix[ev.index(1)]
    for v in ev:            # partial sums exactly p: v + (p - v)
        if v:
            linear.append({one: v, 0: p - v})
            linear.append({one: v, 0: (p - v + 1) % p})
    m1 = ix[ev.index(p - 1)]
    nl.append(({m1: 1}, {m1: 1}, {0: 1}))             # (p - 1)(p - 1) = 1
    nl.append(({m1: 1}, {m1: 1}, {0: 2}))
    nl.append(({0: p - 1}, {one: p - 1}, {one: 1}))
    big = {k: p - 1 for k in range(1 + len(ev), n)}     # 5,000 terms (p - 1)(p - 1) = 1 each
    linear.append({**big, 0: (-5000) % p})
    linear.append({**big, 0: (-4999) % p})
    nl.append((dict(big), {0: 1}, {0: 5000 % p}))
    nl.append(({0: 1}, dict(big), {0: 5001 % p}))
    return RawInput(p, n, linear=linear, nl=nl, prime_name=prime_name), w
