"""Helpers of the lift tests (test_lift_abi.py, test_gpu_lift.py): a Python statement of the lift's
definition (include/rs_simplify.h, ABI 14), circuits whose log has a chosen number of levels, and hand-built
logs around the chunk borders of the device evaluator.  Exact arithmetic in F_p: no tolerances."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

import rsio
import wtnsio as W
from circom_cvm_amd import abi

R = rsio.R


class Refused(ValueError):
    """A refusal of the definition; str() carries the word the library's message carries too."""


# the word of each refusal's message, shared by the model and the tests
WORDS = {"wires": "wires", "one": "w[0]", "range": "not below the prime", "from_range": "`from` is not below",
         "from_zero": "`from` is the constant", "from_wire": "still has a wire", "key": "a key is not below",
         "ptr": "row pointers", "order": "elimination order", "null": "null argument"}


# --------------------------------------------------------------------------- the definition
def lift_model(v, signal_map, log, L, p):
    """The lift of the wire witness `v` through `log` = [(from, {key: coefficient})] and signal_map =
    {label: wire} over L labels -> {"values", "levels", "shadowed", "free", "lifted", "entries",
    "level" (per entry, None for a shadowed one), "free_set"}.  Raises Refused on each refusal.
    The order rule (an owner entry's owned keys belong to later entries) is checked first; it makes the
    recursion of the definition a plain loop from the last entry to the first."""
    if len(v) != len(signal_map):
        raise Refused(WORDS["wires"])
    if not v or v[0] != 1:
        raise Refused(WORDS["one"])
    if any(not 0 <= x < p for x in v):
        raise Refused(WORDS["range"])
    owner = {}
    for i, (frm, to) in enumerate(log):
        if frm >= L:
            raise Refused(WORDS["from_range"])
        if frm == 0:
            raise Refused(WORDS["from_zero"])
        if frm in signal_map:
            raise Refused(WORDS["from_wire"])
        owner[frm] = i                       # the largest i with from_i == s
    for frm, to in log:
        if any(k >= L for k in to):
            raise Refused(WORDS["key"])
    w = [0] * L
    free = set()
    for s in range(L):
        if s in signal_map:
            w[s] = v[signal_map[s]]
        elif s not in owner:
            free.add(s)                      # value 0
    level = [None] * len(log)
    for i, (frm, to) in enumerate(log):
        if owner[frm] == i and any(k in owner and owner[k] <= i for k in to):
            raise Refused(WORDS["order"])
    entries = 0
    for i in range(len(log) - 1, -1, -1):
        frm, to = log[i]
        if owner[frm] != i:
            continue                         # shadowed: defines nothing, creates no dependency
        owned = [owner[k] for k in to if k in owner]     # (a key with coefficient 0 is still a key)
        level[i] = 1 + max(level[j] for j in owned) if owned else 0
        w[frm] = sum(c * w[k] for k, c in to.items()) % p
        entries += len(to)
    own_levels = [x for x in level if x is not None]
    return {"values": w, "levels": 1 + max(own_levels) if own_levels else 0, "shadowed": len(log) - len(own_levels),
            "free": len(free), "lifted": len(own_levels), "entries": entries, "level": level, "free_set": free}


def model_counts(m, L, n_wires):
    """lift_model's result in RsLiftReport.counts() order."""
    return (L, n_wires, m["lifted"], m["free"], m["shadowed"], m["levels"], m["entries"])


# --------------------------------------------------------------------------- rs_output over a hand-built log
class LogHolder:
    """An RsOutput that carries only what the lift reads: n_labels, n_wires, label_to_wire and the log.
    l2w: a list (label -> wire or -1); log: [(from, {key: coefficient})], keys ascending in the arrays."""

    def __init__(self, l2w, log):
        self.l2w = np.array(list(l2w) or [0], dtype=np.int32)
        self.blk = rsio._Block([dict(sorted(to.items())) for _, to in log])
        self.frm = np.array([f for f, _ in log] or [0], dtype=np.uint32)
        o = abi.RsOutput()
        o.n_labels = len(l2w)
        o.n_wires = sum(1 for x in l2w if x >= 0)
        o.label_to_wire = self.l2w.ctypes.data_as(C.POINTER(C.c_int32))
        o.n_log = len(log)
        o.log_from = self.frm.ctypes.data_as(C.POINTER(C.c_uint32))
        o.log_to = self.blk.lc
        self.out = o
        self.signal_map = {s: int(x) for s, x in enumerate(l2w) if x >= 0}
        self.log = log


def l2w_of(L, no_wire):
    """label_to_wire over L labels: the labels of `no_wire` get -1, the others the order-preserving rank."""
    out, nxt = [], 0
    for s in range(L):
        if s in no_wire:
            out.append(-1)
        else:
            out.append(nxt)
            nxt += 1
    return out


# --------------------------------------------------------------------------- K levels through the simplifier
def tower_ids(K, copy=0):
    """The labels of copy `copy`: t[1..K], c[0..K-1], s[1..K+1], u (u + 1 and u + 2 follow it)."""
    b = 1 + copy * (3 * K + 4)
    t = {k: b + k - 1 for k in range(1, K + 1)}
    c = {j: b + K + j for j in range(K)}
    s = {k: b + 2 * K + (K + 1 - k) for k in range(1, K + 2)}      # s[K+1] first, s[1] the largest
    return t, c, s, b + 3 * K + 1


def tower(p, K, copies=1):
    """A pyref System whose --O2 log has exactly K levels: round k eliminates s_k := s_{k+1} + t_k (the row
    c_{k-2} s_k = s_{k+1} + t_k turns linear once c_{k-2} = 1 is known), so s_1 depends on s_2 ... on
    s_K.  u loses its only occurrence without an entry and u + 2 occurs nowhere: the two free labels.
    For K < 3 the last product row takes t_min(i, K) for t_i.  Only label 0 is forbidden."""
    rows = []
    for cp in range(copies):
        t, c, s, u = tower_ids(K, cp)
        tk = lambda i: t[min(i, K)]
        rows.append(R.Con({}, {}, {c[0]: 1, 0: p - 1}))
        rows.append(R.Con({}, {}, {s[1]: 1, s[2]: p - 1, t[1]: p - 1}))
        for k in range(2, K + 1):
            rows.append(R.Con({c[k - 2]: 1}, {s[k]: 1}, _sum({s[k + 1]: 1}, {t[k]: 1}, p)))
            rows.append(R.Con({c[k - 2]: 1}, {c[k - 1]: 1}, {0: 1}))
        rows.append(R.Con({tk(1): 1}, {tk(2): 1}, _sum({tk(3): 1}, {s[K + 1]: 1}, p)))
        rows.append(R.Con({c[0]: 1, 0: p - 1}, {u: 1}, _sum({u + 1: 1}, {t[1]: 1}, p)))
    return R.System(p, 1 + copies * (3 * K + 4), 0, 0, 0, {0}, rows)


def _sum(a, b, p):
    out = dict(a)
    for k, v in b.items():
        out[k] = (out.get(k, 0) + v) % p
    return out


def tower_wire_witness(p, K, copies, signal_map, cons, rng):
    """A wire witness that satisfies the result's rows: random values, then each output row solved for one
    of its t's.  The rows of a tower's result are t_a t_b = t_c + (a sum of t's), one per copy, over
    disjoint labels."""
    v = W.random_vector(rng, len(signal_map), p)
    lab = [1] * (max(signal_map) + 1)
    for s, wire in signal_map.items():
        lab[s] = v[wire]
    for con in cons:
        # solve for a key of C that is in neither A nor B
        cand = [k for k in con.c if k and k not in con.a and k not in con.b and con.c[k] % p]
        k = cand[0]
        ab = sum(c * lab[x] for x, c in con.a.items()) * sum(c * lab[x] for x, c in con.b.items()) % p
        rest = sum(c * lab[x] for x, c in con.c.items() if x != k) % p
        lab[k] = (ab - rest) * pow(con.c[k], -1, p) % p
        v[signal_map[k]] = lab[k]
    return v


# --------------------------------------------------------------------------- hand-built logs
def _coef(rng, ev, p):
    return rng.choice(ev) or 1


def border_log(p, chunk, seed=1):
    """(l2w, log, v): owner entries of 0, 1, chunk - 1 .. 2 chunk + 1 and 5,000 keys at each of levels 0,
    1 and 2 with empty rows between them; padding so that one row of a level begins exactly on a virtual
    chunk border and one ends on it; zero coefficients on owned keys; two shadowed entries (one with a
    different constant); three free labels, one of them used as a key.  Coefficients and values are
    wtnsio.edge_values.  Level 2 is logged first (the log is in elimination order: an entry reads later
    entries' labels)."""
    rng = random.Random(seed)
    ev = W.edge_values(p)
    lens = [0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk - 1, 2 * chunk, 2 * chunk + 1, 5000]
    n_wire = 5200
    wires = list(range(1, n_wire))            # labels 1 .. n_wire - 1 have wires (0 too)
    nxt = [n_wire]

    def fresh():
        nxt[0] += 1
        return nxt[0] - 1

    free = [fresh(), fresh(), fresh()]
    by_level = {0: [], 1: [], 2: []}          # level -> [(from, to)]
    for lv in (0, 1, 2):
        rows = []
        for ln in lens:
            rows.append(ln)
            rows.append(0)
        if lv > 0:
            rows = [max(ln, 1) for ln in rows]     # (a row of level >= 1 holds its owned key: no empty rows there)
        # pad: the level's virtual entries so far, then a row to the next border, a row of exactly one
        # chunk (begins and ends on a border), and a short one that begins on a border
        used = sum(rows)
        rows += [(-used) % chunk or chunk, chunk, 3]
        for ln in rows:
            frm = fresh()
            to = {}
            if lv > 0:
                # an owned key of the level below: the dependency, with a zero coefficient every other time
                dep = rng.choice(by_level[lv - 1])[0]
                to[dep] = 0 if rng.random() < 0.5 else _coef(rng, ev, p)
            keys = rng.sample(wires, max(ln - len(to), 0))
            for k in keys:
                to[k] = rng.choice(ev)
            if ln >= 3 and lv == 0:
                to.pop(keys[0])
                to[free[0]] = _coef(rng, ev, p)   # a free label as a key
            if ln >= 2:
                to.pop(keys[-1], None)
                to[0] = rng.choice(ev)            # the constant
            by_level[lv].append((frm, to))
    log = by_level[2] + by_level[1] + by_level[0]
    # two shadowed entries, before the owners of their labels: same `to` with another constant, and an
    # unrelated one
    f0, t0 = by_level[0][3]
    f1, t1 = by_level[1][5]
    log = [(f0, {**t0, 0: (t0.get(0, 0) + 1) % p}), (f1, {wires[7]: 5 % p})] + log
    L = nxt[0]
    no_wire = set(range(n_wire, L))
    l2w = l2w_of(L, no_wire)
    v = [1] + [rng.choice(ev) for _ in range(n_wire - 1)]
    return l2w, log, v


def chain_log(p, n):
    """Entry i depends on entry i + 1: n levels of one row.  w[from_i] = 2 w[from_{i+1}] + w[1] + 1."""
    l2w = l2w_of(2 + n, set(range(2, 2 + n)))
    log = []
    for i in range(n):
        to = {0: 1, 1: 1}
        if i + 1 < n:
            to[2 + i + 1] = 2 % p
        log.append((2 + i, to))
    return l2w, log, [1, 5 % p]


def wide_log(p, rows, seed=3):
    """`rows` entries of 3 keys at level 1 (logged first), then `rows` at level 0."""
    rng = random.Random(seed)
    ev = W.edge_values(p)
    n_wire = 64
    lo = n_wire + rows                         # level-0 labels n_wire .. lo - 1, level-1 labels lo .. lo + rows - 1
    l2w = l2w_of(lo + rows, set(range(n_wire, lo + rows)))
    lvl1 = [(lo + i, dict(sorted({0: ev[i % len(ev)], 1 + i % (n_wire - 1): ev[(i + 3) % len(ev)],
                                  n_wire + (i * 7 + 1) % rows: ev[(i + 5) % len(ev)] or 1}.items()))) for i in range(rows)]
    lvl0 = [(n_wire + i, {0: ev[(i + 1) % len(ev)], 1 + (i + 9) % (n_wire - 1): ev[(i + 2) % len(ev)],
                          1 + (i + 30) % (n_wire - 1): ev[(i + 7) % len(ev)]}) for i in range(rows)]
    for _, to in lvl0:
        assert len(to) == 3
    v = [1] + [rng.choice(ev) for _ in range(n_wire - 1)]
    return l2w, lvl1 + lvl0, v


def degenerate_logs(p):
    """[(l2w, log, v)]: the empty log with and without non-wire labels; L == 1; a log of shadowed entries
    of a single label (the last one owns it); an owner entry with no keys."""
    return [
        ([0, 1, 2], [], [1, 2, 3]),
        ([0, -1, 1, -1], [], [1, 7 % p]),
        ([0], [], [1]),
        ([0, 1, -1], [(2, {0: 3 % p}), (2, {1: 1}), (2, {0: 1, 1: p - 1})], [1, 9 % p]),
        ([0, -1, -1], [(2, {1: 1}), (1, {})], [1]),
    ]


# --------------------------------------------------------------------------- refusals
def refusal_cases(p):
    """{name: (l2w, log, v, the word of the message)}: every refusal of the definition that shows in the
    data (the device tests run the same table)."""
    l2w, good, v = [0, 1, 2, -1, -1, -1, -1], [(3, {0: 9}), (5, {4: 1, 6: 1}), (4, {2: 1, 3: 3}), (3, {0: 5, 1: 2})], [1, 10, 20]
    W_ = WORDS
    return {
        "one_long": (l2w, good, v + [3], W_["wires"]),
        "one_short": (l2w, good, v[:-1], W_["wires"]),
        "w0_is_2": (l2w, good, [2] + v[1:], W_["one"]),
        "w0_is_0": (l2w, good, [0] + v[1:], W_["one"]),
        "value_is_p": (l2w, good, [1, p, 20], W_["range"]),
        "from_is_L": (l2w, [(7, {0: 1})] + good, v, W_["from_range"]),
        "from_is_0": (l2w, good + [(0, {1: 1})], v, W_["from_zero"]),
        "from_has_wire": (l2w, [(2, {1: 1})] + good, v, W_["from_wire"]),
        "key_is_L": (l2w, good[:3] + [(3, {0: 5, 7: 2})], v, W_["key"]),
        "key_of_shadowed_is_L": (l2w, [(3, {9: 1})] + good[1:], v, W_["key"]),
        "own_from_as_key": (l2w, good[:2] + [(3, {2: 1, 3: 3}), (4, {0: 5, 1: 2})], v, W_["order"]),
        "earlier_entry_read": ([0, 1, -1, -1], [(2, {0: 1}), (3, {2: 1})], [1, 4], W_["order"]),
        "cycle": ([0, 1, -1, -1], [(2, {3: 1}), (3, {2: 1})], [1, 4], W_["order"]),
    }


def expect_refusal(call, word):
    with pytest.raises(abi.RsError) as e:
        call()
    assert e.value.code == -1 and word in str(e.value), str(e.value)
