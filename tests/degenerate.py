"""The empty, single and widest shapes of every entry point as test material (no GPU needed):

  block lattice   a base system per prime restricted to each of the 16 subsets of its four row classes
                  (cons_eq, eq, linear, non-linear; a mask is one character per class in that order),
                  from rsio.gen_system and from soundness.small_circuit (satisfiable under any subset);
  singletons      max_signal = 1, one row of each class alone, only empty rows, every signal forbidden,
                  no public signals, no private inputs, a single linear round, all storage rows emptied;
  DAGs            nine component DAGs whose templates carry no rows, no locals or only partial rows;
  ranks           systems with fewer linear clusters than a sharded group has ranks;
  wide wires      200 rows over 2^24 + 1024 forbidden signals: four-byte wires in the .r1cs writer, and
                  the constraint section built in Python with int.to_bytes as the sort key.

tests/test_degenerate.py proves on the CPU that each case has the shape its name claims and that both
oracles agree on it; tests/test_gpu_degenerate.py runs the same cases through the library."""
from __future__ import annotations

import dataclasses
import random
import struct
from typing import Dict, List, Optional, Tuple

import numpy as np

import dispatch_shapes as ds
import rsio
import soundness as S
from test_gpu_run_tail import emptied_system

R = rsio.R
BN, GL, F257 = R.PRIMES["bn128"], R.PRIMES["goldilocks"], 257
PRIMES3 = (("bn128", BN), ("goldilocks", GL), ("f257", F257))
FLAG_SETS = S.FLAG_SETS
CLASSES = ("cons_eq", "eq", "linear", "non_linear")
MASKS = tuple(format(m, "04b") for m in range(16))
ONESHOT_MASKS = ("0000", "1000", "0111", "1111")
WORLDS = (2, 3, 4)


def abi_name(pname: str) -> Optional[str]:
    """The prime's name for rsio.InputHolder (None: a custom prime)."""
    return pname if pname in R.PRIMES else None


def fl_of(key: str, log: bool = False):
    lvl, rd, old = FLAG_SETS[key]
    return rsio.flags(lvl, rd, old, log=log)


def holder(sys_: "R.System", pname: str) -> "rsio.InputHolder":
    return rsio.InputHolder(sys_, abi_name(pname))


def normal_system() -> "R.System":
    """The ordinary case that runs between the degenerate ones on the same engine."""
    return rsio.gen_system(7, BN, n_sig=80, n_rows=150)


# ============================================================================ A. the block lattice
def row_class(c: "R.Con", p: int) -> int:
    """The block map_tree puts a row into (pyref.classify)."""
    if R.is_constant_equality(c):
        return 0
    if R.is_equality(c, p):
        return 1
    return 2 if R.is_linear(c) else 3


def class_counts(sys_: "R.System") -> Tuple[int, ...]:
    n = [0, 0, 0, 0]
    for c in sys_.rows:
        n[row_class(c, sys_.p)] += 1
    return tuple(n)


def restrict(sys_: "R.System", mask: str) -> "R.System":
    """The rows of the classes whose mask character is 1; everything else as it was."""
    return dataclasses.replace(sys_, rows=[c for c in sys_.rows if mask[row_class(c, sys_.p)] == "1"])


SAT_SEED = 7
_LATTICE: Dict[Tuple[str, str], tuple] = {}


def lattice_base(family: str, pname: str):
    """(System, witnesses or None): `gen` an rsio.gen_system, `sat` soundness.small_circuit(prime, 7)."""
    key = (family, pname)
    if key not in _LATTICE:
        if family == "gen":
            _LATTICE[key] = (rsio.gen_system(31, dict(PRIMES3)[pname], n_sig=60, n_rows=80), None)
        else:
            assert family == "sat"
            _LATTICE[key] = S.small_circuit(pname, SAT_SEED)
    return _LATTICE[key]


def lattice_cases(family: str, pname: str):
    """[(mask, System)] for the 16 subsets."""
    base, _ = lattice_base(family, pname)
    return [(m, restrict(base, m)) for m in MASKS]


# ============================================================================ B. singletons and headers
def _small(p, rows, S_=8, n_out=1, n_pub=1, n_priv=2, forb=(0, 1, 2)) -> "R.System":
    return R.System(p, S_, n_out, n_pub, n_priv, set(forb), rows)


def all_forbidden_system(p: int) -> "R.System":
    sys_ = rsio.gen_system(33, p, n_sig=40, n_rows=60)
    return dataclasses.replace(sys_, forbidden=set(range(sys_.max_signal)))


def single_round_system(p: int) -> "R.System":
    """Round 1 eliminates every linear row and no non-linear row turns linear: later rounds have an
    empty list (dispatch_shapes' chain with probes)."""
    b = ds.Builder(3, p)
    b.probes(ds.chain(b, 12)["probe"])
    return b.system()


def singletons(p: int) -> Dict[str, "R.System"]:
    m = p - 1
    rows_mix = rsio.gen_system(34, p, n_sig=30, n_rows=40).rows
    return {
        "max_signal_1": R.System(p, 1, 0, 0, 0, {0}, []),
        "x_eq_0": _small(p, [R.Con({}, {}, {5: 1})]),
        "x_eq_c": _small(p, [R.Con({}, {}, {5: 2 % p, 0: 3 % p})]),
        "x_eq_y": _small(p, [R.Con({}, {}, {5: 2 % p, 6: (p - 2) % p})]),
        "one_linear": _small(p, [R.Con({}, {}, {4: 1, 5: m, 6: 2 % p, 0: 1})]),
        "ab_eq_c": _small(p, [R.Con({4: 1}, {5: m}, {6: 1, 0: 2 % p})]),
        "ab_eq_0": _small(p, [R.Con({4: 1}, {5: m}, {})]),
        "nl_empty_b": _small(p, [R.Con({4: 1, 5: 1}, {}, {6: 1})]),
        "only_empty_rows": _small(p, [R.Con({}, {}, {}) for _ in range(3)]),
        "all_forbidden": all_forbidden_system(p),
        # signal 1 is the first private input here and is defined away: a count of the deleted inputs that
        # starts behind an output that is not there misses it
        "no_publics": R.System(p, 31, 0, 0, 4, {0}, rows_mix + [R.Con({}, {}, {1: 1, 0: (p - 5) % p})]),
        "no_private_inputs": R.System(p, 31, 2, 2, 0, {0, 1, 2, 3, 4}, rows_mix),
        "single_round": single_round_system(p),
        "all_storage_emptied": emptied_system(p, k=8),
    }


# the singletons whose rows have a solution: soundness.check runs on the engine's result.  Not
# all_storage_emptied, although it has one: its signals sat in a non-linear row after round 1 and left
# every row in round 2, and the reference keeps their wires (the corner soundness.py's witness-map check
# is stricter in); it stays pinned by oracle parity.
SOUND_SINGLETONS = ("max_signal_1", "x_eq_0", "x_eq_c", "x_eq_y", "one_linear", "ab_eq_c", "ab_eq_0", "nl_empty_b",
                    "only_empty_rows", "single_round")


# ---------------------------------------------------------------------------- the DAGs
def dags(p: int) -> Dict[str, tuple]:
    """name -> (nodes, main, n_pub_out, n_pub_in, n_priv_in, forbidden of main)."""
    m = p - 1
    N, C = R.DagNode, R.Con
    empty = lambda: C({}, {}, {})   # noqa: E731
    out: Dict[str, tuple] = {}
    out["main_alone_no_constraints"] = ([N([], [1, 2, 3])], 0, 1, 1, 1, {0, 1, 2})
    out["main_no_locals"] = ([N([], [])], 0, 0, 0, 0, {0})
    out["main_only_empty_constraints"] = ([N([empty(), empty()], [1, 2, 3])], 0, 1, 1, 1, {0, 1, 2})
    bare, hollow = N([], [1]), N([empty(), empty()], [1, 2])
    out["children_without_rows"] = ([bare, hollow, N([], [1, 2], edges=[(0, 2), (1, 3), (0, 5)])], 2, 1, 1, 0, {0, 1, 2})
    konst = N([C({}, {}, {0: 5 % p}), C({}, {}, {1: 1, 2: m})], [1, 2])
    out["constant_only_row"] = ([konst, N([C({}, {}, {0: 7 % p}), C({1: 1}, {2: 1}, {3: 1})], [1, 2], edges=[(0, 2), (0, 4)])],
                                1, 1, 1, 0, {0, 1, 2})
    part = lambda: [C({1: 1}, {}, {}), C({}, {2: m}, {}), C({1: 2 % p}, {2: 1}, {})]   # noqa: E731
    out["partial_non_linear_rows"] = ([N(part(), [1, 2]), N(part() + [C({}, {}, {1: 1, 3: m, 4: 1})], [1, 2], edges=[(0, 2)])],
                                      1, 1, 1, 0, {0, 1, 2})
    out["main_first_unreachable_after"] = ([N([C({1: 1}, {2: 1}, {3: 1}), C({}, {}, {2: 1, 3: m})], [1, 2, 3]),
                                            N([C({}, {}, {1: 1, 0: 1})], [1, 2])], 0, 1, 1, 1, {0, 1, 2})
    chain = [N([C({1: 1}, {1: 1}, {1: 1})], [1])]
    for t in range(1, 300):   # level t: its one signal equals its child's (local id 2 = in_number 1 + 1)
        chain.append(N([C({}, {}, {1: 1, 2: m}) if t % 3 else C({1: 1}, {2: 1}, {0: 1})], [1], edges=[(t - 1, 1)]))
    out["chain_300_deep"] = (chain, 299, 1, 0, 0, {0, 1})
    gate = N([], [], custom_gate=True)
    out["custom_gate_no_locals"] = ([gate, N([C({1: 1}, {2: 1}, {3: 1}), C({}, {}, {2: 1, 3: m, 1: 1})], [1, 2, 3],
                                              edges=[(0, 3), (0, 3)])], 1, 1, 1, 1, {0, 1, 2})
    return out


# ============================================================================ D. ranks with nothing to do
def rank_cases(p: int, world: int) -> Dict[str, Tuple["R.System", dict]]:
    """name -> (System, the numbers its name claims): `clusters` linear clusters in round 1 (compared
    with `world` as `rel` says) and `rounds` calls of the linear simplification."""
    out: Dict[str, Tuple["R.System", dict]] = {}

    def chains(seed, sizes, probes=True, extra=None):
        b = ds.Builder(seed, p)
        for n in sizes:
            cl = ds.chain(b, n)
            if probes:
                b.probes(cl["probe"])
        if extra:
            extra(b)
        return b.system()

    b = ds.Builder(41, p)
    b.probes(b.take(12))
    out["no_linear_rows"] = (b.system(), dict(clusters=0, rel="below", rounds=1))
    out["one_cluster"] = (chains(42, [12]), dict(clusters=1, rel="below", rounds=1))
    out["world_minus_1_clusters"] = (chains(43, [8 + i for i in range(world - 1)]), dict(clusters=world - 1, rel="below", rounds=1))
    out["world_clusters"] = (chains(47, [8 + i for i in range(world)]), dict(clusters=world, rel="at", rounds=1))
    out["one_process4_cluster"] = (chains(44, [ds.P4_MIN + 10], probes=False), dict(clusters=1, rel="below", rounds=1, p4=True))
    out["no_non_linear_rows"] = (chains(45, [6 + i for i in range(world + 2)], probes=False),
                                 dict(clusters=world + 2, rel="above", rounds=1))
    out["all_forbidden"] = (all_forbidden_system(p), dict(rel="none", rounds=2))   # (round 2 takes nothing either)
    out["round2_one_cluster"] = (chains(46, [6 + i for i in range(world + 1)], extra=lambda b: ds.storage_row(b, 2, [4])),
                                 dict(clusters=world + 1, rel="above", rounds=2, round2_subs=1))
    out["max_signal_1"] = (R.System(p, 1, 0, 0, 0, {0}, []), dict(clusters=0, rel="below", rounds=1))
    return out


RANK_CASES = ("no_linear_rows", "one_cluster", "world_minus_1_clusters", "world_clusters", "one_process4_cluster",
              "no_non_linear_rows", "all_forbidden", "round2_one_cluster", "max_signal_1")
HOST_TRANSPORT_CASE = ("one_cluster", 2)


def takeable_clusters(sys_: "R.System") -> int:
    """Linear clusters of round 1 that hold a signal a rank could take."""
    return sum(1 for c in ds.cluster_shapes(sys_) if c["takeable"] > 0)


# ============================================================================ E. four-byte wires
WIDE_S = (1 << 24) + 1024
WIDE_EDGE_IDS = (1, 2, 255, 256, 257, 65535, 65536, 65537, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 255,
                 (1 << 24) + 256, 0x0100ff, 0x00ff00ff, 0x01000100, WIDE_S - 1)


def byte_length(w: int) -> int:
    return max(1, (w.bit_length() + 7) // 8)


def wide_rows(p: int = BN, seed: int = 5) -> List["R.Con"]:
    """200 rows, half linear and half non-linear, of 3 to 9 entries: most keys from WIDE_EDGE_IDS, the
    rest uniform below WIDE_S; the first row of either half holds a key of every byte length."""
    rng = random.Random(seed)

    def keys(n, must=()):
        ks = set(must)
        while len(ks) < n:
            ks.add(rng.choice(WIDE_EDGE_IDS) if rng.random() < 0.7 else rng.randrange(1, WIDE_S))
        ks = list(ks)
        rng.shuffle(ks)
        return ks

    def coef():
        return rng.choice((1, p - 1, 2, rng.randrange(1, p)))

    every = (255, 256, 65536, 1 << 24)
    rows = []
    for i in range(100):
        n = rng.randint(3, 9)
        rows.append(R.Con({}, {}, {k: coef() for k in keys(max(n, 4) if i == 0 else n, every if i == 0 else ())}))
    for i in range(100):
        n = rng.randint(3, 9)
        ks = keys(max(n, 6) if i == 0 else n, every if i == 0 else ())
        if i == 0:      # every byte length inside one part (C)
            rest = [k for k in ks if k not in every]
            a, b_, c = rest[:1], rest[1:2], list(every) + rest[2:]
        else:
            na = rng.randint(1, n - 2)
            nb = rng.randint(1, n - 1 - na)
            a, b_, c = ks[:na], ks[na:na + nb], ks[na + nb:]
        rows.append(R.Con({k: coef() for k in a}, {k: coef() for k in b_}, {k: coef() for k in c}))
    return rows


class WideHolder(rsio.InputHolder):
    """The rs_input of the wide system: every signal forbidden, the array made by numpy.arange."""

    def __init__(self, p: int = BN, pname: str = "bn128"):
        self.sys = R.System(p, WIDE_S, 2, 2, 4, {0}, wide_rows(p))
        super().__init__(self.sys, pname)
        self.forb = np.arange(WIDE_S, dtype=np.uint32)
        self.inp.n_forbidden = WIDE_S
        import ctypes as C
        self.inp.forbidden = self.forb.ctypes.data_as(C.POINTER(C.c_uint32))


def le_sorted_lc(m: Dict[int, int], fs: int) -> bytes:
    """One linear combination of a constraint section, entries ordered by the wire's little-endian byte
    string as Python's int.to_bytes gives it (independent of both writers and of pyref._le_key)."""
    out = [struct.pack("<I", len(m))]
    for w in sorted(m, key=lambda w: w.to_bytes(max(1, (w.bit_length() + 7) // 8), "little")):
        out.append(struct.pack("<I", w) + m[w].to_bytes(fs, "little"))
    return b"".join(out)


def constraint_section(cons, fs: int) -> bytes:
    return b"".join(le_sorted_lc(q, fs) for c in cons for q in (c.a, c.b, c.c))


# ============================================================================ both oracles
def oracles_agree(sys_: "R.System", pname: str, key: str):
    """pyref (with its log) and refcpu on one case -> pyref's Result; raises when they differ."""
    fl = fl_of(key)
    res = R.simplification(sys_, rsio.py_flags(fl), want_log=True)
    h = holder(sys_, pname)
    cons, sm, npiw, log = rsio.oracle_run_log(h.inp, fl)
    d = rsio.same_result(res, (cons, sm, len(sm), npiw))
    assert d is None, f"pyref and refcpu differ: {d}"
    assert log == rsio.pyref_log(res.log), "pyref's and refcpu's logs differ"
    return res
