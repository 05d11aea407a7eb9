"""The input contract of include/rs_simplify.h on the GPU, through every entry path (load = rs_engine_load
/ run / fetch, simplify = rs_engine_simplify on a pageable input, oneshot = rs_simplify, group2 = two
engines of an in-process group on device 0).  Order is free: rows arrive in any key order and the result
equals the oracle's on the canonical form (keys ascending), bit for bit.  Malformed input: every defect
class of tests/input_contract.py is RS_E_INVALID and the engine runs a valid input right after.  The
keys-first load of rs_engine_simplify at unc_cap - 1, unc_cap and unc_cap + 1 uncertain rows, with the
branch read from the library's own RS_PROF lines.  Coefficients on the carry and limb edges of field.hpp
for every prime.  The shapes are proved on the CPU by tests/test_input_contract.py."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import input_contract as ic
import rsio
import circom_cvm_amd as M
from circom_cvm_amd import abi

pytestmark = pytest.mark.gpu
R = rsio.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BN, GL = R.PRIMES["bn128"], R.PRIMES["goldilocks"]
PRIMES3 = [("bn128", BN), ("goldilocks", GL), (None, ic.F257)]
P3_IDS = ["bn128", "goldilocks", "F_257"]
FLAGS = {"O2": ("O2", None), "O1": ("O1", None), "O2round1": ("O2", 1)}
_ENG = None
_GROUP = None


def engine():
    global _ENG
    if _ENG is None:
        _ENG = M.Engine(0)
    return _ENG


def group2():
    global _GROUP
    if _GROUP is None:
        g = M.Group(2)
        engs = [M.Engine(0) for _ in range(2)]
        for r, e in enumerate(engs):
            e.join_group(g, r)
        _GROUP = (g, engs)
    return _GROUP[1]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    global _ENG, _GROUP
    if _ENG is not None:
        _ENG.close()
        _ENG = None
    if _GROUP is not None:
        for e in _GROUP[1]:
            e.close()
        _GROUP[0].close()
        _GROUP = None


def fl_of(name):
    return rsio.flags(*FLAGS[name])


# ---------------------------------------------------------------------------- the entry paths
def run_path(path, inp, fl):
    """The result arrays of `inp` through one entry path (group2: every rank's)."""
    e = engine()
    if path == "load":
        e.load(inp)
        e.run(fl)
        out = e.fetch()
        return [rsio.output_arrays(out.c)]
    if path == "simplify":
        return [rsio.output_arrays(e.simplify(inp, fl))]
    if path == "oneshot":
        out = C.POINTER(abi.RsOutput)()
        abi.check(abi.lib().rs_simplify(C.byref(inp), C.byref(fl), C.byref(out)))
        try:
            return [rsio.output_arrays(out.contents)]
        finally:
            abi.lib().rs_output_free(out)
    assert path in ("group2_load", "group2_simplify")
    outs, errs = group_call(path, inp, fl)
    for ex in errs:
        if ex is not None:
            raise ex
    return outs


def group_call(path, inp, fl):
    """Both ranks of the group run `inp`; -> (per-rank arrays, per-rank exception)."""
    engs = group2()
    outs, errs = [None, None], [None, None]

    def work(r):
        try:
            if path == "group2_simplify":
                outs[r] = rsio.output_arrays(engs[r].simplify(inp, fl))
            else:
                engs[r].load(inp)
                engs[r].run(fl)
                o = engs[r].fetch()
                outs[r] = rsio.output_arrays(o.c)
        except Exception as ex:  # noqa: BLE001 -- returned
            errs[r] = ex

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
        assert not t.is_alive(), "a rank of the group hung"
    return outs, errs


def assert_matches(path, inp, fl, ref, what):
    for r, got in enumerate(run_path(path, inp, fl)):
        d = rsio.diff_output_arrays(got, ref)
        assert d is None, f"{what} via {path} (rank {r}): {d}"


_BASES = {}


def base(name, pname, p):
    """The canonical holder of a base system (cached) and its oracle results per flag."""
    key = (name, p)
    if key not in _BASES:
        if name == "lengths":
            sys_ = ic.lengths_system(p)
        else:
            sys_ = rsio.gen_system(21 if name == "gen" else 22, p, n_sig=120, n_rows=200, big_cluster=400 if name == "gen_big" else 0)
        _BASES[key] = (rsio.InputHolder(sys_, pname), {})
    h, refs = _BASES[key]
    return h, refs


def ref_of(h, refs, flname):
    if flname not in refs:
        refs[flname] = rsio.oracle_arrays(h.inp, fl_of(flname))[0]
    return refs[flname]


# ---------------------------------------------------------------------------- order is free
@pytest.mark.parametrize("pname,p", PRIMES3, ids=P3_IDS)
@pytest.mark.parametrize("name", ["gen", "gen_big", "lengths"])
def test_order_is_free(name, pname, p):
    """Every permutation kind on each block alone and on all six, at --O2, --O1 and --O2round 1: load and
    simplify equal the oracle on the canonical form."""
    h, refs = base(name, pname, p)
    for kind, blocks in ic.order_cases(name == "lengths"):
        g, cnt = ic.permute(h, kind, blocks, seed=11)
        assert all(cnt[q] > 0 for q in blocks), (kind, cnt)
        for flname in FLAGS:
            ref = ref_of(h, refs, flname)
            for path in ("load", "simplify"):
                assert_matches(path, g.inp, fl_of(flname), ref, f"{name} {kind} {[ic.BLOCKS[q] for q in blocks]} {flname}")


@pytest.mark.parametrize("pname,p", PRIMES3, ids=P3_IDS)
@pytest.mark.parametrize("name", ["gen", "gen_big", "lengths"])
@pytest.mark.parametrize("path", ["oneshot", "group2_load", "group2_simplify"])
def test_order_is_free_other_paths(path, name, pname, p):
    """The all-blocks random case through rs_simplify and on both ranks of an in-process group, on every
    base system at --O2, --O1 and --O2round 1."""
    h, refs = base(name, pname, p)
    g, cnt = ic.permute(h, "random", range(6), seed=11)
    assert all(n > 0 for n in cnt.values())
    for flname in FLAGS:
        assert_matches(path, g.inp, fl_of(flname), ref_of(h, refs, flname), f"{name} random all {flname}")


def test_order_of_an_r1cs_file(tmp_path):
    """An --O0 .r1cs stores a row's keys by their little-endian byte strings: with ids above 255 the rows
    rs_engine_read_r1cs_o0 hands over are not all ascending, and rs_engine_simplify takes them as they are."""
    sys_ = ic.lengths_system(BN)
    ident = R.Result(sys_.rows, {i: i for i in range(sys_.max_signal)}, sys_.n_priv_in)
    data = R.result_to_r1cs(sys_, ident)
    path = str(tmp_path / "lengths_O0.r1cs")
    with open(path, "wb") as f:
        f.write(data)
    canon = rsio.InputHolder(R.read_r1cs_bytes(data)[0], "bn128")   # the same rows, keys ascending
    e = engine()
    view = e.read_r1cs(path)
    unsorted = 0
    for nm in ("linear", "nl_a", "nl_b", "nl_c"):
        blk = getattr(view, nm)
        want = getattr(canon.inp, nm)
        assert (blk.n_rows, blk.nnz) == (want.n_rows, want.nnz)
        ptr, col, _ = rsio._lc_arrays(blk)
        unsorted += sum(bool((np.diff(col[int(ptr[r]):int(ptr[r + 1])].astype(np.int64)) <= 0).any())
                        for r in range(int(blk.n_rows)))
    assert unsorted > 0
    for flname in FLAGS:
        fl = fl_of(flname)
        ref, _ = rsio.oracle_arrays(canon.inp, fl)
        d = rsio.diff_output_arrays(rsio.output_arrays(e.simplify(view, fl)), ref)
        assert d is None, (flname, d)


# ---------------------------------------------------------------------------- malformed input
_GOOD = {}


def _good():
    if not _GOOD:
        h = rsio.InputHolder(rsio.gen_system(7, BN, n_sig=80, n_rows=150), "bn128")
        _GOOD["h"], _GOOD["ref"] = h, rsio.oracle_arrays(h.inp, rsio.flags("O2"))[0]
    return _GOOD["h"], _GOOD["ref"]


def expect_invalid(path, g, what):
    """`g` is RS_E_INVALID through `path`; then a valid input on the same engine equals the oracle."""
    fl = rsio.flags("O2")
    with pytest.raises(M.RsError) as ei:
        run_path(path, g.inp, fl)
    assert ei.value.code == -1, (what, path, str(ei.value))
    h, ref = _good()
    assert_matches(path, h.inp, fl, ref, f"the valid input after {what}")


@pytest.mark.parametrize("defect", list(ic.DEFECTS))
def test_malformed_is_rejected(defect):
    """Every defect class in every block that has a place for it, on load and on simplify.  (Value
    defects of `eq` on simplify: test_eq_values_*.)  The value defects sit in the last entry of the
    block, so on simplify a sorted linear block is rejected only when its values land, after the
    clustering has begun on its keys (keys first: test_keys_first_boundaries runs that case again and
    reads the branch)."""
    tried, want = set(), set()
    for pname, p in PRIMES3:
        h, _ = base("lengths", pname, p)
        assert ic.invalid(h) is None
        for q in ic.defect_blocks(defect, p):       # (proved on the CPU: exactly the blocks with a place for it)
            for path in ("load", "simplify"):
                if not (path == "simplify" and q == ic.EQ and defect in ic.VALUE_DEFECTS):
                    want.add((p, q, path))
        for q in range(6):
            g = ic.defect(h, defect, q)
            if g is None:
                continue
            assert ic.invalid(g) is not None
            for path in ("load", "simplify"):
                if path == "simplify" and q == ic.EQ and defect in ic.VALUE_DEFECTS:
                    continue
                expect_invalid(path, g, f"{defect} in {ic.BLOCKS[q]} ({pname or 'F_257'})")
                tried.add((p, q, path))
    assert tried == want and tried, sorted(want - tried)


@pytest.mark.parametrize("defect,q", [("value_eq_p", ic.LIN), ("key_eq_max_signal", ic.NLA)])
@pytest.mark.parametrize("path", ["group2_load", "group2_simplify"])
def test_malformed_on_a_group(path, defect, q):
    """Both ranks reject (RS_E_INVALID, or RS_E_RCCL for a rank released from a collective by the other's
    failure), and the group's next call equals the oracle on every rank."""
    h, _ = base("lengths", "bn128", BN)
    g = ic.defect(h, defect, q)
    fl = rsio.flags("O2")
    outs, errs = group_call(path, g.inp, fl)
    assert all(isinstance(e, M.RsError) and e.code in (-1, -4) for e in errs), errs
    assert any(e.code == -1 for e in errs), errs
    good, ref = _good()
    assert_matches(path, good.inp, fl, ref, f"the group's next call after {defect}")


def _eq_rows(h):
    """(rows of eq with both ends forbidden, the others)."""
    forb = set(int(f) for f in h.forb)
    b = h.blocks[ic.EQ]
    kept = [r for r in range(int(b.lc.n_rows)) if all(int(k) in forb for k in b.col[slice(*ic.rows_of(b, r))])]
    return kept, [r for r in range(int(b.lc.n_rows)) if r not in kept]


@pytest.mark.parametrize("pname,p", PRIMES3, ids=P3_IDS)
@pytest.mark.parametrize("order", ["ascending", "reversed"])
def test_eq_values_of_kept_rows_are_checked(order, pname, p):
    """rs_engine_simplify reads the values of the eq rows it keeps (both ends forbidden, a cluster of
    their own) from the host input: a zero or non-canonical one is RS_E_INVALID, in either key order.
    Under the primes below 2^64 also 2^64, whose limb 0 alone is zero and whose limb 1 a one-word
    comparison would not see."""
    h, _ = base("lengths", pname, p)
    kept, _ = _eq_rows(h)
    assert len(kept) >= 2
    values = [0, p, (1 << 256) - 1] + ([1 << 64, (1 << 64) + 1] if p < (1 << 64) else [])
    assert (len(values) == 5) == (pname != "bn128")
    for v in values:
        for which in (0, 1):
            g = ic.copy_holder(h)
            ic._set_val(g.blocks[ic.EQ], ic.rows_of(g.blocks[ic.EQ], kept[-1])[0] + which, v)
            if order == "reversed":
                g, _ = ic.permute(g, "reversed", [ic.EQ])
            assert ic.invalid(g) is not None
            for path in ("simplify", "load"):
                expect_invalid(path, g, f"value {v:#x} in a kept eq row")


def test_eq_values_of_eliminated_rows_are_not_inspected_by_simplify():
    """The other half (include/rs_simplify.h): rs_engine_simplify never uploads the values of eq; a zero
    value in a row the run eliminates is accepted and the result equals the oracle on the clean input
    (the reference does not read these values either).  rs_engine_load validates every value."""
    h, refs = base("lengths", "bn128", BN)
    _, gone = _eq_rows(h)
    g = ic.copy_holder(h)
    for r in gone[:3]:
        ic._set_val(g.blocks[ic.EQ], ic.rows_of(g.blocks[ic.EQ], r)[0], 0)
    assert ic.invalid(g) is not None
    for flname in FLAGS:
        assert_matches("simplify", g.inp, fl_of(flname), ref_of(h, refs, flname), f"zero values in eliminated eq rows {flname}")
    expect_invalid("load", g, "zero values in eliminated eq rows")


# ---------------------------------------------------------------------------- keys first
def _child(case):
    env = {**os.environ, "RS_PROF": "1"}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "keysfirst_child.py"), case], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    first = r.stderr.split("[child] rejected")[0]    # the first call's lines
    branch = re.findall(r"\[rs-prof\] linear rows: (keys first|keys \+ values)", first)
    settled = [int(x) for x in re.findall(r"\[rs-prof\] keys-first: (\d+) rows settled from host values", first)]
    return res, branch, settled


@pytest.mark.parametrize("case", ["cap-1", "cap", "cap+1", "cap_reversed", "plain", "late_bad_value"])
def test_keys_first_boundaries(case):
    """rs_engine_simplify's keys-first load with the uncertain-row list one short of full, exactly full
    and overflowing by one (the guard holds, the frames run on values), with the unsorted flag, and
    without any uncertain row: the branch the run reports is the expected one, the number of rows it
    settled from host values is the CPU certificate, and the result equals the oracle.  late_bad_value: a
    zero value behind sorted keys is rejected after the keys-first branch was taken, and the engine
    recovers."""
    res, branch, settled = _child(case)
    cap = res["unc_cap"]
    want_n = {"cap-1": cap - 1, "cap": cap, "cap+1": cap + 1, "cap_reversed": cap, "plain": 0, "late_bad_value": cap - 1}[case]
    assert res["uncertain"] == want_n
    assert res["diff"] is None, res
    if case == "cap_reversed":
        assert res["not_ascending"] == 1 and branch == ["keys + values"] and settled == []
    elif case == "cap+1":     # the list overflowed: nothing was settled from host values, and the run says nothing of the kind
        assert res["not_ascending"] == 0 and branch == ["keys + values"] and settled == []
    else:
        assert res["not_ascending"] == 0 and branch == ["keys first"] and settled == [want_n]
    assert res["code"] == (-1 if case == "late_bad_value" else 0)


# ---------------------------------------------------------------------------- edge coefficients
_EDGE_PRIMES = [(nm, p) for nm, p in R.PRIMES.items()] + [(None, ic.F257)]


@pytest.mark.parametrize("pname,p", _EDGE_PRIMES, ids=[nm or f"F_{p}" for nm, p in _EDGE_PRIMES])
def test_edge_coefficients(pname, p):
    """Systems whose every coefficient sits on a carry or limb edge, with and without a process_4
    cluster, at --O2 and --O2round 1, on load and simplify: equal to refcpu, and for the three
    smallest to pyref's big-int arithmetic directly."""
    for seed, big in ((1, 0), (2, 0), (3, 0), (4, 400), (5, 400)):
        sys_ = ic.edge_system(seed, p, n_sig=60, n_rows=80, big_cluster=big)
        h = rsio.InputHolder(sys_, pname)
        for flname in ("O2", "O2round1"):
            fl = fl_of(flname)
            ref, _ = rsio.oracle_arrays(h.inp, fl)
            for path in ("load", "simplify"):
                assert_matches(path, h.inp, fl, ref, f"edge seed {seed} {flname}")
            if not big:
                e = engine()
                e.load(h.inp)
                e.run(fl)
                out = e.fetch()
                res = R.simplification(sys_, rsio.py_flags(fl))
                assert rsio.same_result(res, rsio.output_to_py(out.c)) is None, (seed, flname)
