"""CPU proof of tests/degenerate.py: every case has the shape its name claims, and oracle/pyref.py and
refcpu agree on it (result and substitution log), so tests/test_gpu_degenerate.py cannot pass vacuously.
The exact set of cases is asserted here: a case that stops being built fails."""
import ctypes as C
import struct

import numpy as np
import pytest

import degenerate as D
import dispatch_shapes as ds
import readerio
import rsio
import soundness as S
from circom_cvm_amd import abi

R = rsio.R
P_IDS = [nm for nm, _ in D.PRIMES3]

SINGLETONS = ["max_signal_1", "x_eq_0", "x_eq_c", "x_eq_y", "one_linear", "ab_eq_c", "ab_eq_0", "nl_empty_b", "only_empty_rows",
              "all_forbidden", "no_publics", "no_private_inputs", "single_round", "all_storage_emptied"]
DAGS = ["main_alone_no_constraints", "main_no_locals", "main_only_empty_constraints", "children_without_rows", "constant_only_row",
        "partial_non_linear_rows", "main_first_unreachable_after", "chain_300_deep", "custom_gate_no_locals"]
RANKS = ["no_linear_rows", "one_cluster", "world_minus_1_clusters", "world_clusters", "one_process4_cluster", "no_non_linear_rows",
         "all_forbidden", "round2_one_cluster", "max_signal_1"]


def test_the_exact_set_of_cases():
    assert D.MASKS == tuple(f"{a}{b}{c}{d}" for a in "01" for b in "01" for c in "01" for d in "01")
    assert sorted(D.FLAG_SETS) == ["O1", "O2", "O2round1", "O2round2", "old"]
    assert [nm for nm, _ in D.PRIMES3] == ["bn128", "goldilocks", "f257"]
    for _, p in D.PRIMES3:
        assert list(D.singletons(p)) == SINGLETONS
        assert list(D.dags(p)) == DAGS
        for w in D.WORLDS:
            assert list(D.rank_cases(p, w)) == RANKS == list(D.RANK_CASES)
    assert set(D.SOUND_SINGLETONS) <= set(SINGLETONS) and set(D.ONESHOT_MASKS) <= set(D.MASKS)
    assert D.HOST_TRANSPORT_CASE == ("one_cluster", 2) and D.WORLDS == (2, 3, 4)


# ---------------------------------------------------------------------------- A. the block lattice
@pytest.mark.parametrize("pname", P_IDS)
@pytest.mark.parametrize("family", ["gen", "sat"])
def test_lattice(family, pname):
    base, wit = D.lattice_base(family, pname)
    full = D.class_counts(base)
    assert all(n > 0 for n in full), full
    census = []
    for mask, sys_ in D.lattice_cases(family, pname):
        assert D.class_counts(sys_) == tuple(n if ch == "1" else 0 for n, ch in zip(full, mask)), mask
        ce, eq, lin, nl = R.classify(sys_)
        assert (len(ce), len(eq), len(lin), len(nl)) == D.class_counts(sys_)
        for key in D.FLAG_SETS:
            res = D.oracles_agree(sys_, pname, key)
            census.append((len(sys_.rows), len(res.constraints), len(res.signal_map), len(res.log)))
            if family == "sat":   # no case of the satisfiable family may be left out of the soundness check
                assert S.consistent_log(sys_, res.log), (mask, key)
                S.check(sys_, res, wit)
    assert len(census) == 16 * 5
    assert any(n_out == 0 and wires > 1 for _, n_out, wires, _ in census)
    assert any(n_in > 0 and n_out == 0 for n_in, n_out, _, _ in census)
    assert any(n_in > 0 and n_log == 0 for n_in, _, _, n_log in census)
    assert any(n_in == 0 and n_out == 0 and n_log == 0 for n_in, n_out, _, n_log in census)


# ---------------------------------------------------------------------------- B. singletons
def _shape(res):
    return len(res.constraints), len(res.signal_map), len(res.log)


@pytest.mark.parametrize("pname,p", D.PRIMES3, ids=P_IDS)
def test_singletons(pname, p):
    cases = D.singletons(p)
    got = {}
    for name, sys_ in cases.items():
        for key in D.FLAG_SETS:
            res = D.oracles_agree(sys_, pname, key)
            got[name, key] = res
            if name in D.SOUND_SINGLETONS:
                assert S.consistent_log(sys_, res.log)
                S.check(sys_, res)
    o2 = {name: got[name, "O2"] for name in cases}
    assert _shape(o2["max_signal_1"]) == (0, 1, 0) and cases["max_signal_1"].max_signal == 1
    for name, klass in (("x_eq_0", 0), ("x_eq_c", 0), ("x_eq_y", 1), ("one_linear", 2), ("ab_eq_c", 3), ("ab_eq_0", 3), ("nl_empty_b", 3)):
        assert len(cases[name].rows) == 1 and D.class_counts(cases[name])[klass] == 1, name
    for name in ("x_eq_0", "x_eq_c", "x_eq_y", "one_linear"):      # the one row is eliminated: zero rows, three wires
        assert _shape(o2[name]) == (0, 3, 1), name
    assert _shape(got["one_linear", "O1"]) == (1, 6, 0)              # --O1 keeps a linear row
    assert _shape(o2["ab_eq_c"]) == (1, 6, 0) and _shape(o2["ab_eq_0"]) == (1, 5, 0)
    assert not cases["ab_eq_0"].rows[0].c and not cases["nl_empty_b"].rows[0].b
    r1 = got["nl_empty_b", "O2round1"]         # fix_constraint leaves 0 = C, a linear row that only round 2 takes
    assert _shape(r1) == (1, 4, 0) and not r1.constraints[0].a and _shape(o2["nl_empty_b"]) == (0, 3, 1)
    assert D.class_counts(cases["only_empty_rows"]) == (0, 0, 3, 0) and _shape(o2["only_empty_rows"]) == (0, 3, 0)
    af = cases["all_forbidden"]
    for key in D.FLAG_SETS:     # nothing is eliminated at any level: identity map, empty log
        r = got["all_forbidden", key]
        assert r.signal_map == {i: i for i in range(af.max_signal)} and not r.log, key
    assert len(o2["all_forbidden"].constraints) > 0
    npub = cases["no_publics"]
    assert (npub.n_pub_out, npub.n_pub_in, npub.forbidden) == (0, 0, {0}) and npub.n_priv_in == 4
    for key in D.FLAG_SETS:     # the first private input (signal 1) lost its wire
        r = got["no_publics", key]
        assert 1 not in r.signal_map and 1 in {s.frm for s in r.log} and r.no_private_inputs_witness < 4
    assert cases["no_private_inputs"].n_priv_in == 0 and o2["no_private_inputs"].no_private_inputs_witness == 0
    sr = cases["single_round"]
    assert ds.linear_rounds(sr, None) == 1 and D.class_counts(sr)[2] == 12
    assert all(c.a and c.b for c in o2["single_round"].constraints) and len(o2["single_round"].constraints) > 0
    assert _shape(got["single_round", "O2round2"]) == _shape(o2["single_round"])
    em = cases["all_storage_emptied"]
    assert sum(1 for c in got["all_storage_emptied", "O2round1"].constraints if c.a) > 0
    for key in ("O2", "O2round2", "old"):
        assert sum(1 for c in got["all_storage_emptied", key].constraints if c.a) == 0, key
    assert ds.linear_rounds(em, None) >= 2


@pytest.mark.parametrize("pname,p", D.PRIMES3, ids=P_IDS)
def test_dags(pname, p):
    flat = {}
    for name, (nodes, main, no, npb, npr, forb) in D.dags(p).items():
        sys_, b = R.flatten_dag(p, nodes, main, no, npb, npr, forb)
        ce, eq, lin, nl = R.classify(sys_)
        assert (ce, eq, lin, nl) == (b["cons_eq"], b["eq"], b["linear"], b["non_linear"]), name
        for key in ("O1", "O2", "O2round1"):
            D.oracles_agree(sys_, pname, key)
        flat[name] = (sys_, b)
    n = lambda name: (flat[name][0].max_signal, D.class_counts(flat[name][0]))   # noqa: E731
    assert n("main_alone_no_constraints") == (4, (0, 0, 0, 0))
    assert n("main_no_locals") == (1, (0, 0, 0, 0))
    assert n("main_only_empty_constraints") == (4, (0, 0, 2, 0))
    assert n("children_without_rows") == (7, (0, 0, 0, 0))         # main 2 + child 1 + child 2 + child 1
    s, b = flat["constant_only_row"]
    assert [c.c for c in b["linear"]] == [{0: 7 % p}, {0: 5 % p}, {0: 5 % p}] and not b["cons_eq"]
    assert len(b["eq"]) == 2 and len(b["non_linear"]) == 1
    s, b = flat["partial_non_linear_rows"]
    assert len(b["non_linear"]) == 6 and sum(1 for c in b["non_linear"] if not c.b) == 2
    assert sum(1 for c in b["non_linear"] if not c.a) == 2 and sum(1 for c in b["non_linear"] if c.a and c.b and not c.c) == 2
    assert n("main_first_unreachable_after") == (4, (0, 1, 0, 1))
    s, b = flat["chain_300_deep"]
    assert s.max_signal == 301 and len(s.rows) == 300 and b["witness"] == list(range(301))
    s, b = flat["custom_gate_no_locals"]
    assert s.max_signal == 4 and s.forbidden == {0, 1, 2} and len(s.rows) == 2


# ---------------------------------------------------------------------------- D. ranks with nothing to do
@pytest.mark.parametrize("world", D.WORLDS)
def test_rank_cases(world):
    for pname, p in D.PRIMES3[:1]:
        for name, (sys_, want) in D.rank_cases(p, world).items():
            D.oracles_agree(sys_, pname, "O2")
            n = D.takeable_clusters(sys_)
            if "clusters" in want:
                assert n == want["clusters"], (name, n)
            rel = want["rel"]
            assert {"below": n < world, "at": n == world, "above": n > world, "none": n == 0}[rel], (name, n, world)
            assert ds.linear_rounds(sys_, None) == want["rounds"], name
            if want.get("p4"):
                sh = ds.cluster_shapes(sys_)
                assert len(sh) == 1 and sh[0]["p4"] and not D.class_counts(sys_)[3]
            if "round2_subs" in want:
                assert ds.round2_shapes(sys_)["n_subs"] == want["round2_subs"]
    assert not D.class_counts(D.rank_cases(D.BN, world)["no_non_linear_rows"][0])[3]
    assert not D.class_counts(D.rank_cases(D.BN, world)["no_linear_rows"][0])[2]
    af = D.rank_cases(D.BN, world)["all_forbidden"][0]
    assert len(ds.cluster_shapes(af)) > 0 and af.forbidden == set(range(af.max_signal))


# ---------------------------------------------------------------------------- E. four-byte wires
def test_wide_wires(tmp_path):
    h = D.WideHolder()
    rows = h.sys.rows
    assert len(rows) == 200 and D.class_counts(h.sys) == (0, 0, 100, 100)
    assert all(3 <= len(c.a) + len(c.b) + len(c.c) <= 9 for c in rows)
    used = {k for c in rows for q in (c.a, c.b, c.c) for k in q}
    assert set(D.WIDE_EDGE_IDS) <= used and max(used) < D.WIDE_S == (1 << 24) + 1024
    assert any({D.byte_length(k) for k in q} == {1, 2, 3, 4} for c in rows for q in (c.a, c.b, c.c))
    # keys whose little-endian order is not the numeric one, inside one linear combination
    assert any(sorted(q) != sorted(q, key=lambda w: w.to_bytes(4, "little")) for c in rows for q in (c.a, c.b, c.c))
    # the Python section against pyref's own writer on the same rows (another sort key, the same order)
    want = D.constraint_section(rows, 32)
    assert want == b"".join(R._lc_block(q, 32) for c in rows for q in (c.a, c.b, c.c))
    # the oracle keeps every row and the identity wire map; the host writer rs_write_r1cs on the oracle's
    # own output sorts four-byte wires as Python's to_bytes does
    lib = rsio.oracle_lib()
    out = C.POINTER(abi.RsOutput)()
    fl = rsio.flags("O2")
    assert lib.refcpu_simplify(C.byref(h.inp), C.byref(fl), 1, C.byref(out), None, None) == 0
    try:
        ref = rsio.output_arrays(out.contents)
        cons = rsio.output_to_py(out.contents)[0]
        path = str(tmp_path / "wide.r1cs")
        abi.check(abi.lib().rs_write_r1cs(path.encode(), C.byref(h.inp), out))
    finally:
        lib.refcpu_output_free(out)
    assert ref["n_wires"] == D.WIDE_S and np.array_equal(ref["l2w"], np.arange(D.WIDE_S, dtype=np.int32))
    assert ref["n_constraints"] == 200
    with open(path, "rb") as f:
        data = f.read()
    # (the rows come back in the result's order, every one of them unchanged)
    canon = lambda cs: sorted(tuple(tuple(sorted(q.items())) for q in (c.a, c.b, c.c)) for c in cs)   # noqa: E731
    assert canon(cons) == canon(rows)
    _, body, size = readerio.sections(data)[2]
    want = D.constraint_section(cons, 32)
    assert size == len(want) and data[body:body + size] == want
    assert struct.unpack_from("<I", data, readerio.sections(data)[1][1] + 4 + 32)[0] == D.WIDE_S    # n_wires
