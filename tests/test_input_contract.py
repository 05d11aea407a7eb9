"""CPU proofs for tests/input_contract.py (no GPU): the permutations really leave rows unsorted and are
undone by canonicalising, the validator model accepts every permuted holder and rejects every defect,
the uncertain-row gadget has exactly the count the keys-first boundary needs (certificate = intended,
pyref = refcpu), and pyref's big-int arithmetic agrees with refcpu on the edge-coefficient systems."""
import pytest

import dispatch_shapes as ds
import input_contract as ic
import rsio

R = rsio.R
BN = R.PRIMES["bn128"]


def _bases():
    """(name, holder, le_bytes applies) of the order-is-free cases, as tests/test_gpu_input_contract.py builds them."""
    out = []
    for pname, p in (("bn128", BN), ("goldilocks", R.PRIMES["goldilocks"]), (None, ic.F257)):
        tag = pname or "F_257"
        out += [(f"gen-{tag}", rsio.InputHolder(rsio.gen_system(21, p, n_sig=120, n_rows=200), pname), False),
                (f"gen_big-{tag}", rsio.InputHolder(rsio.gen_system(22, p, n_sig=120, n_rows=200, big_cluster=400), pname), False),
                (f"lengths-{tag}", rsio.InputHolder(ic.lengths_system(p), pname), True)]
    return out


# ---------------------------------------------------------------------------- the named literals
def test_named_literals_resolve_and_move_the_cases():
    k, umin, udiv = ds.constant("kSortInsertMax"), ds.constant("kUncMin"), ds.constant("kUncDiv")
    assert k > 3 and umin > 0 and udiv > 0
    assert ic.row_lengths() == [1, 2, 3, k - 1, k, k + 1, 64, 65, 200]
    assert ic.unc_cap(0) == umin and ic.unc_cap(10 * umin * udiv) == 10 * umin
    # the sources use the names where the literals stood
    assert "m <= kSortInsertMax" in ds._text("kernels.hpp")
    assert "std::max<uint64_t>(kUncMin, lin.n / kUncDiv)" in ds._text("run.hpp")


def test_lengths_system_has_every_length_in_every_block():
    h = rsio.InputHolder(ic.lengths_system(BN), "bn128")
    want = set(ic.row_lengths())
    for q in (ic.LIN, ic.NLA, ic.NLB, ic.NLC):
        b = h.blocks[q]
        have = {ic.rows_of(b, r)[1] - ic.rows_of(b, r)[0] for r in range(int(b.lc.n_rows))}
        assert want - have <= ({1} if q == ic.LIN else set()), (ic.BLOCKS[q], sorted(want - have))
    c = h.blocks[ic.NLC]
    assert any(ic.rows_of(c, r)[0] == ic.rows_of(c, r)[1] for r in range(int(c.lc.n_rows)))  # empty nl_c rows
    assert int(h.blocks[ic.LIN].col.max()) > 255
    # eq rows with both ends forbidden, each a cluster of its own
    forb = set(int(f) for f in h.forb)
    e = h.blocks[ic.EQ]
    both = [tuple(int(x) for x in e.col[2 * r:2 * r + 2]) for r in range(int(e.lc.n_rows))
            if all(int(x) in forb for x in e.col[2 * r:2 * r + 2])]
    assert len(both) >= 2
    for x, y in both:
        assert sum(int(k) in (x, y) for k in e.col[: int(e.lc.nnz)]) == 2


# ---------------------------------------------------------------------------- permutations, validator
@pytest.mark.parametrize("name,h,le", _bases(), ids=[b[0] for b in _bases()])
def test_permutations_unsort_validate_and_canonicalise(name, h, le):
    assert ic.invalid(h) is None
    assert all(ic.not_ascending(b) == 0 for b in h.blocks)
    cases = ic.order_cases(le)
    assert {k for k, _ in cases} == set(ic.KINDS) - (set() if le else {"le_bytes"})
    for kind, blocks in cases:
        g, cnt = ic.permute(h, kind, blocks, seed=11)
        assert set(cnt) == set(blocks)
        assert all(cnt[q] > 0 for q in blocks), (name, kind, {ic.BLOCKS[q]: n for q, n in cnt.items()})
        assert all(ic.not_ascending(g.blocks[q]) == 0 for q in range(6) if q not in blocks)
        assert ic.invalid(g) is None, (kind, blocks)
        assert not ic.same_arrays(g, h)
        assert ic.same_arrays(ic.canonical(g), h), (kind, blocks)


def _defect_bases():
    out = [("bn128", rsio.InputHolder(ic.lengths_system(BN), "bn128")),
           ("goldilocks", rsio.InputHolder(ic.lengths_system(R.PRIMES["goldilocks"]), "goldilocks")),
           ("F_257", rsio.InputHolder(ic.lengths_system(257)))]
    return out


@pytest.mark.parametrize("pname,h", _defect_bases(), ids=[b[0] for b in _defect_bases()])
def test_validator_rejects_every_defect(pname, h):
    assert ic.invalid(h) is None
    applied = set()
    for name in ic.DEFECTS:
        for q in range(6):
            g = ic.defect(h, name, q)
            if g is None:
                continue
            applied.add((name, q))
            assert ic.invalid(g) is not None, (name, ic.BLOCKS[q])
            assert ic.invalid(h) is None    # the original is untouched
    small = pname != "bn128"
    for name in ic.DEFECTS:
        blocks = {q for n, q in applied if n == name}
        if name == "value_limb1" and not small:
            assert blocks == set()          # 2^64 is canonical for a 254-bit prime
        elif name.startswith("dup_apart"):
            assert blocks == {ic.LIN, ic.NLA, ic.NLB, ic.NLC}, name   # rows of three entries or more
        else:
            assert blocks == set(range(6)), name
        assert blocks == set(ic.defect_blocks(name, ic.prime_of(h))), name   # (what the GPU test counts on)
    # the unsorted duplicates sit apart, in rows on either side of the sort threshold
    k = ds.constant("kSortInsertMax")
    for name, lo, hi in (("dup_apart_short", 3, k), ("dup_apart_long", k + 1, 1 << 30)):
        g = ic.defect(h, name, ic.LIN)
        b = g.blocks[ic.LIN]
        rows = [r for r in range(int(b.lc.n_rows)) if len(set(b.col[slice(*ic.rows_of(b, r))].tolist())) < ic.rows_of(b, r)[1] - ic.rows_of(b, r)[0]]
        assert len(rows) == 1
        s, e = ic.rows_of(b, rows[0])
        assert lo <= e - s <= hi and b.col[s] == b.col[e - 1] and ic.not_ascending(b) == 1


# ---------------------------------------------------------------------------- keys first: the gadget
def _gadget_sizes():
    base = ic.unc_cap(0)
    return [base - 1, base, base + 1]


@pytest.mark.parametrize("total", _gadget_sizes())
def test_uncertain_gadget_certificate(total):
    n_dup = total // 2
    sys_ = ic.uncertain_gadget(n_dup, total - n_dup, BN)
    n_lin = len(R.classify(sys_)[2])
    assert n_lin // ds.constant("kUncDiv") < ds.constant("kUncMin")   # so unc_cap is kUncMin
    assert ic.unc_cap(n_lin) == ds.constant("kUncMin")
    assert ic.uncertain_rows(sys_) == total
    # each kind alone
    assert ic.uncertain_rows(ic.uncertain_gadget(7, 0, BN)) == 7
    assert ic.uncertain_rows(ic.uncertain_gadget(0, 5, BN)) == 5
    h = rsio.InputHolder(sys_, "bn128")
    fl = rsio.flags("O2")
    res = R.simplification(sys_, rsio.py_flags(fl))
    ref, _, _ = rsio.oracle_run(h.inp, fl)
    assert rsio.same_result(res, ref) is None


def test_plain_system_has_no_uncertain_row():
    assert ic.uncertain_rows(ic.plain_system(BN)) == 0


# ---------------------------------------------------------------------------- edge coefficients
_EDGE_PRIMES = [(nm, p) for nm, p in R.PRIMES.items()] + [(None, ic.F257), (None, ic.F97)]


def test_edge_coefficient_sets():
    for _, p in _EDGE_PRIMES:
        E = ic.edge_coefficients(p)
        assert all(0 < v < p for v in E) and E == sorted(set(E))
        assert {1, 2, p - 1, p - 2, (p + 1) // 2, (p - 1) // 2} <= set(E)
    E = set(ic.edge_coefficients(BN))
    for k in (29, 58, 63, 64, 116, 128, 192, 232):
        assert {(1 << k) - 1, 1 << k, (1 << k) + 1, BN - (1 << k)} <= E
    assert (1 << 255) not in E and ((1 << 256) - 1) % BN in E and ((1 << 64) - 1) in E
    G = set(ic.edge_coefficients(R.PRIMES["goldilocks"]))
    assert (1 << 63) in G and (1 << 64) not in G and ((1 << 128) - 1) % R.PRIMES["goldilocks"] in G


def test_edge_rewrite_keeps_shape_and_the_generator():
    a = rsio.gen_system(5, BN, n_sig=60, n_rows=80)
    e = ic.edge_system(5, BN, n_sig=60, n_rows=80)
    assert [[sorted(m) for m in (c.a, c.b, c.c)] for c in a.rows] == [[sorted(m) for m in (c.a, c.b, c.c)] for c in e.rows]
    assert sum(R.is_equality(c, BN) for c in e.rows) >= sum(R.is_equality(c, BN) for c in a.rows) > 0
    E = set(ic.edge_coefficients(BN))
    assert all(v in E or (R.is_equality(c, BN) and BN - v in E) for c in e.rows for m in (c.a, c.b, c.c) for v in m.values())
    assert ic.invalid(rsio.InputHolder(e, "bn128")) is None


@pytest.mark.parametrize("pname,p", _EDGE_PRIMES, ids=[nm or f"F_{p}" for nm, p in _EDGE_PRIMES])
def test_edge_systems_pyref_equals_refcpu(pname, p):
    for seed, big in ((1, 0), (2, 0), (3, 400)):
        sys_ = ic.edge_system(seed, p, n_sig=60, n_rows=80, big_cluster=big)
        h = rsio.InputHolder(sys_, pname)
        for fl in (rsio.flags("O2"), rsio.flags("O2", rounds=1)):
            res = R.simplification(sys_, rsio.py_flags(fl))
            ref, _, _ = rsio.oracle_run(h.inp, fl)
            assert rsio.same_result(res, ref) is None, (seed, big)
