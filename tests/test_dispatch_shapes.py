"""CPU proofs for the dispatch-boundary cases of dispatch_shapes.py (no GPU):
  * the constants parser reads what the sources say, and raises on what it cannot resolve;
  * every case's certificate equals the value the case claims -- N - 1, N or N + 1 of a parsed
    constant -- so tests/test_gpu_dispatch.py runs the kernels at the shapes it names;
  * every file the build's sources include is in the list build() checks for staleness."""
import os
import re

import pytest

import dispatch_shapes as ds
import rsio

R = rsio.R


# ---------------------------------------------------------------------------- the parser
def test_parser_reads_the_sources():
    # several definitions on one line, the #define indirection, launch-site template arguments
    assert (ds.constant("kMergeK"), ds.constant("kMergeO"), ds.constant("kMergeD")) == (ds.k.kMergeK, ds.k.kMergeO, ds.k.kMergeD)
    assert ds.constant("kFwT") == ds.constant("FW_T") and ds.constant("kFwE") == ds.constant("FW_E")
    assert ds.k.kMergeO < ds.k.kMergeK
    src = open(os.path.join(ds.CSRC, "frames_wave.hpp")).read()
    assert int(re.search(r"#define FW_T (\d+)", src).group(1)) == ds.k.kFwT
    src = open(os.path.join(ds.CSRC, "cluster.hpp")).read()
    assert int(re.search(r"kWaveMin = (\d+);", src).group(1)) == ds.k.kWaveMin
    assert f"k_big_main<{ds.k.tail_cap}>" in open(os.path.join(ds.CSRC, "engine.hip")).read()
    assert f"d_big_main_cluster<{ds.k.spec_cap}>" in open(os.path.join(ds.CSRC, "spec_loop.hpp")).read()
    for nm in ds.K._names:
        assert isinstance(getattr(ds.k, nm), int) and getattr(ds.k, nm) > 0


def test_parser_raises_on_what_it_cannot_resolve():
    with pytest.raises(KeyError):
        ds.constant("kNoSuchConstant")
    with pytest.raises(KeyError):
        ds.constant("kFwPT")            # an expression (kFwT / 64), not an integer
    with pytest.raises(KeyError):
        ds.template_arg("engine.hip", "k_no_such_kernel")
    with pytest.raises(KeyError):
        ds.template_arg("kernels.hpp", "d_big_main_cluster")   # only the template's own parameter there


# ---------------------------------------------------------------------------- the gadgets' two facts
def test_forbidden_signals_glue_and_fix_lengths():
    p = R.PRIMES["bn128"]
    b = ds.Builder(1, p)
    g = b.forbid(1)[0]
    for _ in range(5):
        b.lin([g] + b.take(2))
    x = ds.star(b, 7)
    sys_ = b.system()
    sh = ds.cluster_shapes(sys_)
    assert sorted(c["rows"] for c in sh) == [1, 5]
    res = R.simplification(sys_, R.Flags(), want_log=True)
    assert [len(s.to) for s in res.log if s.frm == x] == [7]


# ---------------------------------------------------------------------------- shape proofs
_SHAPES = [(c, old) for c in ds.CASES for old in c.olds]


@pytest.mark.parametrize("case,old", _SHAPES, ids=[f"{c.name}{'-old' if o else ''}" for c, o in _SHAPES])
def test_shape(case, old):
    sys_, info = case.build(R.PRIMES["bn128"])
    checks = case.certify(sys_, info, old)
    assert checks
    for rd, want in (case.n_rounds or {}).items():
        checks.append((f"linear rounds at rounds={rd}", ds.linear_rounds(sys_, rd, old), want))
    bad = [(what, got, want) for what, got, want in checks if got != want or type(got) is not type(want)]
    assert not bad, f"{case.name}: (quantity, certificate, intended) {bad}"


def test_case_table_is_complete():
    """Every boundary of the table appears at each of its values."""
    names = {c.name for c in ds.CASES}
    k = ds.k
    want = set()
    for base, ds_ in (("kWaveMin", (-1, 0, 1)), ("kHeavyNnz", (-1, 0, 1)), ("kClSmall", (0, 1)), ("p4_head", (-1, 0, 1)),
                      ("p4_tail", (-1, 0, 1)), ("kFinWaveBelow", (-1, 0, 1)), ("kClMid_ordered", (-1, 0, 1)),
                      ("kClMid_order_free", (-1, 0, 1)), ("kHeadLimit", (-1, 0, 1)), ("kTailSplit", (0, 1)),
                      ("kSpecTabMax_p4", (-1, 0, 1)), ("kSpecTabMax_p3", (-1, 0, 1)), ("kGiantRows", (-1, 0, 1)), ("kClLds", (0, 1)),
                      ("frames_terms", (-1, 0, 1)), ("frames_entries", (0, 1)), ("frames_batch_terms", (0, 1)),
                      ("frames_batch_entries", (0, 1)), ("frames_runs", (0, 1)), ("frames_fix_terms", (0, 1)),
                      ("giant_merge_sum", (0, 1)), ("round2_terms", (-1, 0, 1)), ("round2_entries", (0, 1))):
        want |= {f"{base}{d:+d}" for d in ds_}
    want |= {"p4_order_free", "p4_one_ordered_row", "kGiantRows_order_free", "frames_fix_65_rows"}
    for where in ("small", "tail", "head"):
        want |= {f"row_{where}_{n}" for n in (k.kSpecK - 1, k.kSpecK, k.kSpecK + 1, k.tail_cap, k.tail_cap + 1, k.spec_cap, k.spec_cap + 1)}
        want |= {f"merge_{where}_{cap}{d:+d}" for cap in (k.tail_cap, k.spec_cap) for d in (0, 1, 2)}
    want |= {f"row_head512_{k.spec_cap + d}" for d in (0, 1)} | {f"merge_head512_{k.spec_cap}{d:+d}" for d in (0, 1, 2)}
    want |= {f"giant_row_{k.kGhRowMax + d}" for d in (0, 1)} | {f"giant_rhs_{k.kGhRhsMax + d}" for d in (0, 1)}
    for t in ("head", "tail"):
        want |= {f"compose_{t}_len64", f"compose_{t}_len65", f"compose_{t}_deps4", f"compose_{t}_deps5"}
        want |= {f"compose_{t}_{b}{d:+d}" for b in ("E", "kMergeO", "kMergeK") for d in (-1, 0, 1)}
        want |= {f"compose_{t}_kMergeD{d:+d}" for d in (0, 1)}
    assert want - names == set()
    # the marked rows: goldilocks (the one-word field path) and the old heuristics
    by = {c.name: c for c in ds.CASES}
    for nm in ("kWaveMin-1", "kWaveMin+0", "kWaveMin+1", "p4_order_free", "p4_one_ordered_row"):
        assert "goldilocks" in by[nm].primes
    for nm in ("kWaveMin+0", "kClSmall+0", "kClSmall+1", "p4_head-1", "p4_head+0", "p4_head+1", "kGiantRows+0", "kClLds+0", "kClLds+1"):
        assert True in by[nm].olds
    # the round-2 cases run under --O2 and --O2round 2 and must make a second linear round that
    # substitutes something (test_shape proves both); every frames case states its round count
    for c in ds.CASES:
        if c.name.startswith("round2_"):
            assert c.rounds == (None, 2) and c.n_rounds == {None: 2, 2: 2}
        if c.name.startswith("frames_"):
            assert c.n_rounds is not None


# ---------------------------------------------------------------------------- the log's reference
_LOGS = {}


def _log_licence(case):
    """(difference between refcpu's log and pyref's literal log, entries with a zero-valued
    non-constant key) of a case at its first variant -- the run tests/test_gpu_dispatch_log.py makes."""
    if case.name not in _LOGS:
        prime, old, rounds = ds.variants(case)[0]
        sys_, _ = case.build(R.PRIMES[prime])
        h = rsio.InputHolder(sys_)
        fl = rsio.flags("O2", rounds, old, log=True)
        ref = rsio.pyref_log(R.simplification(sys_, rsio.py_flags(fl), want_log=True).log)
        got = rsio.oracle_run_log(h.inp, fl, threads=8)[3]
        _LOGS[case.name] = (ds.log_diff(got, ref), len(ds.zero_entries(ref)), len(ref))
    return _LOGS[case.name]


@pytest.mark.parametrize("case", ds.CASES, ids=[c.name for c in ds.CASES])
def test_refcpu_log_is_pyrefs(case):
    """refcpu's substitution log equals pyref's literal one (zero-valued keys kept), entry for entry:
    what makes refcpu the reference of tests/test_gpu_dispatch_log.py.  No case is left out."""
    d, _, _ = _log_licence(case)
    assert d is None, f"refcpu's log differs from pyref's: {d}"


def test_every_family_logs_a_zero_key():
    """At least one log of each family holds a zero-valued non-constant key, so comparing the logs of
    the existing cases already tells a pool that keeps explicit zeros from one that prunes them.
    The round2_* cases cannot hold one whatever their seeds: round 2 meets each late star as a cluster
    of one row, and a zero key needs a composition.  For that family the log counted with theirs is the
    certified round-2 composition of cancel_cases.py (zero_round2), which the GPU runs with the log on
    like the rest."""
    import cancel_cases as cc
    have = {}
    for case in ds.CASES + [c for c in cc.CANCEL_CASES if c.name == "zero_round2"]:
        d, zeros, _ = _log_licence(case)
        assert d is None, f"{case.name}: {d}"
        fam = "round2" if case.name == "zero_round2" else ds.log_family(case.name)
        have[fam] = have.get(fam, 0) + (zeros > 0)
    assert set(have) == {"cluster", "row", "merge", "compose", "giant", "round2", "frames"}
    for fam in ("cluster", "row", "merge", "compose", "giant", "round2"):
        assert have[fam] >= 1, f"no log of the {fam} cases holds a zero-valued non-constant key"


# ---------------------------------------------------------------------------- the build's dependency list
def _includes(path):
    with open(path) as f:
        return re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), flags=re.M)


def test_build_dependency_list_covers_every_include():
    """Starting from build.SOURCES and cli.cpp, every quoted #include (transitively) is a file build()
    checks for staleness: a change to any of them rebuilds librs_simplify.so."""
    from circom_cvm_amd import build as B
    listed = {os.path.normpath(os.path.join(B.CSRC, f)) for f in B.SOURCES + B.HEADERS}
    todo = [os.path.normpath(os.path.join(B.CSRC, f)) for f in B.SOURCES + ["cli.cpp"]]
    seen = set(todo)
    while todo:
        cur = todo.pop()
        for inc in _includes(cur):
            path = os.path.normpath(os.path.join(os.path.dirname(cur), inc))
            assert os.path.exists(path), f"{cur} includes {inc}, which does not exist"
            if path not in seen:
                seen.add(path)
                todo.append(path)
    missing = sorted(os.path.relpath(f, B.CSRC) for f in seen - listed - {os.path.normpath(os.path.join(B.CSRC, "cli.cpp"))})
    assert missing == [], f"included but not in build.py's dependency list: {missing}"
