"""The certified cases on the SHARDED path: in-process groups of 2, 3 and 4 engines on device 0 (the
groups of tests/test_gpu_sharded.py), every rank compared with the single-engine CPU oracle.

  test_deal              the deal's remainders (shard_cases.deal_cases): every rank's arrays, the
                         counters equal over ranks, and per rank a tail / lane launch exactly when
                         shard_cases.owner_of deals it a tail / lane cluster;
  test_dispatch_sharded  the 141 dispatch cases (and the two shard_cases adds) at world 3, log off (the
                         filtered exchange) and log on (`need` null: every right-hand side travels),
                         arrays and log against refcpu's, and rs_stats.exchange_bytes of the two runs
                         against the CPU model's filtered right-hand sides;
  test_cancel_sharded    the 44 certified cancellations at world 2 through load / run / fetch and
                         rs_engine_simplify, log on and off.

tests/test_shard_cases.py proves on the CPU which of these exchange the cluster they are about, and
that the filter both keeps and drops something in every family.  The log is what shows a right-hand
side copied wrongly through the pack, the gather, the unpack or the re-pointing behind the gathered
pool: the arrays stay right whenever the signal is not relevant.

One group per world serves every case of the module; an ordinary input runs after every twentieth
case and the empty input after the largest, both against the oracle (stale state)."""
import threading

import pytest

import dispatch_shapes as ds
import rsio
import shard_cases as sc
import test_gpu_sharded as SH

R = rsio.R
pytestmark = pytest.mark.gpu
BN = R.PRIMES["bn128"]
JOIN_S = 120
PYREF_BELOW = 2000
_COUNT = {}
_STALE = {}
_REPEATED = []      # dispatch cases whose first run exchanged more than once (see test_dispatch_sharded)


@pytest.fixture(scope="module", autouse=True)
def _release():
    """The groups' engines go when the module is done (later modules need the device memory)."""
    yield
    SH.release_groups()


def run_ranks(inp, fl, world, path="load"):
    """SH.sharded_run / SH.sharded_simplify with the log: per rank (arrays, log, stats)."""
    engs = SH.group(world)
    outs, errs = [None] * world, [None] * world

    def work(r):
        try:
            if path == "load":
                engs[r].load(inp)
                engs[r].run(fl)
                out = engs[r].fetch()  # owns the rs_output while it is read
                o = out.c
            else:
                o = engs[r].simplify(inp, fl)  # views the engine's buffers until its next call
            outs[r] = (rsio.output_arrays(o), rsio.output_log(o), engs[r].stats())
        except Exception as ex:  # noqa: BLE001 -- reported below
            errs[r] = ex

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=JOIN_S)
        assert not t.is_alive(), "a rank of the sharded run hung"
    for e in errs:
        if e is not None:
            raise e
    return outs


def check_ranks(outs, ref, ref_log, what):
    world = len(outs)
    for r, (got, log, st) in enumerate(outs):
        d = rsio.diff_output_arrays(got, ref)
        assert d is None, f"{what}: rank {r}/{world}: {d}"
        d = ds.log_diff(log, ref_log)
        assert d is None, f"{what}: rank {r}/{world}: log: {d}"
        assert int(st.world) == world
    for f in ("n_substitutions", "n_clusters", "rounds", "exchange_bytes"):
        assert len({int(getattr(st, f)) for _, _, st in outs}) == 1, f"{what}: {f} differs over the ranks"


def _stale(which):
    if which not in _STALE:
        sys_ = rsio.gen_system(7, BN, n_sig=80, n_rows=150) if which == "ordinary" else R.System(BN, 80, 1, 1, 2, {0, 1, 2}, [])
        h = rsio.InputHolder(sys_, "bn128")
        fl = rsio.flags("O2", log=True)
        _STALE[which] = (h, fl, rsio.oracle_arrays(h.inp, fl)[0], rsio.oracle_run_log(h.inp, fl)[3])
    return _STALE[which]


def after_case(world, largest=False):
    """The group's next call is an ordinary input after every twentieth case, the empty one after the
    largest."""
    _COUNT[world] = _COUNT.get(world, 0) + 1
    for which, due in (("ordinary", _COUNT[world] % 20 == 0), ("empty", largest)):
        if due:
            h, fl, ref, ref_log = _stale(which)
            for path in ("load", "simplify"):
                check_ranks(run_ranks(h.inp, fl, world, path), ref, ref_log, f"the {which} input via {path} after case {_COUNT[world]}")


# ---------------------------------------------------------------------------- the deal
_DEALS = [(w, c) for w in sc.DEAL_WORLDS for c in sc.deal_cases(w)]
_DEAL_REF = {}


def _deal_ref(case):
    if case.name not in _DEAL_REF:
        sys_, _ = case.build(BN)
        h = rsio.InputHolder(sys_)
        _DEAL_REF[case.name] = (h, rsio.oracle_arrays(h.inp, rsio.flags("O2"), threads=8)[0], ds.cluster_shapes(sys_))
    return _DEAL_REF[case.name]


@pytest.mark.parametrize("world,case", _DEALS, ids=[f"{c.name}-w{w}" for w, c in _DEALS])
def test_deal(world, case):
    """rs_stats.tail_launches and small_launches both count the rank's own share: run_linear_simplification
    replaces n_big / n_small by the rank's (n_rep + snake_count(n_tb), snake_count(n_small)) before the
    launches, and the counters add `n_tgroups` when n_tail = n_big - n_head is non-zero and 1 when
    n_small is."""
    h, ref, shapes = _deal_ref(case)
    share = sc.shares(shapes, world)
    outs = run_ranks(h.inp, rsio.flags("O2"), world)
    check_ranks(outs, ref, [], case.name)
    for r, (_, _, st) in enumerate(outs):
        assert int(st.n_clusters) == len(shapes) == ds.k.kHeadLimit + case.t + case.s and int(st.rounds) == 1
        assert (int(st.tail_launches) > 0) == bool(share["tail"][r]), f"rank {r}: tail_launches {int(st.tail_launches)}, dealt {share['tail'][r]}"
        assert (int(st.small_launches) > 0) == bool(share["lane"][r]), f"rank {r}: small_launches {int(st.small_launches)}, dealt {share['lane'][r]}"
        assert int(st.head_launches) == 1
    after_case(world)


# ---------------------------------------------------------------------------- the dispatch cases
_DISPATCH = sc.SHARD_DISPATCH + sc.SHARD_EXTRA


@pytest.mark.parametrize("case", _DISPATCH, ids=[c.name for c in _DISPATCH])
def test_dispatch_sharded(case):
    """Both runs of a case share its build and its oracle results.  The single-engine launch counters
    of case.stats are not asserted: the deal changes them by design."""
    world = sc.DISPATCH_WORLD
    prime, old, rounds = sc.first_variant(case)
    sys_, _ = case.build(R.PRIMES[prime])
    h = rsio.InputHolder(sys_)
    off, on = rsio.flags("O2", rounds, old), rsio.flags("O2", rounds, old, log=True)
    ref, _ = rsio.oracle_arrays(h.inp, off, threads=8)
    ref_log = rsio.oracle_run_log(h.inp, on, threads=8)[3]
    st = {}
    for key, fl, want_log in (("on", on, ref_log), ("off", off, [])):
        outs = run_ranks(h.inp, fl, world)
        check_ranks(outs, ref, want_log, f"{case.name}, log {key}")
        st[key] = outs[0][2]
        if case.n_rounds is not None:
            assert int(st[key].rounds) == case.n_rounds[rounds]
    # exchange_bytes: 16 per record, 36 per entry, 24 per rank and exchange (shard_exchange); one exchange
    # with the log on differs from one with it off by the entries the filter dropped.  The counter adds
    # up every exchange that ran, also the one of an attempt whose head then ran out of pool and was
    # repeated with a larger one (run_linear_simplification's attempt loop: the tail is done and
    # exchanged while the head is still going).  The engine remembers the pool that fitted, so only the
    # first run of an input can repeat: the log-on run goes first and may hold a whole number of
    # exchanges (at most the loop's eight attempts), the log-off run holds exactly one.
    n_rounds = int(st["off"].rounds)
    assert n_rounds == int(st["on"].rounds)
    log1 = ref_log if n_rounds == 1 else rsio.oracle_run_log(h.inp, rsio.flags("O2", 1, old, log=True), threads=8)[3]
    model = sc.exchange_model(sys_, R.Flags(use_old_heuristics=old), world, log1=log1)
    b_on, b_off = int(st["on"].exchange_bytes), int(st["off"].exchange_bytes)
    print(f"{case.name}: rounds {n_rounds}, exchange_bytes on {b_on} off {b_off}, model: {len(model['exchanged'])} exchanged, "
          f"{len(model['dropped'])} dropped, {sc.filtered_bytes(model)} bytes")
    if n_rounds == 1:
        one = b_off + sc.filtered_bytes(model)
        assert (b_on == 0 if one == 0 else b_on % one == 0 and 1 <= b_on // one <= 8), f"log on {b_on}, log off {b_off}, filtered by the model {sc.filtered_bytes(model)}"
        if b_on != one:
            _REPEATED.append(case.name)
    else:
        assert b_on >= b_off
        if model["dropped"]:
            assert b_on > b_off
    after_case(world, largest=case.name == sc.LARGEST["dispatch"])


def test_repeated_exchanges_are_few():
    """A run repeats its exchange only when its pool has to grow, the pool then at least doubles (or takes
    what the device has left) and the engines remember it: from the 2^20 entries an engine starts with
    to 2^27 (4.8 GB, more than any case here fills) that is seven cases at the most.  Every other case met
    the byte equality with one exchange on each side."""
    assert len(_REPEATED) <= 7, _REPEATED


# ---------------------------------------------------------------------------- the cancellations
@pytest.mark.parametrize("case", sc.SHARD_CANCEL, ids=[c.name for c in sc.SHARD_CANCEL])
def test_cancel_sharded(case):
    world = sc.CANCEL_WORLD
    prime, old, rounds = sc.first_variant(case)
    sys_, _ = case.build(R.PRIMES[prime])
    h = rsio.InputHolder(sys_)
    off, on = rsio.flags("O2", rounds, old), rsio.flags("O2", rounds, old, log=True)
    ref, _ = rsio.oracle_arrays(h.inp, off, threads=8)
    ref_log = rsio.oracle_run_log(h.inp, on, threads=8)[3]
    if len(sys_.rows) < PYREF_BELOW:
        d = ds.log_diff(ref_log, rsio.pyref_log(R.simplification(sys_, rsio.py_flags(on), want_log=True).log))
        assert d is None, f"the oracle's log differs from pyref's: {d}"
    for key, fl, want_log in (("on", on, ref_log), ("off", off, [])):
        for path in ("load", "simplify"):
            outs = run_ranks(h.inp, fl, world, path)
            check_ranks(outs, ref, want_log, f"{case.name} via {path}, log {key}")
            if case.n_rounds is not None:
                assert int(outs[0][2].rounds) == case.n_rounds[rounds]
    after_case(world, largest=case.name == sc.LARGEST["cancel"])
