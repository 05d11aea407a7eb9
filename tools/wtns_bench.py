"""The witness on one result: the check (rs_check_witness on the host, rs_engine_check_witness on the
device) per class set -- the input rows, the output rows, the substitution log, all three -- and the
projection (rs_write_wtns against rs_engine_write_wtns), each beside a floor that only moves the bytes: for
the check the witness's pread into page-locked memory and its H2D, plus the input's H2D for RS_WIT_INPUT;
for the projection the D2H of n8 * n_wires bytes and their pwrite to a fresh pre-allocated file.  Every
figure is warm (one untimed pass, then the best of --reps) in one process.  The engine holds the --O2
result, with the substitution log on, of an rs_synth input (kind 0 at 10 M rows: the metric circuit).
The witness is a random canonical vector with w[0] = 1 (rs_synth makes no witness and none can be derived
cheaply from its rows; what the evaluation costs does not depend on whether rows hold).  Asserts that the
host and device reports and files agree, sweeps RS_WIT_CHUNK over 256 .. 8192 on the device call, and
prints one JSON line (--out: also written there)."""
import argparse
import ctypes as C
import filecmp
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import circom_cvm_amd as M  # noqa: E402
from circom_cvm_amd import abi  # noqa: E402
from json_bench import JsonFloor  # noqa: E402
from reader_bench import Floor  # noqa: E402

SWEEP = (256, 512, 1024, 2048, 4096, 8192)
BN128 = 21888242871839275222246405745257275088548364400416034343698204186575808495617
SETS = (("input", abi.WIT_INPUT), ("output", abi.WIT_OUTPUT), ("log", abi.WIT_LOG),
        ("all", abi.WIT_INPUT | abi.WIT_OUTPUT | abi.WIT_LOG))


def random_witness(n: int, p: int, seed: int):
    """n canonical values (4 limbs each) with w[0] = 1: the top limb is drawn below p's top limb."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] %= np.uint64(p >> 192)
    a[0] = (1, 0, 0, 0)
    arr = np.ascontiguousarray(a.reshape(-1))
    w = abi.RsWitness()
    w.prime_id = abi.RS_PRIME_CUSTOM
    for k in range(4):
        w.prime[k] = (p >> (64 * k)) & abi.U64_MAX
    w.n8, w.n = 32, n
    w.val = arr.ctypes.data_as(C.POINTER(C.c_uint64))
    return abi.Witness(struct=w, keep=arr)


def best_of(reps, f):
    best, keep = None, None
    for i in range(reps + 1):
        t0 = time.perf_counter()
        r = f()
        dt = (time.perf_counter() - t0) * 1000
        if i and (best is None or dt < best):
            best, keep = dt, r
    return best, keep


def triples(rep):
    return [(int(rep.checked[i]), int(rep.failed[i]), int(rep.first_failed[i])) for i in range(6)]


def input_bytes(x) -> int:
    return sum(8 * (int(b.n_rows) + 1) + 36 * int(b.nnz) for b in (x.cons_eq, x.eq, x.linear, x.nl_a, x.nl_b, x.nl_c))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--kind", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--out", default=None, help="also write the JSON there")
    ap.add_argument("--no-host", action="store_true", help="leave the host twins out (the device figures alone)")
    args = ap.parse_args()
    inp = M.Input.synth(args.kind, args.rows, 42)
    pin = M.PinnedInput(inp.c)   # page-locked, as the reader's view is: the input's H2D at link speed
    eng = M.Engine(0)
    eng.load(inp.c)
    eng.run(abi.make_flags("O2", log=True))
    out = eng.fetch()
    n = int(inp.c.max_signal)
    w = random_witness(n, BN128, 7)
    res = {"tool": "wtns_bench", "kind": args.kind, "rows": args.rows, "reps": args.reps, "labels": n,
           "witness": "random canonical vector, w[0] = 1", "witness_bytes": 32 * n, "input_bytes": input_bytes(inp.c),
           "constraints_out": int(out.c.n_constraints), "entries_out": int(out.c.a.nnz + out.c.b.nnz + out.c.c.nnz),
           "log_rows": int(out.c.n_log), "log_entries": int(out.c.log_to.nnz), "wires": int(out.c.n_wires)}
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        wt = os.path.join(tmp, "in.wtns")
        w.write(wt)
        head = os.path.getsize(wt) - 32 * n
        os.environ.pop("RS_WIT_CHUNK", None)
        res["load_wtns_ms"] = round(best_of(args.reps, lambda: eng.load_wtns(wt))[0], 2)
        fd = os.open(wt, os.O_RDONLY)
        fl = Floor(32 * n)
        res["load_floor_ms"] = round(best_of(args.reps, lambda: fl.run(fd, head))[0], 2)
        fl.close()
        os.close(fd)
        in_floor = JsonFloor(res["input_bytes"], 0)
        res["input_h2d_floor_ms"] = round(best_of(args.reps, lambda: in_floor.run_both(os.path.join(tmp, "none")))[0], 2)
        in_floor.close()
        checks = {}
        for name, what in SETS:
            dev_ms, rep = best_of(args.reps, lambda: eng.check_witness(what, pin.c))
            d = {"device_ms": round(dev_ms, 2), "device_in_ms": round(rep.in_ms, 2), "device_kernel_ms": round(rep.kernel_ms, 2),
                 "floor_ms": round(res["load_floor_ms"] + (res["input_h2d_floor_ms"] if what & abi.WIT_INPUT else 0), 2),
                 "checked": [int(x) for x in rep.checked], "failed": [int(x) for x in rep.failed]}
            if not args.no_host:
                runs = []
                for i in range(args.reps + 1):
                    t0 = time.perf_counter()
                    hrep = abi.check_witness(w, what, inp.c, out.c)
                    if i:
                        runs.append((time.perf_counter() - t0) * 1000)
                assert triples(hrep) == triples(rep), f"the host and device reports differ ({name})"
                d.update(host_ms=round(min(runs), 2), host_spread_ms=round(max(runs) - min(runs), 2), reports_agree=True,
                         device_beats_host_by_more_than_3_spreads=bool(min(runs) - dev_ms > 3 * (max(runs) - min(runs))))
            checks[name] = d
        res["check"] = checks
        sweep = {}
        for c in SWEEP:
            os.environ["RS_WIT_CHUNK"] = str(c)
            ms, rep = best_of(args.reps, lambda: eng.check_witness(SETS[3][1], pin.c))
            assert [int(x) for x in rep.failed] == checks["all"]["failed"], f"the report depends on the chunk ({c})"
            sweep[str(c)] = {"device_ms": round(ms, 2), "kernel_ms": round(rep.kernel_ms, 2)}
        os.environ.pop("RS_WIT_CHUNK", None)
        res["chunk_sweep_all"] = sweep
        # ---- the projection
        dev_out, host_out, floor_out = (os.path.join(tmp, x) for x in ("dev.wtns", "host.wtns", "floor.bin"))
        proj = {"out_bytes": 32 * int(out.c.n_wires)}
        proj["device_ms"] = round(best_of(args.reps, lambda: eng.write_wtns(dev_out))[0], 2)
        if not args.no_host:
            runs = []
            for i in range(args.reps + 1):
                t0 = time.perf_counter()
                w.write(host_out, out.c)
                if i:
                    runs.append((time.perf_counter() - t0) * 1000)
            assert filecmp.cmp(host_out, dev_out, shallow=False), "the host and device projections differ"
            proj.update(host_ms=round(min(runs), 2), host_spread_ms=round(max(runs) - min(runs), 2), files_agree=True,
                        device_beats_host_by_more_than_3_spreads=bool(min(runs) - proj["device_ms"] > 3 * (max(runs) - min(runs))))
        pf = JsonFloor(0, proj["out_bytes"])
        proj["floor_ms"] = round(best_of(args.reps, lambda: pf.run_both(floor_out))[0], 2)
        pf.close()
        res["projection"] = proj
    out.free()
    pin.free()
    inp.free()
    eng.close()
    text = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
