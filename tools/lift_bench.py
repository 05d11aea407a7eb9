"""The lift on one result: rs_lift_witness on the host against rs_engine_lift_witness on the device, beside
the floor that only moves the log's bytes (their H2D through page-locked staging buffers, as wtns_bench's
log floor does); and the lifted witness's file, rs_engine_write_wtns_resident against the host's
rs_write_wtns(path, w, NULL), beside the floor of its D2H plus pwrite.  Every figure is warm (one untimed
pass, then the best of --reps) in one process.  The engine holds the --O2 result, with the substitution
log on, of an rs_synth input (kind 0 at 10 M rows: the metric circuit).  The wire vector is a random
canonical vector with v[0] = 1 (rs_synth makes no witness; what the lift costs does not depend on whether
rows hold).  Asserts that the host and device values, reports and files agree, sweeps RS_WIT_CHUNK over
256 .. 8192 on the device call, and prints one JSON line (--out: also written there)."""
import argparse
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
from wtns_bench import BN128, SWEEP, best_of, random_witness  # noqa: E402


def values(w) -> np.ndarray:
    c = w.c
    return np.ctypeslib.as_array(c.val, shape=(4 * int(c.n),)).copy()


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
    eng = M.Engine(0)
    eng.load(inp.c)
    eng.run(abi.make_flags("O2", log=True))
    out = eng.fetch()
    n_wires, n_labels = int(out.c.n_wires), int(out.c.n_labels)
    v = random_witness(n_wires, BN128, 7)
    log_bytes = 4 * int(out.c.n_log) + 8 * (int(out.c.n_log) + 1) + 36 * int(out.c.log_to.nnz)
    res = {"tool": "lift_bench", "kind": args.kind, "rows": args.rows, "reps": args.reps, "labels": n_labels, "wires": n_wires,
           "witness": "random canonical vector, v[0] = 1", "log_rows": int(out.c.n_log), "log_entries": int(out.c.log_to.nnz),
           "log_bytes": log_bytes}

    def device_lift():
        eng.load_witness(v)      # (not timed by the report: the lift's own times are in_ms / kernel_ms / total_ms)
        return eng.lift_witness()

    os.environ.pop("RS_WIT_CHUNK", None)
    device_lift()
    reps = [device_lift() for _ in range(args.reps)]
    rep = min(reps, key=lambda r: r.total_ms)
    dev = {"total_ms": round(rep.total_ms, 2), "in_ms": round(rep.in_ms, 2), "kernel_ms": round(rep.kernel_ms, 2),
           "levels": int(rep.levels), "lifted": int(rep.lifted), "free_labels": int(rep.free_labels), "shadowed": int(rep.shadowed),
           "entries": int(rep.entries)}
    res["device"] = dev
    lifted = eng.fetch_witness()
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        fl = JsonFloor(log_bytes, 0)
        res["log_h2d_floor_ms"] = round(best_of(args.reps, lambda: fl.run_both(os.path.join(tmp, "none")))[0], 2)
        fl.close()
        if not args.no_host:
            runs, hw, hrep = [], None, None
            for i in range(args.reps + 1):
                t0 = time.perf_counter()
                hw, hrep = abi.lift_witness(v, out.c)
                if i:
                    runs.append((time.perf_counter() - t0) * 1000)
            assert hrep.counts() == rep.counts(), "the host and device reports differ"
            assert np.array_equal(values(hw), values(lifted)), "the host and device values differ"
            res["host"] = {"ms": round(min(runs), 2), "spread_ms": round(max(runs) - min(runs), 2), "values_agree": True,
                           "device_beats_host_by_more_than_3_spreads": bool(min(runs) - rep.total_ms > 3 * (max(runs) - min(runs)))}
        sweep = {}
        for c in SWEEP:
            os.environ["RS_WIT_CHUNK"] = str(c)
            device_lift()
            r = min((device_lift() for _ in range(args.reps)), key=lambda x: x.total_ms)
            assert r.counts() == rep.counts(), f"the report depends on the chunk ({c})"
            sweep[str(c)] = {"total_ms": round(r.total_ms, 2), "kernel_ms": round(r.kernel_ms, 2)}
        os.environ.pop("RS_WIT_CHUNK", None)
        res["chunk_sweep"] = sweep
        # ---- the lifted witness's file (the resident witness is the lifted one)
        dev_out, host_out, floor_out = (os.path.join(tmp, x) for x in ("dev.wtns", "host.wtns", "floor.bin"))
        wr = {"out_bytes": 32 * n_labels}
        wr["device_ms"] = round(best_of(args.reps, lambda: eng.write_wtns_resident(dev_out))[0], 2)
        if not args.no_host:
            runs = []
            for i in range(args.reps + 1):
                t0 = time.perf_counter()
                lifted.write(host_out)
                if i:
                    runs.append((time.perf_counter() - t0) * 1000)
            assert filecmp.cmp(host_out, dev_out, shallow=False), "the host and device files differ"
            wr.update(host_ms=round(min(runs), 2), host_spread_ms=round(max(runs) - min(runs), 2), files_agree=True,
                      device_beats_host_by_more_than_3_spreads=bool(min(runs) - wr["device_ms"] > 3 * (max(runs) - min(runs))))
        pf = JsonFloor(0, wr["out_bytes"])
        wr["floor_ms"] = round(best_of(args.reps, lambda: pf.run_both(floor_out))[0], 2)
        pf.close()
        res["write_resident"] = wr
    out.free()
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
