"""The JSON writers on one result: for <prefix>_constraints.json and <prefix>_substitutions.json each, the
host writer (rs_write_constraints_json / rs_write_substitution_json over the fetched output), the device
writer (rs_engine_write_constraints_json / rs_engine_write_substitution_json) and a floor -- the D2H of as
many bytes as the file has, in ImageOut's 32 MB chunks, and their pwrite to a fresh pre-allocated file; for
the log also the H2D of the log's arrays through page-locked staging buffers -- each warm (one untimed
pass, then the best of --reps), in one process.  The engine holds the --O2 result, with the substitution
log on, of an rs_synth input (kind 0 at 10 M rows: the metric circuit).  Asserts that the two writers'
files are identical, then prints one JSON line: the times, the host's spread over its runs, the device
call's split from rs_json_stats, how far it sits above the floor, and (--sweep) the device writer at
RS_JSON_CHUNK = 4 .. 64 KiB."""
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
from reader_bench import Floor  # noqa: E402

SWEEP = (4096, 8192, 16384, 32768, 65536)


class JsonFloor(Floor):
    """The H2D of `in_size` bytes of host memory through Floor's page-locked buffers (0: none), then the
    D2H of `out_size` bytes of the same device array and their pwrite to a fresh file (its blocks
    allocated up front, like the writers'), the next chunk's D2H in flight during a pwrite."""

    def __init__(self, in_size: int, out_size: int):
        super().__init__(max(in_size, out_size))
        self.in_size, self.out_size = in_size, out_size
        self.src = memoryview(np.zeros(max(in_size, 1), np.uint8))

    def run_both(self, path: str) -> float:
        t0 = time.perf_counter()
        for i, o in enumerate(range(0, self.in_size, self.chunk)):
            b = i % len(self.host)
            n = min(self.chunk, self.in_size - o)
            if i >= len(self.host):
                self._ok(self.hip.hipEventSynchronize(self.events[b]))
            self.views[b][:n] = self.src[o:o + n]
            self._ok(self.hip.hipMemcpyAsync(C.c_void_p(self.dev.value + o), self.host[b], C.c_size_t(n), 1, self.stream))
            self._ok(self.hip.hipEventRecord(self.events[b], self.stream))
        self._ok(self.hip.hipStreamSynchronize(self.stream))
        out = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        os.posix_fallocate(out, 0, max(self.out_size, 1))
        offs = list(range(0, self.out_size, self.chunk))

        def d2h(i):
            n = min(self.chunk, self.out_size - offs[i])
            b = i % len(self.host)
            self._ok(self.hip.hipMemcpyAsync(self.host[b], C.c_void_p(self.dev.value + offs[i]), C.c_size_t(n), 2, self.stream))
            self._ok(self.hip.hipEventRecord(self.events[b], self.stream))

        if offs:
            d2h(0)
        for i, o in enumerate(offs):
            if i + 1 < len(offs):
                d2h(i + 1)
            b = i % len(self.host)
            self._ok(self.hip.hipEventSynchronize(self.events[b]))
            n = min(self.chunk, self.out_size - o)
            done = 0
            while done < n:
                done += os.pwrite(out, self.views[b][done:n], o + done)
        os.ftruncate(out, self.out_size)
        os.close(out)
        return (time.perf_counter() - t0) * 1000


def bench(kind, eng, out, tmp, reps, sweep, device_only=False):
    host_f = abi.lib().rs_write_constraints_json if kind == "constraints" else abi.lib().rs_write_substitution_json
    dev_f = eng.write_constraints_json if kind == "constraints" else eng.write_substitution_json
    host_out, dev_out, floor_out = (os.path.join(tmp, f"{n}_{kind}.json") for n in ("host", "dev", "floor"))
    host = []
    for i in range(0 if device_only else reps + 1):
        t0 = time.perf_counter()
        abi.check(host_f(host_out.encode(), out.ptr))
        if i:
            host.append((time.perf_counter() - t0) * 1000)

    def device():
        best, stats = None, None
        for i in range(reps + 1):
            t0 = time.perf_counter()
            dev_f(dev_out)
            dt = (time.perf_counter() - t0) * 1000
            if i and (best is None or dt < best):
                best, stats = dt, eng.json_stats()
        return best, stats

    os.environ.pop("RS_JSON_CHUNK", None)
    dev_ms, stats = device()
    out_size = os.path.getsize(dev_out)
    if device_only:  # (RS_PROF runs: the device call's split alone)
        os.remove(dev_out)
        return {"out_bytes": out_size, "device_writer_ms": round(dev_ms, 2), "device_in_ms": round(stats.in_ms, 2),
                "device_kernels_ms": round(stats.kernel_ms, 2), "device_out_ms": round(stats.out_ms, 2)}
    assert out_size == os.path.getsize(host_out)
    assert filecmp.cmp(host_out, dev_out, shallow=False), f"the host and device writers' {kind} files differ"
    chunks = {}
    for c in sweep:
        os.environ["RS_JSON_CHUNK"] = str(c)
        ms, st = device()
        chunks[str(c)] = {"device_writer_ms": round(ms, 2), "kernels_ms": round(st.kernel_ms, 2)}
    os.environ.pop("RS_JSON_CHUNK", None)
    os.remove(host_out)
    os.remove(dev_out)

    o = out.c
    in_size = 0 if kind == "constraints" else 4 * int(o.n_log) + 8 * (int(o.n_log) + 1) + 36 * int(o.log_to.nnz)
    floor = JsonFloor(in_size, out_size)
    floor_ms = None
    for i in range(reps + 1):
        dt = floor.run_both(floor_out)
        if i:
            floor_ms = dt if floor_ms is None else min(floor_ms, dt)
    floor.close()
    os.remove(floor_out)
    host_ms, spread = min(host), max(host) - min(host)
    res = {"out_bytes": out_size, "in_bytes": in_size, "writers_agree": True,
           "host_writer_ms": round(host_ms, 2), "host_runs_ms": [round(x, 2) for x in host], "host_spread_ms": round(spread, 2),
           "device_writer_ms": round(dev_ms, 2), "floor_ms": round(floor_ms, 2),
           "device_beats_host_by_more_than_3_spreads": bool(host_ms - dev_ms > 3 * spread),
           "device_over_floor": round(dev_ms / floor_ms, 3), "host_over_device": round(host_ms / dev_ms, 2),
           "device_in_ms": round(stats.in_ms, 2), "device_kernels_ms": round(stats.kernel_ms, 2),
           "device_out_ms": round(stats.out_ms, 2), "kernels_share": round(stats.kernel_ms / stats.write_ms, 3)}
    if chunks:
        res["chunk_sweep"] = chunks
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--kind", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--sweep", action="store_true", help="also the device writer at RS_JSON_CHUNK = 4 .. 64 KiB")
    ap.add_argument("--device-only", action="store_true", help="only the device writers (e.g. under RS_PROF)")
    args = ap.parse_args()
    inp = M.Input.synth(args.kind, args.rows, 42)
    eng = M.Engine(0)
    eng.load(inp.c)
    eng.run(abi.make_flags("O2", log=True))
    out = eng.fetch()
    inp.free()
    res = {"tool": "json_bench", "kind": args.kind, "rows": args.rows, "reps": args.reps,
           "constraints_out": int(out.c.n_constraints), "entries": int(out.c.a.nnz + out.c.b.nnz + out.c.c.nnz),
           "log_rows": int(out.c.n_log), "log_entries": int(out.c.log_to.nnz)}
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        for kind in ("constraints", "substitutions"):
            res[kind] = bench(kind, eng, out, tmp, args.reps, SWEEP if args.sweep else (), args.device_only)
    out.free()
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
