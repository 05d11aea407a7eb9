"""The .sym writers on one file: rs_write_sym (host), rs_engine_write_sym (device) and a floor -- pread of
the input into page-locked memory, its H2D, the D2H of as many bytes as the output has and their pwrite,
and nothing else -- each warm (one untimed pass, then the best of --reps), in one process.  The engine
holds the --O2 result of an rs_synth input (kind 0 at 10 M rows: the metric circuit); the --O0 .sym has
one `i,i,i % 3,main.s[i]` line per signal and is written once to a temporary file.  Asserts that the two
writers' files are identical, then prints one JSON line: the three times, the host's spread over its
runs, the device call's split from rs_stats and how far it sits above the floor."""
import argparse
import ctypes as C
import filecmp
import json
import os
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import circom_cvm_amd as M  # noqa: E402
from circom_cvm_amd import abi  # noqa: E402
from reader_bench import Floor  # noqa: E402


class SymFloor(Floor):
    """Floor's pread + H2D of the input, then the D2H of `out_size` bytes of the same device array and
    their pwrite to a fresh file (its blocks allocated up front, like the writers'), the next chunk's D2H
    in flight during a pwrite."""

    def __init__(self, size: int, out_size: int):
        super().__init__(max(size, out_size))
        self.in_size, self.out_size = size, out_size

    def run_both(self, fd: int, path: str) -> float:
        t0 = time.perf_counter()
        self.size = self.in_size
        self.run(fd, 0)
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


def write_o0_sym(path: str, n_labels: int):
    with open(path, "w") as f:
        for lo in range(1, n_labels, 1 << 20):
            f.write("".join(f"{i},{i},{i % 3},main.s[{i}]\n" for i in range(lo, min(lo + (1 << 20), n_labels))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--kind", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    inp = M.Input.synth(args.kind, args.rows, 42)
    n_labels = int(inp.c.max_signal)
    eng = M.Engine(0)
    eng.load(inp.c)
    eng.run(abi.make_flags("O2"))
    out = eng.fetch()
    inp.free()
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        src, host_out, dev_out, floor_out = (os.path.join(tmp, n) for n in ("in_O0.sym", "host.sym", "dev.sym", "floor.sym"))
        write_o0_sym(src, n_labels)
        in_size = os.path.getsize(src)

        host = []
        for i in range(args.reps + 1):
            t0 = time.perf_counter()
            abi.check(abi.lib().rs_write_sym(src.encode(), host_out.encode(), out.ptr))
            if i:
                host.append((time.perf_counter() - t0) * 1000)
        out_size = os.path.getsize(host_out)

        dev_ms, stats = None, None
        for i in range(args.reps + 1):
            t0 = time.perf_counter()
            eng.write_sym(src, dev_out)
            dt = (time.perf_counter() - t0) * 1000
            if i and (dev_ms is None or dt < dev_ms):
                dev_ms, stats = dt, eng.stats()
        assert filecmp.cmp(host_out, dev_out, shallow=False), "the host and device writers' files differ"
        out.free()
        eng.close()

        floor = SymFloor(in_size, out_size)
        fd = os.open(src, os.O_RDONLY)
        floor_ms = None
        for i in range(args.reps + 1):
            dt = floor.run_both(fd, floor_out)
            if i:
                floor_ms = dt if floor_ms is None else min(floor_ms, dt)
        os.close(fd)
        floor.close()
    host_ms, spread = min(host), max(host) - min(host)
    print(json.dumps({
        "tool": "sym_bench", "kind": args.kind, "rows": args.rows, "signals": n_labels, "in_bytes": in_size,
        "out_bytes": out_size, "reps": args.reps, "writers_agree": True,
        "host_writer_ms": round(host_ms, 2), "host_runs_ms": [round(x, 2) for x in host], "host_spread_ms": round(spread, 2),
        "device_writer_ms": round(dev_ms, 2), "floor_ms": round(floor_ms, 2),
        "device_beats_host_by_more_than_spread": bool(host_ms - dev_ms > spread),
        "device_over_floor": round(dev_ms / floor_ms, 3), "host_over_device": round(host_ms / dev_ms, 2),
        "device_in_ms": round(stats.sym_in_ms, 2), "device_kernels_ms": round(stats.sym_kernel_ms, 2),
        "device_out_ms": round(stats.sym_out_ms, 2)}))


if __name__ == "__main__":
    main()
