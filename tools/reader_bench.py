"""The --O0 readers on one file: rs_read_r1cs_o0 (host), rs_engine_read_r1cs_o0 (device) and a floor
-- pread of the constraint section into page-locked memory plus its H2D, and nothing else -- each warm
(one untimed pass, then the best of --reps).  The file is the identity result of an rs_synth input
written with rs_write_r1cs: the non-linear rows, then cons_eq, eq and linear as C-only rows, with
label_to_wire the identity.  Asserts that the two readers agree field for field and array for array,
then prints one JSON line (device_over_floor, the kernels' share from rs_stats, ...).  RS_PROF=1 adds
the time of every kernel step on stderr."""
import argparse
import ctypes as C
import json
import os
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import circom_cvm_amd as M  # noqa: E402
from circom_cvm_amd import abi  # noqa: E402
import readerio  # noqa: E402


def identity_output(x: abi.RsInput):
    """The rs_output that keeps every row of `x` and every signal: (struct, the arrays it points at)."""
    def arr(b):
        n, nnz = int(b.n_rows), int(b.nnz)
        return (np.ctypeslib.as_array(b.ptr, shape=(n + 1,)), np.ctypeslib.as_array(b.col, shape=(max(nnz, 1),))[:nnz],
                np.ctypeslib.as_array(b.val, shape=(max(nnz, 1) * 4,))[:4 * nnz])
    lin = [arr(b) for b in (x.cons_eq, x.eq, x.linear)]
    n_lin = sum(p.shape[0] - 1 for p, _, _ in lin)
    keep = []
    out = abi.RsOutput()
    for q, b in enumerate((x.nl_a, x.nl_b, x.nl_c)):
        ptr, col, val = arr(b)
        if q < 2:  # the linear rows' A and B are empty
            ptr = np.concatenate([ptr, np.full(n_lin, ptr[-1], np.uint64)])
        else:
            ptrs, cols, vals, base = [ptr], [col], [val], int(ptr[-1])
            for p, c, v in lin:
                ptrs.append(p[1:] + np.uint64(base))
                cols.append(c)
                vals.append(v)
                base += int(p[-1])
            ptr, col, val = np.concatenate(ptrs), np.concatenate(cols), np.concatenate(vals)
        ptr = np.ascontiguousarray(ptr, np.uint64)
        col = np.ascontiguousarray(col if col.size else np.zeros(1, np.uint32), np.uint32)
        val = np.ascontiguousarray(val if val.size else np.zeros(4, np.uint64), np.uint64)
        keep += [ptr, col, val]
        lc = abi.RsLc(ptr.shape[0] - 1, int(ptr[-1]), ptr.ctypes.data_as(C.POINTER(C.c_uint64)),
                      col.ctypes.data_as(C.POINTER(C.c_uint32)), val.ctypes.data_as(C.POINTER(C.c_uint64)))
        setattr(out, "abc"[q], lc)
    n = int(x.max_signal)
    l2w = np.arange(n, dtype=np.int32)
    keep.append(l2w)
    out.n_constraints = int(x.nl_a.n_rows) + n_lin
    out.n_labels = out.n_wires = n
    out.label_to_wire = l2w.ctypes.data_as(C.POINTER(C.c_int32))
    out.no_private_inputs_witness = int(x.n_priv_in)
    return out, keep


class Floor:
    """pread of a byte range into page-locked staging buffers and their H2D, double-buffered."""

    def __init__(self, size: int, chunk: int = 32 << 20, bufs: int = 4):
        self.hip = C.CDLL("libamdhip64.so.7")
        self.chunk, self.size = min(chunk, max(size, 1)), size
        self.dev, self.stream = C.c_void_p(), C.c_void_p()
        self._ok(self.hip.hipMalloc(C.byref(self.dev), C.c_size_t(max(size, 1))))
        self._ok(self.hip.hipStreamCreateWithFlags(C.byref(self.stream), 1))  # non-blocking
        self.host, self.views, self.events = [], [], []
        for _ in range(bufs):
            p, e = C.c_void_p(), C.c_void_p()
            self._ok(self.hip.hipHostMalloc(C.byref(p), C.c_size_t(self.chunk), 0))
            self._ok(self.hip.hipEventCreateWithFlags(C.byref(e), 2))  # no timing
            self.host.append(p)
            self.views.append(memoryview((C.c_uint8 * self.chunk).from_address(p.value)).cast("B"))
            self.events.append(e)

    @staticmethod
    def _ok(rc):
        if rc:
            raise OSError(f"HIP error {rc}")

    def run(self, fd: int, off: int) -> float:
        t0 = time.perf_counter()
        for i, o in enumerate(range(0, self.size, self.chunk)):
            b = i % len(self.host)
            n = min(self.chunk, self.size - o)
            if i >= len(self.host):
                self._ok(self.hip.hipEventSynchronize(self.events[b]))
            got = 0
            while got < n:
                k = os.preadv(fd, [self.views[b][got:n]], off + o + got)
                if k <= 0:
                    raise OSError("short read")
                got += k
            self._ok(self.hip.hipMemcpyAsync(C.c_void_p(self.dev.value + o), self.host[b], C.c_size_t(n), 1, self.stream))
            self._ok(self.hip.hipEventRecord(self.events[b], self.stream))
        self._ok(self.hip.hipStreamSynchronize(self.stream))
        return (time.perf_counter() - t0) * 1000

    def close(self):
        for p in self.host:
            self.hip.hipHostFree(p)
        for e in self.events:
            self.hip.hipEventDestroy(e)
        self.hip.hipStreamDestroy(self.stream)
        self.hip.hipFree(self.dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--kind", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    inp = M.Input.synth(args.kind, args.rows, 42)
    out, keep = identity_output(inp.c)
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        path = os.path.join(tmp, "in_O0.r1cs")
        abi.check(abi.lib().rs_write_r1cs(path.encode(), C.byref(inp.c), C.byref(out)))
        n_cons = int(out.n_constraints)
        del out, keep
        inp.free()
        size = os.path.getsize(path)
        with open(path, "rb") as f:
            head = f.read(24)
        assert struct.unpack_from("<I", head, 12)[0] == 2  # the writer puts the constraint section first
        sec_off, sec_size = 24, struct.unpack_from("<Q", head, 16)[0]

        host_ms, want = None, None
        for i in range(args.reps + 1):
            t0 = time.perf_counter()
            h = M.Input.read_r1cs(path)
            dt = (time.perf_counter() - t0) * 1000
            if i:
                host_ms = dt if host_ms is None else min(host_ms, dt)
            if i == args.reps:
                want = readerio.input_arrays(h.c)
            h.free()

        eng = M.Engine(0)
        dev_ms, stats = None, None
        for i in range(args.reps + 1):
            t0 = time.perf_counter()
            view = eng.read_r1cs(path)
            dt = (time.perf_counter() - t0) * 1000
            if i and (dev_ms is None or dt < dev_ms):
                dev_ms, stats = dt, eng.stats()
        diff = readerio.diff_inputs(want, readerio.input_arrays(view))
        assert diff is None, diff
        eng.close()

        floor = Floor(sec_size - sec_size % 4)
        fd = os.open(path, os.O_RDONLY)
        floor_ms = None
        for i in range(args.reps + 1):
            dt = floor.run(fd, sec_off)
            if i:
                floor_ms = dt if floor_ms is None else min(floor_ms, dt)
        os.close(fd)
        floor.close()
    print(json.dumps({
        "tool": "reader_bench", "kind": args.kind, "rows": args.rows, "constraints": n_cons, "file_bytes": size,
        "section_bytes": sec_size, "reps": args.reps, "readers_agree": True,
        "host_reader_ms": round(host_ms, 2), "device_reader_ms": round(dev_ms, 2), "floor_ms": round(floor_ms, 2),
        "device_over_floor": round(dev_ms / floor_ms, 3), "host_over_device": round(host_ms / dev_ms, 2),
        "device_upload_ms": round(stats.read_upload_ms, 2), "device_kernels_ms": round(stats.read_kernel_ms, 2),
        "device_d2h_ms": round(stats.read_d2h_ms, 2),
        "kernels_share": round(stats.read_kernel_ms / stats.read_ms, 3)}))


if __name__ == "__main__":
    main()
