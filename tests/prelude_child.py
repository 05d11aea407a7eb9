"""The replay path of chosen cases, read from the library's own RS_PROF lines, in a process of its own
(tests/test_gpu_prelude.py starts it with RS_PROF set, which the library reads once when it is loaded).
gpu_clusters prints `[rs-prof] host replay: N clusters (M order-free), ...` once per clustering that
holds a cluster of more than kClMid and at most kClLds rows, and nothing for any other.  This process
writes `[child] case NAME` to stderr before each case and prints one JSON line per case: the comparison
with the oracle and rs_stats.cluster_host_ms.

    python tests/prelude_child.py NAME [NAME ...]     a case of prelude_cases.py or dispatch_shapes.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, d)

import dispatch_shapes as ds  # noqa: E402
import prelude_cases as pc  # noqa: E402
import rsio  # noqa: E402
import circom_cvm_amd as M  # noqa: E402

R = rsio.R


def main(names) -> int:
    by = {c.name: c for c in ds.CASES + pc.CASES}
    eng = M.Engine(0)
    try:
        for nm in names:
            sys_, _ = by[nm].build(R.PRIMES["bn128"])
            h = rsio.InputHolder(sys_, "bn128")
            fl = rsio.flags("O2")
            ref, _ = rsio.oracle_arrays(h.inp, fl, threads=8)
            sys.stderr.write(f"[child] case {nm}\n")
            sys.stderr.flush()
            eng.load(h.inp)
            eng.run(fl)
            out = eng.fetch()
            print(json.dumps({"case": nm, "diff": rsio.diff_output_arrays(rsio.output_arrays(out.c), ref),
                              "cluster_host_ms": float(eng.stats().cluster_host_ms)}))
    finally:
        eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
