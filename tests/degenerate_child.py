"""One rank of tests/test_gpu_degenerate.py::test_one_cluster_over_the_host_transport: an engine on device 0
joins the group `tag` as `rank` (rs_engine_join_host), runs one rank case of tests/degenerate.py host ->
host twice and load / run / fetch once at --O2 and --O1, and checks every view against the oracle.
usage: degenerate_child.py <world> <rank> <tag> <case>"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import degenerate as D  # noqa: E402
import rsio  # noqa: E402
import circom_cvm_amd as M  # noqa: E402

world, rank, tag, case = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
e = M.Engine(0)
e.join_host(world, rank, tag)
h = D.holder(D.rank_cases(D.BN, world)[case][0], "bn128")
for key in ("O2", "O1"):
    fl = D.fl_of(key)
    ref, _ = rsio.oracle_arrays(h.inp, fl)
    for i in range(2):
        diff = rsio.diff_output_arrays(rsio.output_arrays(e.simplify(h.inp, fl)), ref)
        if diff is not None:
            print(f"rank {rank} {key} call {i}: differs from the oracle: {diff}", flush=True)
            sys.exit(3)
    assert e.stats().world == world
    e.load(h.inp)
    e.run(fl)
    out = e.fetch()
    diff = rsio.diff_output_arrays(rsio.output_arrays(out.c), ref)
    if diff is not None:
        print(f"rank {rank} {key}: load/run/fetch differs from the oracle: {diff}", flush=True)
        sys.exit(4)
e.close()
print(f"rank {rank} ok", flush=True)
