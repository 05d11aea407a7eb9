"""bench.py --dump-outputs and the plain / --full split.  The dump is float64 and exact (64-bit words as
their 32-bit halves), sampled with a fixed seed above DUMP_ENTRIES, and on the GPU it is the result of
the timed host -> host path: equal, file for file, to the dump of the CPU oracle's output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import circom_cvm_amd as M
import rsio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["l2w"] + [f"{q}_{part}" for q in "abc" for part in ("ptr", "col", "val")]


def _oracle(rows):
    inp = M.Input.synth(0, rows, 42, "bn128")
    try:
        return rsio.oracle_arrays(inp.c, rsio.flags("O2"), threads=2)[0]
    finally:
        inp.free()


@pytest.fixture(scope="module")
def oracle_out():
    return _oracle(3000)


def _originals(arr):
    d = {"l2w": arr["l2w"]}
    for q in "abc":
        d[q + "_ptr"], d[q + "_col"], d[q + "_val"] = arr[q][0], arr[q][1], arr[q][2].reshape(-1, 4)
    return d


def _back(dumped, like):
    """The unsigned integers a dumped array stands for."""
    if like.dtype.itemsize < 8:
        return dumped.astype(like.dtype)
    u = dumped.astype(np.uint64)
    r = u[:, 0::2] | (u[:, 1::2] << np.uint64(32))
    return r.reshape(like.shape)


def test_dump_is_exact_float64(oracle_out, tmp_path):
    bench.dump_outputs(str(tmp_path), oracle_out)
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in NAMES + ["scalars", "summary"])
    sc = np.load(tmp_path / "scalars.npy")
    assert sc.dtype == np.float64
    assert sc.tolist() == [oracle_out[k] for k in ("n_constraints", "n_wires", "npiw", "n_labels")]
    summary = np.load(tmp_path / "summary.npy")
    assert summary.dtype == np.float64 and summary.shape == (len(NAMES), 3)
    total = sc.nbytes + summary.nbytes
    for i, (name, x) in enumerate(_originals(oracle_out).items()):
        assert name == NAMES[i]
        d = np.load(tmp_path / (name + ".npy"))
        total += d.nbytes
        assert d.dtype == np.float64 and d.shape[0] == x.shape[0] <= bench.DUMP_ENTRIES
        assert np.array_equal(_back(d, x), x), name
        s = int(np.sum(np.ascontiguousarray(x).view("<u4"), dtype=np.uint64))
        assert summary[i].tolist() == [x.shape[0], s & 0xFFFFFFFF, s >> 32]
    assert oracle_out["n_constraints"] > 0 and total < 64e6


def test_dump_sample_is_fixed(oracle_out, tmp_path, monkeypatch):
    """Above DUMP_ENTRIES an array is written as a sample: the same rows on every call, in the array's
    order, with the summary still the whole array's.  The worst-case size stays under the 64 MB cap."""
    per_entry = 8 * (2 + 3 * (2 + 1 + 8))  # l2w (at most 2 words), ptr (2) + col + val (8) per block, as float64
    assert bench.DUMP_ENTRIES * per_entry + 8 * (4 + 3 * len(NAMES)) < 64e6
    monkeypatch.setattr(bench, "DUMP_ENTRIES", 64)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), oracle_out)
    bench.dump_outputs(str(b), oracle_out)
    summary = np.load(a / "summary.npy")
    for i, (name, x) in enumerate(_originals(oracle_out).items()):
        d = np.load(a / (name + ".npy"))
        assert np.array_equal(d, np.load(b / (name + ".npy"))), name
        assert x.shape[0] > 64 and d.shape[0] == 64 and summary[i][0] == x.shape[0]
        # a subsequence of the array: every sampled row is found at increasing positions
        got = _back(d, x[:64]).reshape(64, -1)
        rows = np.ascontiguousarray(x).reshape(x.shape[0], -1)
        pos = 0
        for r in got:
            hit = np.flatnonzero((rows[pos:] == r).all(axis=1))
            assert hit.size, name
            pos += int(hit[0]) + 1


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_their_result(tmp_path):
    """A plain run at a small size: --steps is the number of timed steps, the line has ms_per_step and
    none of the extras' results, and the dumped arrays are the oracle's for the same arguments."""
    rows = 30000
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--rows", str(rows), "--dump-outputs", str(tmp_path / "gpu")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "constraints/s" and line["higher_is_better"] is True
    # value = constraints / step time; ms_per_step is printed rounded to 3 decimals (half a microsecond off at most)
    rel = 0.0006 / line["ms_per_step"] + 1e-6
    assert abs(line["value"] - line["config"]["constraints"] / (line["ms_per_step"] / 1000.0)) <= rel * line["value"]
    assert line["bit_exact"] is None and line["cpu_baseline"] is None and line["hbm_resident"] is None
    assert not {"link", "write_r1cs", "flatten_dag", "templated", "linear1M", "o1", "weak_shards"} & set(line)
    bench.dump_outputs(str(tmp_path / "cpu"), _oracle(rows))
    for name in NAMES + ["scalars", "summary"]:
        g, c = np.load(tmp_path / "gpu" / (name + ".npy")), np.load(tmp_path / "cpu" / (name + ".npy"))
        assert g.dtype == np.float64 and g.shape == c.shape and np.array_equal(g, c), name
