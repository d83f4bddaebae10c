"""bench.py's command line, as far as it can be checked without a GPU."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                         check=True).stdout
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in out


def test_dump_outputs_is_exact_float64(tmp_path):
    import bench
    merges = np.array([[97, 98, 256, 0xFFFFFFFF], [256, 99, 257, 3]], dtype=np.uint32)
    bench.dump_outputs(str(tmp_path / "d"), merges)
    got = np.load(tmp_path / "d" / "merges.npy")
    assert got.dtype == np.float64 and got.shape == (2, 4)
    assert np.array_equal(got.astype(np.uint32), merges)
