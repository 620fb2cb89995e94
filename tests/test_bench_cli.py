"""CPU checks of bench.py's command line and its --dump-outputs writer
(no GPU: the parser runs before any device work; the writer takes plain
Partial structs)."""
import os
import subprocess
import sys

import numpy as np

import banyandb_amd as ba
import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _partials():
    vals = [(2 ** 60 + 12345, 7, -5, 2 ** 40 + 1, 1.5),
            (-(2 ** 61) - 3, 0, ba.INT64_MAX, ba.INT64_MIN, -0.25)]
    parts = []
    for s, c, mn, mx, sf in vals:
        p = ba.Partial()
        p.sum_i, p.count, p.min_i, p.max_i, p.sum_f = s, c, mn, mx, sf
        parts.append(p)
    return vals, parts


def test_help_lists_full_and_dump_outputs():
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"),
                        "--help"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in p.stdout


def test_steps_below_one_is_an_error():
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"),
                        "--steps", "0"], capture_output=True, text=True)
    assert p.returncode == 2
    assert "--steps" in p.stderr


def test_dump_partials_int64_fields_are_exact(tmp_path):
    vals, parts = _partials()
    d = str(tmp_path / "out")
    bench.dump_partials(d, parts, ["sum", "count", "min", "max"], False)
    assert sorted(os.listdir(d)) == sorted(
        f"{f}{s}.npy" for f in ("sum_i", "count", "min_i", "max_i")
        for s in ("", "_lo32"))
    for col, f in ((0, "sum_i"), (1, "count"), (2, "min_i"), (3, "max_i")):
        hi = np.load(os.path.join(d, f + ".npy"))
        lo = np.load(os.path.join(d, f + "_lo32.npy"))
        assert hi.dtype == np.float64 and lo.dtype == np.float64
        assert hi.shape == lo.shape == (2,)
        for g in range(2):
            want = vals[g][col]
            assert lo[g] == want & 0xFFFFFFFF
            # the float64 is the value rounded: within one ulp (<= 2^10
            # for |v| < 2^63), so with the exact low 32 bits it pins the
            # int64
            assert abs(int(hi[g]) - want) <= 1024


def test_dump_partials_writes_only_configured_fields(tmp_path):
    vals, parts = _partials()
    d = str(tmp_path / "out")
    bench.dump_partials(d, parts, ["sum", "count"], True, prefix="f64_")
    assert sorted(os.listdir(d)) == ["f64_count.npy", "f64_count_lo32.npy",
                                     "f64_sum_f.npy"]
    sf = np.load(os.path.join(d, "f64_sum_f.npy"))
    assert sf.dtype == np.float64
    assert sf.tolist() == [v[4] for v in vals]
