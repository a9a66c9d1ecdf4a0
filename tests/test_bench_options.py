"""bench.py's plain / --full split and --dump-outputs: a plain run keeps only the dense steps
(every side leg switched off, null in its line), --full leaves the legs to their own --no-...
switches, and --dump-outputs writes the sampled volume of the last timed step as float32 .npy
files of at most 64 MB in all, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

BENCH = os.path.join(REPO, "bench.py")
LEGS = ("no_hash", "no_cpu", "no_ingest", "no_dropin", "no_mesh", "no_lounge")


def _parse(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    import bench
    return bench.parse()


def test_plain_run_switches_every_side_leg_off(monkeypatch):
    a = _parse(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert not a.full and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    assert all(getattr(a, leg) for leg in LEGS)


def test_full_run_keeps_the_legs_and_their_switches(monkeypatch):
    a = _parse(monkeypatch, ["--full"])
    assert a.full and not any(getattr(a, leg) for leg in LEGS)
    a = _parse(monkeypatch, ["--full", "--no-cpu", "--dump-outputs", "d"])
    assert a.no_cpu and not a.no_hash and a.dump_outputs == "d"


def test_dump_sample_fits_the_size_limit():
    import bench
    # three float32 arrays and the float64 indices
    assert bench.DUMP_SAMPLE * (3 * 4 + 8) <= 64_000_000


@pytest.mark.gpu
def test_plain_run_dumps_the_sampled_volume(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", "96",
                        "--preheat-ms", "0", "--dump-outputs", str(out)], capture_output=True, text=True,
                       timeout=170, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    line = lines[0]
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert line["ms_per_step"] > 0 and line["value"] > 0 and line["dtype"] == "f64"
    assert line["value"] == pytest.approx(1e3 * line["frames_per_step"] / line["ms_per_step"], rel=1e-3)
    for leg in ("cold_window", "hash", "pcie_inclusive", "dropin", "lounge_2cm", "mesh", "cpu_baseline"):
        assert line[leg] is None, leg
    got = {f: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["color.npy", "tsdf.npy", "voxel_index.npy", "weight.npy"]
    assert sum(a.nbytes for a in got.values()) <= 64_000_000
    assert all(a.dtype in (np.float32, np.float64) and a.ndim == 1 for a in got.values())
    idx = got["voxel_index.npy"]
    assert len({len(a) for a in got.values()}) == 1 and np.all(np.diff(idx) >= 0) and idx[-1] < 512 ** 3
    import bench
    assert np.array_equal(idx, np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, 512 ** 3,
                                                                                       size=bench.DUMP_SAMPLE)))
    # three steps of 32 frames were fused: observed voxels carry weights 1..96, the rest the
    # fresh volume's tsdf 1, weight 0, colour 0
    w, t, c = got["weight.npy"], got["tsdf.npy"], got["color.npy"]
    seen = w > 0
    assert 0.05 < seen.mean() < 1  # (one frame alone updates 8-17 % of the volume)
    assert w.max() <= 96 and np.array_equal(w, np.round(w)) and np.all(np.abs(t) <= 1)
    assert np.all(t[~seen] == 1) and np.all(c[~seen] == 0)
