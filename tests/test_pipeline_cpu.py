"""The integrate's launch schedule on the CPU: tools/check_pipeline.cpp enumerates the header the
library's host loops take it from (csrc/tsdf_pipeline.h) -- calls of 1..9 batches of 1, 2, 8 and 32
frames, ragged last batches, every rotation of the buffer sets -- under the address and
undefined-behaviour sanitizers."""
import os
import re
import subprocess

import pytest

from conftest import PKG, REPO


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = os.path.join(tmp_path_factory.mktemp("pipeline"), "chk")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(REPO, "tools", "check_pipeline.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    rows = {m.group(1): (int(m.group(2)), int(m.group(3)))
            for m in re.finditer(r"pipeline (\w+) checked (\d+) bad (\d+)", out.stdout)}
    assert out.returncode == 0 and not out.stderr, out.stdout + out.stderr
    return rows


# (the calls enumerated: sum over nbat in {1, 2, 8, 32} of 9 * nbat frame counts, x 3 rotations)
CALLS = 3 * 9 * (1 + 2 + 8 + 32)


@pytest.mark.parametrize("prop, at_least", [
    ("launches", CALLS),   # exactly nb + 2 launches, L = -2 .. nb-1, and none outside
    ("once", CALLS),       # batch j: prepped in launch j-2, culled in j-1, integrated in j, once each
    ("same_set", CALLS),   # ... with one buffer set, slot and frame range in all three stages
    ("distinct", CALLS),   # the batches of one launch: distinct sets and places in the Batch array
    ("slots", CALLS - 3 * (1 + 2 + 8 + 32)),  # the slot filled before launch L: free of L-1, L, L+1; that of L-2
    ("frames", CALLS),     # f0 = j * nbat, 1 <= n <= nbat, only the last batch short, the n sum to n_frames
    ("rot", CALLS),        # the next call's rotation: (rot + nb) % kSets
    ("dense", CALLS // 3),  # rot = 0: set j % kSets
    ("inline", CALLS),     # the in-line walk: the same frames, slot j % kSlots
])
def test_schedule_property(report, prop, at_least):
    n, bad = report[prop]
    assert n >= at_least and bad == 0
