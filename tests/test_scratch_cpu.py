"""The layout of a call's device arrays in one allocation, on the CPU: tools/check_scratch.cpp drives the
header both meshers take it from (csrc/tsdf_scratch.h) -- every single request and pair, and 2000 lists
of 3..7 requests, of 1-, 4- and 8-byte elements with counts of 0, 1 and around the 256-byte boundaries,
bound into a malloc'ed block of exactly bytes() and written end to end; counts past 2^31 by their
offsets alone -- under the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import pytest

from conftest import PKG, REPO


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = os.path.join(tmp_path_factory.mktemp("scratch"), "chk")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(REPO, "tools", "check_scratch.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    rows = {m.group(1): (int(m.group(2)), int(m.group(3)))
            for m in re.finditer(r"scratch (\w+) checked (\d+) bad (\d+)", out.stdout)}
    assert out.returncode == 0 and not out.stderr, out.stdout + out.stderr
    return rows


# (the lists enumerated: 3 sizes x 13 counts alone, their pairs, and the drawn ones)
LISTS = 39 + 39 * 39 + 2000


@pytest.mark.parametrize("prop, at_least", [
    ("aligned", LISTS),      # every array starts on a multiple of 256 (one check per array)
    ("ordered", LISTS),      # the ranges are disjoint and lie in request order
    ("bytes", LISTS),        # bytes(): the end of the last range, rounded up to 256
    ("bound", 2 * LISTS),    # each pointer is base + offset; each array keeps its pattern with all written
    ("large", 7),            # 2^31 + 3 eight-byte elements and what follows: nothing computed in 32 bits
    ("repeat", LISTS),       # a second layout of the same requests has the same offsets and size
])
def test_layout_property(report, prop, at_least):
    n, bad = report[prop]
    assert n >= at_least and bad == 0
