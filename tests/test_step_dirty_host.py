"""step_dirty's word-parallel arithmetic on the host (babyai_amd/csrc/bbai_dirty.hpp: four lut keys per word, the agent's id patched in once
per chunk, the changed cells as 16 bits split at the env boundary) against the per-cell definition, which tests/step_dirty_host.cpp writes
out plainly: every first cell 0..48 x every live count 1..16, encodings from the reachable ranges and their extremes, old ids equal /
differing in one byte by 0x01, 0x7F, 0x80, 0xFF / differing everywhere, the byte-flag function on all 16 zero / non-zero patterns, luts whose
agent's table differs from the plain one on every key and luts in which keys share ids.  The program is stand-alone (its own main): it is
compiled twice, plain and with the address and undefined-behaviour sanitizers, and both are run directly -- nothing is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "step_dirty_host.cpp")
BASE = ["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "babyai_amd", "csrc")]
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_packed_scan_equals_the_per_cell_definition(tmp_path, build):
    exe = str(tmp_path / ("step_dirty_host_" + build))
    subprocess.check_call(BASE + BUILDS[build] + ["-o", exe, SRC])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert run.returncode == 0, run.stdout[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    assert last.startswith("ok ") and int(last.split()[1]) > 500000, last
