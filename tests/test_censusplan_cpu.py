"""CPU: the launch decisions of the barcode census (seqkit_amd/csrc/sk_censusplan.h), in a stand-alone program under the address and
undefined-behaviour sanitizers."""
import os
import subprocess

from seqkit_amd import build


def test_census_plan_under_asan(tmp_path):
    """tests/cpp/censusplan_test.cpp: every SK_CENSUS_* variable at both ends of its range and just outside (SK_CENSUS_TILES present
    but unusable included); tiles per step at pitches 40/41 and 64/65; the row widths at 8/9 and 20/21 characters and records at
    24/25; the twelve instantiations by name; ten launches from end to end — tiles, wave slot, front-table entries, LDS bytes, grid,
    region capacity, instantiation — and the front-table knob against the layout's own limit; records at 2^19 -+ 1 rows; the grid at
    1, 3 and 256 CUs; a region at 1 024 / 1 025 workgroups and at the 2^27-record bound; the 2 GiB clamp of a launch at pitch 64;
    the smaller bite at room = least -+ 1, the rounding to 64 rows, the growth at exactly `need`, just above it and at the 2^32
    refusal — all against numbers written out by hand.  A sweep over barcode length x pitch x records x knobs x rows x CUs holds
    every launch to the LDS ceiling and to the layout as the kernel reads it (front table, sixteen slots and cursors without
    overlap, both queues inside a slot), to an instantiation that exists and is the one asked for, to a grid of at least one
    workgroup; and every walk over an input to bites that cover it exactly once, start on whole 64 rows and never leave the table
    more than half full without a grow."""
    exe = tmp_path / "censusplan_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", build.CSRC, "-o", str(exe), os.path.join(build.REPO, "tests", "cpp", "censusplan_test.cpp")], check=True)
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, check=True, env={"ASAN_OPTIONS": "detect_leaks=0"}).stdout.decode()
    assert out.startswith("ok: "), out
