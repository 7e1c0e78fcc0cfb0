"""CPU: the launch decisions of the fused tile pass and the demultiplex kernels (seqkit_amd/csrc/sk_tileplan.h), in a stand-alone
program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

from seqkit_amd import build


def test_launch_plan_under_asan(tmp_path):
    """tests/cpp/tileplan_test.cpp: which lookup kernel a shape gets (pitch, key dwords, table size, the 1.5 M-row and 4 M-row
    thresholds, every SK_DEMUX_* / SK_LUT_* knob), its waves, LDS layout and workgroup cap; which shapes one many-batch launch serves;
    when the barcodes go by the table, when they ride in the tile pass (every factor switched off in turn) and when the neighbourhood
    table is wanted; slots, image and workgroup cap of the mate pass and the blocked pass on both sides of every boundary; the long-row
    fallback; the shape search's candidates and its choice among invented occupancy answers, ties included; the grid at 1, 3 and 256
    CUs — all against numbers written out by hand.  A sweep over the cross product of small value sets of every input holds every
    plan to the LDS ceiling, the kernels' launch bounds, many_ok => LDSTAB and the list of instantiations that exist."""
    exe = tmp_path / "tileplan_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", build.CSRC, "-o", str(exe), os.path.join(build.REPO, "tests", "cpp", "tileplan_test.cpp")], check=True)
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, check=True, env={"ASAN_OPTIONS": "detect_leaks=0"}).stdout.decode()
    assert out.startswith("ok: "), out
