"""CPU: the host side of `sam to` over the windows of the two file calls (seqkit_amd/csrc/sam_pairing.h) — the window loop of the
device-paired path and the host pairing that SEQKIT_HOST_PAIRING=1 and a declined sk_bam_file_pairs fall back to — in a stand-alone
program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

from seqkit_amd import build


def test_pairing_host_side_under_asan(tmp_path):
    """tests/cpp/pairing_test.cpp: 30 000 records of names that come one to six times, in windows of 1, 7, 1000 and all records, under a
    good key and under one that collides all the time; one name on 4 096 records; no records; an empty name and an empty text: the three
    outputs equal a std::map statement of the reference's loop, and the device-paired windows pass through unchanged."""
    exe = tmp_path / "pairing_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", build.CSRC, "-I", os.path.join(build.REPO, "include"), "-o", str(exe),
                    os.path.join(build.REPO, "tests", "cpp", "pairing_test.cpp")], check=True)
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, check=True, env={"ASAN_OPTIONS": "detect_leaks=0"}).stdout.decode()
    assert out.startswith("ok: "), out
