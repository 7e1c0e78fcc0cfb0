"""CPU: what `sam discard tail artifacts` computes on the host (seqkit_amd/csrc/sam_tails.h: the .fai parser, the offset arithmetic,
count_mismatches, count_right_end_offset, check_threshold), in a stand-alone program under the address and undefined-behaviour
sanitizers."""
import os
import subprocess

from seqkit_amd import build


def test_sam_tails_under_asan(tmp_path):
    """tests/cpp/sam_tails_test.cpp: well-formed and malformed index lines, the byte of a base at line ends and beyond 32 bits, a
    chromosome cut short, the reference's 29 self-test expectations, and walks that stop at a record's and a chromosome's edges, every
    buffer a heap block of exactly its contents' size"""
    exe = tmp_path / "sam_tails_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", build.CSRC, "-o", str(exe), os.path.join(build.REPO, "tests", "cpp", "sam_tails_test.cpp")], check=True)
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, check=True, env={"ASAN_OPTIONS": "detect_leaks=0"}).stdout.decode()
    assert out.startswith("ok: "), out
