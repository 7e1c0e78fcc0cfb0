"""CPU: the record passes' working memory (seqkit_amd/csrc/sk_passmem.h) and the reader of the BAM header's reference list
(sk_bamfmt.h: bamfmt::RefList), in a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

from seqkit_amd import build


def test_pass_memory_and_reference_list_under_asan(tmp_path):
    """tests/cpp/passmem_test.cpp: the five file calls' layouts at record counts around the 256-byte granule and at 2^32 - 1 (aligned,
    disjoint, inside a total that equals the sum written out by hand, every region memset in a heap buffer of exactly that total), the
    two placements and the never-borrow flag; the header reader over every prefix of a header in a heap buffer of exactly that
    length, and its bad and empty cases."""
    exe = tmp_path / "passmem_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", build.CSRC, "-o", str(exe), os.path.join(build.REPO, "tests", "cpp", "passmem_test.cpp")], check=True)
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, check=True, env={"ASAN_OPTIONS": "detect_leaks=0"}).stdout.decode()
    assert out.startswith("ok: "), out
