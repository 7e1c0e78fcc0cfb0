"""CPU: what the host-pointer entry points stage through the ctx's workspace (seqkit_amd/csrc/sk_hoststage.h), in a stand-alone
program under the address and undefined-behaviour sanitizers."""
import os
import subprocess

from seqkit_amd import build


def test_staged_columns_under_asan(tmp_path):
    """tests/cpp/hoststage_test.cpp: the column list of every host-pointer entry point in every mode that changes it, at batch sizes
    around the row granules and the 256-byte granule, at chunk budgets of 2^6, 2^7, 2^12, 2^15 and the call's own, at row pitches from
    1 to 65535: the rows of a chunk equal the rule written out by hand and obey its granule and minimum; the chunks cover the batch
    once and in order; every region starts on a multiple of 256, the regions of a half are disjoint and inside it, the half equals
    the sum written out by hand, the halves and the tail add up to the total; every region of every chunk is memset in a heap buffer
    of exactly that total; the copies of every chunk start at the chunk's first row of the caller's column."""
    exe = tmp_path / "hoststage_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", build.CSRC, "-o", str(exe), os.path.join(build.REPO, "tests", "cpp", "hoststage_test.cpp")], check=True)
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, check=True, env={"ASAN_OPTIONS": "detect_leaks=0"}).stdout.decode()
    assert out.startswith("ok: "), out
