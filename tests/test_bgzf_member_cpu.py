"""CPU: the BGZF member framer of seqkit_amd/csrc/sk_bamfmt.h (bgzf_head, bgzf_stored, bgzf_trailer), in a stand-alone program under
the address and undefined-behaviour sanitizers."""
import os
import subprocess

from seqkit_amd import build


def test_members_under_asan(tmp_path):
    """tests/cpp/bgzf_member_test.cpp: members of 0, 1, 2, 0xfeff, 0xff00 and 65535 - 26 - 5 bytes, stored and deflated by zlib, framed in
    heap buffers of exactly the member's size: the head field by field, BSIZE, the stored block's LEN and ~LEN, CRC32 and ISIZE against
    zlib's crc32, and the whole member through zlib's gzip decoder back to the input; an empty stored member against the EOF block: the
    same head and trailer, another BSIZE and payload."""
    exe = tmp_path / "bgzf_member_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", build.CSRC, "-o", str(exe), os.path.join(build.REPO, "tests", "cpp", "bgzf_member_test.cpp"), "-lz"], check=True)
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, check=True, env={"ASAN_OPTIONS": "detect_leaks=0"}).stdout.decode()
    assert out.startswith("ok: "), out
