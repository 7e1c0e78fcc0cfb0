"""CPU: host::GzWriter::write_members and pairing::write_member_windows (seqkit_amd/csrc/host_common.cpp, sam_pairing.h), which take the
finished members of sk_bam_file_pairs_gz to their files, in a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import subprocess
import zlib

from seqkit_amd import build
from tests.bam_out_util import zlib_members

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def stored(data):
    """the stored-block member tests/cpp/gz_members_test.cpp writes for `data`"""
    payload = b"\x01" + len(data).to_bytes(2, "little") + (len(data) ^ 0xFFFF).to_bytes(2, "little") + data
    head = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0]) + (18 + len(payload) + 8 - 1).to_bytes(2, "little")
    return head + payload + zlib.crc32(data).to_bytes(4, "little") + len(data).to_bytes(4, "little")


def pattern(n, salt):
    return bytes(65 + (k * (salt + 3)) % 23 for k in range(n))


def test_finished_members_reach_the_file_in_order_under_asan(hip_lib, tmp_path):
    """tests/cpp/gz_members_test.cpp: members on a fresh writer, zero bytes, and members between buffered texts of a few bytes and of
    several pool jobs: every file is what was handed in, in the order of the calls, and one EOF block; the windows of a stub pass through
    write_member_windows unchanged"""
    exe = tmp_path / "gz_members_test"
    csrc = build.CSRC
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(build.REPO, "include"), "-I", csrc, "-o", str(exe),
                    os.path.join(build.REPO, "tests", "cpp", "gz_members_test.cpp"), os.path.join(csrc, "host_common.cpp"), os.path.join(csrc, "host_inflate.cpp"),
                    "-L", build.LIBDIR, "-lseqkit_hip", f"-Wl,-rpath,{build.LIBDIR}", "-lz", "-ldl"], check=True)
    d = tmp_path / "out"
    d.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("SEQKIT_GPU_DEFLATE", None)
    out = subprocess.run([str(exe), str(d)], stdout=subprocess.PIPE, check=True, timeout=120, env=env).stdout.decode()
    assert out.startswith("ok: "), out
    two = stored(b"first member\n") + stored(pattern(40000, 1))
    mid, last = stored(b"between the texts\n"), stored(pattern(0xFF00, 2))
    assert (d / "fresh.gz").read_bytes() == two + EOF_BLOCK
    assert (d / "zero.gz").read_bytes() == EOF_BLOCK
    raw = (d / "order.gz").read_bytes()
    assert raw.endswith(mid + EOF_BLOCK) and raw.count(EOF_BLOCK) == 1
    a, b = raw.index(mid), raw.index(last)
    assert 0 < a < b < len(raw) - len(mid) - 28 and raw.count(mid) == 2 and raw.count(last) == 1    # the members as they were handed in
    join = lambda data: b"".join(zlib_members(data))
    assert join(raw[:a]) == b"head\n"
    assert join(raw[a + len(mid):b]) == pattern(1300000, 3)
    assert join(raw[b + len(last):len(raw) - len(mid) - 28]) == b"tail\n"
