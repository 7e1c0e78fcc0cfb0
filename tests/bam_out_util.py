"""What the tests of the three BAM-writing commands (`sam trim qnames` and its two siblings, `sam minimize`, `sam mark duplicates`)
share: the check of a rewrite-window call's windows, and the run of a command over its three paths."""
import struct
import zlib

import pytest

from tests import cli_util as cu


def zlib_members(data):
    """every BGZF member of data inflated by zlib itself, its CRC-32 and ISIZE checked; each member is at most 64 KiB"""
    out, at = [], 0
    while at < len(data):
        xlen, bsize = struct.unpack_from("<H", data, at + 10)[0], struct.unpack_from("<H", data, at + 16)[0] + 1
        assert bsize <= 65536 and data[at:at + 4] == b"\x1f\x8b\x08\x04"
        d = zlib.decompressobj(-15)
        raw = d.decompress(data[at + 12 + xlen:at + bsize - 8])
        assert d.eof and not d.unused_data
        crc, isize = struct.unpack_from("<II", data, at + bsize - 8)
        assert zlib.crc32(raw) == crc and len(raw) == isize
        out.append(raw)
        at += bsize
    assert at == len(data)
    return out


def checked_windows(ctx, result, m):
    """result: what ctx.bam_file_rewrite / _minimize / _markdup returned, (handled, records, [duplicates,] inflated output bytes, info);
    m: the command's model module.  The windows are taken and checked: (handled, inflated output, members, windows, info)."""
    handled, n_rec, raw_bytes, info = result[0], result[1], result[-2], result[-1]
    if not handled:
        assert all(v == 0 for v in result[1:-1])
        return False, None, None, 0, info
    wins = list(ctx.bam_file_rewrite_windows())
    assert wins[0]["n"] == 0 and wins[0]["first"] == 0 and wins[0]["bgzf"]          # the header's members first
    at = 0
    for w in wins[1:]:                                                                # then the records, in order
        assert w["first"] == at and w["n"] > 0
        at += w["n"]
    assert at == n_rec
    data = b"".join(w["bgzf"] for w in wins)
    assert data.endswith(m.EOF_BLOCK)
    mem = m.members(data)
    assert mem[-1][0] == b""
    assert all(0 < len(x) <= 0xFF00 for x, _ in mem[:-1])
    for w in wins:                                                                    # each window's members inflate to its raw bytes
        assert len(b"".join(x for x, _ in m.members(w["bgzf"]))) == w["raw_bytes"]
    out = b"".join(x for x, _ in mem)
    assert len(out) == raw_bytes
    return True, out, mem, len(wins), info


@pytest.fixture(scope="module")
def sam(hip_lib):
    from seqkit_amd import build
    build.build_hosts()
    return cu.SAM


def inflated(m, data):
    return b"".join(x for x, _ in m.members(data))


def three(sam, m, words, path, extra=(), expect_path="device path", env=None):
    """device path, host reader, stdin: (code, inflated stdout, stderr) of each, checked equal; the trace names the path"""
    who = ("sam " + " ".join(words) + ": ").encode()
    argv = list(words) + list(extra)
    runs = []
    for e, args, stdin in (({"SK_BAMFILE_TRACE": "1"}, argv + [str(path)], None),
                           ({"SK_BAMFILE_TRACE": "1", "SEQKIT_HOST_INFLATE": "1"}, argv + [str(path)], None),
                           ({"SK_BAMFILE_TRACE": "1"}, argv + ["-"], open(path, "rb").read())):
        runs.append(cu.run(sam, args, stdin=stdin, env=dict(e, **(env or {}))))
    traces = [[ln for ln in err.split(b"\n") if ln.startswith(who)] for _, _, err in runs]
    assert traces[0] and traces[0][0].startswith(who + expect_path.encode()), traces[0]
    assert traces[1] == [who + b"host reader"] and traces[2] == traces[1]
    assert runs[0][0] == runs[1][0] == runs[2][0]
    for _, out, _ in runs:
        assert out.endswith(m.EOF_BLOCK)
    outs = [inflated(m, out) for _, out, _ in runs]
    assert outs[0] == outs[1] == outs[2]
    strip = [b"\n".join(ln for ln in err.split(b"\n") if not ln.startswith(who) and not ln.startswith(b"sk_bam")) for _, _, err in runs]
    assert strip[0] == strip[1] == strip[2]
    return runs[0][0], outs[0], strip[0], runs
