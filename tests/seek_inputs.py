"""Shared by the seek table's tests (test_seek_table*.py, test_seek_decompress_fake_device.py, test_stream_seek_gpu.py): the table frame
of include/lizard_amd.h Part 3b written with struct — a model that shares no code with lizard_seek_host.c —, and for a stream that ends
in a usable table one damaged variant per rule of "usable"."""
import struct

MAGIC, TAG, VERSION = 0x184D2A5E, 0x4B535A4C, 1
USABLE, NONE, MORE, DAMAGED = 0, 1, 2, 3


def table_bytes(n):
    return 24 * n + 24


def pack_table(entries, n=None, version=VERSION, tag=TAG, magic=MAGIC, size=None):
    """entries: (offset, decodedBytes, prefixBytes[, flags]) per item."""
    body = b"".join(struct.pack("<QQII", e[0], e[1], e[2], e[3] if len(e) > 3 else 0) for e in entries)
    count = len(entries) if n is None else n
    return struct.pack("<II", magic, 24 * len(entries) + 16 if size is None else size) + body + struct.pack("<QII", count, version, tag)


def unpack_table(stream):
    """(entries as 4-tuples, tableOffset) of a stream that ends in a table frame; no judgement."""
    n, version, tag = struct.unpack("<QII", stream[-16:])
    at = len(stream) - table_bytes(n)
    return [struct.unpack_from("<QQII", stream, at + 8 + 24 * i) for i in range(n)], at


def damaged(stream):
    """[(name, bytes)]: variants of `stream` (which ends in a usable table of >= 3 items), one per rule a usable table obeys; none of
    them may be found usable, and the frames in front of the table are untouched in all but the last two."""
    entries, at = unpack_table(stream)
    n, body = len(entries), stream[:at]
    assert n >= 3

    def with_entry(i, **kw):
        e = dict(zip(("offset", "decoded", "prefix", "flags"), entries[i]), **kw)
        return entries[:i] + [(e["offset"], e["decoded"], e["prefix"], e["flags"])] + entries[i + 1:]

    out = [
        ("the tag is another", body + pack_table(entries, tag=TAG ^ 0x100)),
        ("the version is 2", body + pack_table(entries, version=2)),
        ("the size field is 8 too large", body + pack_table(entries, size=24 * n + 24)),
        ("the frame's magic is the tensor header's", body + pack_table(entries, magic=0x184D2A54)),
        ("the footer counts one item fewer", body + pack_table(entries, n=n - 1)),
        ("the footer counts one item more", body + pack_table(entries, n=n + 1)),
        ("the footer counts no item", body + pack_table(entries, n=0)),
        ("the footer counts 2^40 items", body + pack_table(entries, n=1 << 40)),
        ("entry 0 starts at 1", body + pack_table(with_entry(0, offset=1))),
        ("entry 1 starts inside entry 0's prefix", body + pack_table(with_entry(1, offset=entries[0][0] + entries[0][2]))),
        ("entry 1 starts behind entry 2", body + pack_table(with_entry(1, offset=entries[2][0] + 1))),
        ("the last entry starts behind the table's start", body + pack_table(with_entry(n - 1, offset=at + 1))),
        ("the last entry's prefix reaches the table", body + pack_table(with_entry(n - 1, prefix=at - entries[n - 1][0]))),
        ("a flag is set", body + pack_table(with_entry(1, flags=1))),
        ("the decoded sizes wrap", body + pack_table(with_entry(0, decoded=(1 << 64) - 1))),
        ("a byte behind the table", stream + b"\0"),
    ]
    assert tuple(name for name, _ in out) == DAMAGED_NAMES
    return out


# the names, for tests that parametrize over the variants without building a stream while they are collected
DAMAGED_NAMES = ("the tag is another", "the version is 2", "the size field is 8 too large", "the frame's magic is the tensor header's",
                 "the footer counts one item fewer", "the footer counts one item more", "the footer counts no item",
                 "the footer counts 2^40 items", "entry 0 starts at 1", "entry 1 starts inside entry 0's prefix", "entry 1 starts behind entry 2",
                 "the last entry starts behind the table's start", "the last entry's prefix reaches the table", "a flag is set",
                 "the decoded sizes wrap", "a byte behind the table")
LYING_NAMES = ("entry 1 decodes to one byte more", "entry 1 decodes to one byte less", "entry 1 starts one byte late",
               "two seekable streams back to back", "entry 1's prefix is one byte short")


def lying(stream):
    """[(name, bytes)]: USABLE tables that do not describe the frames in front of them; a reader must notice from the decoder's answers."""
    entries, at = unpack_table(stream)
    body = stream[:at]
    e1 = entries[1]
    out = [
        ("entry 1 decodes to one byte more", body + pack_table(entries[:1] + [(e1[0], e1[1] + 1, e1[2], 0)] + entries[2:])),
        ("entry 1 decodes to one byte less", body + pack_table(entries[:1] + [(e1[0], max(e1[1], 1) - 1, e1[2], 0)] + entries[2:])),
        ("entry 1 starts one byte late", body + pack_table(entries[:1] + [(e1[0] + 1, e1[1], e1[2], 0)] + entries[2:])),
        # the rules cannot refuse this one: the second table's offsets count from ITS stream's start, its last item "ends" where the
        # table starts, so that item swallows everything in between; only the decoder can tell
        ("two seekable streams back to back", stream + stream),
        ("entry 1's prefix is one byte short", body + pack_table(entries[:1] + [(e1[0], e1[1], max(e1[2], 1) - 1, 0)] + entries[2:])),
    ]
    assert tuple(name for name, _ in out) == LYING_NAMES
    return [(name, b) for name, b in out if b != stream]     # (a stream without prefixes has none to shorten)
