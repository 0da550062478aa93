"""The zlib streams and the one-bit mutations that the Adler-32 verification tests share (tests/test_deflate_verify.py on the host,
tests/test_deflate_verify_gpu.py on the device): the streams of test_deflate_streams_of_every_block_type_on_the_device — stored, fixed
and dynamic blocks, levels 0 / 1 / 6 / 9, run-length and Huffman-only strategies, a match at the far end of the window — and, per
stream, every bit of the two header bytes, every bit of the four trailer bytes, the padding bits in front of a stored block's LEN and
seeded positions in between. What is expected of a case is whatever zlib does with it: ``zlib_outcome``."""
import zlib

import numpy as np

from treedetection_amd.synth import make_tile

SETTINGS = ((0, 0), (1, 0), (6, 0), (9, 0), (6, zlib.Z_FIXED), (6, zlib.Z_RLE), (6, zlib.Z_HUFFMAN_ONLY))
RANDOM_FLIPS_PER_STREAM = 24


def _raster(bands, h, w, seed=0):
    rgb, _ = make_tile(seed, max(h, w))
    img = np.concatenate([rgb, rgb[..., 1:2]], axis=2)[:h, :w, :bands].transpose(2, 0, 1).copy()
    img[:, h // 5: h // 2, w // 8: w // 2] = 7
    img[:, -40:, -90:] = np.arange(90, dtype=np.uint8)
    return img


def valid_streams():
    """→ (streams, raws): 49 zlib streams and what each inflates to."""
    rng = np.random.default_rng(7)
    img = _raster(4, 300, 1100, seed=2)
    raws = [img.transpose(1, 2, 0).tobytes(), bytes(200000), rng.integers(0, 256, 150000, dtype=np.uint8).tobytes(), b"x",
            (b"abcdefghijklmnopqrstuvwxyz0123456789" * 3000), rng.integers(0, 3, 250000, dtype=np.uint8).tobytes()]
    far = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()         # a match that reaches back exactly 32 768 bytes
    raws.append(far + far[:300] + far[5:400])
    streams, expect = [], []
    for raw in raws:
        for level, strategy in SETTINGS:
            c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
            streams.append(c.compress(raw) + c.flush())
            expect.append(raw)
    return streams, expect


def flips(streams):
    """→ [(stream index, bit position)]: bit position = 8 * byte + bit, bit 0 the byte's lowest. Deterministic."""
    rng = np.random.default_rng(20240611)
    out = []
    for k, s in enumerate(streams):
        n = len(s)
        bits = list(range(16)) + list(range(8 * (n - 4), 8 * n))        # the header, the trailer
        if (s[2] >> 1) & 3 == 0:                                        # first block stored: bits 3 .. 7 of its first byte are padding
            bits += [16 + b for b in range(3, 8)]
        if n > 6:
            bits += sorted(int(b) for b in rng.integers(16, 8 * (n - 4), RANDOM_FLIPS_PER_STREAM))
        out += [(k, b) for b in bits]
    return out


def flipped(s, bit):
    m = bytearray(s)
    m[bit >> 3] ^= 1 << (bit & 7)
    return bytes(m)


def zlib_outcome(s):
    """What zlib makes of a stream: its bytes, or None when it raises or the stream is incomplete."""
    d = zlib.decompressobj()
    try:
        out = d.decompress(s)
    except zlib.error:
        return None
    return out if d.eof else None
