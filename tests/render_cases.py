"""Shared by the render suites (test_render_host.py, test_gpu_render.py): a PNG decoder made of zlib and struct, and the
seeded box generator of the device tests."""
import struct
import zlib

import numpy as np


def png_chunks(data):
    """-> [(type, body)] of a PNG byte string; asserts the signature and every chunk's CRC"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xffffffff, kind
        chunks.append((kind, body))
        pos += 12 + n
    assert pos == len(data)
    return chunks


def decode_png(data):
    """the uint8 [h, w, 3] image of an 8-bit RGB PNG whose rows all carry filter type 0 (asserted)"""
    chunks = png_chunks(data)
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[2][1] == b""
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()
    return raw[:, 1:].reshape(h, w, 3)


KINDS = ("inside", "point", "left", "right", "top", "bottom", "outside", "inverted", "huge", "nan", "inf")


def random_boxes(rng, n, H, W, kinds=None):
    """n rows (x1, y1, x2, y2, score) on an H x W canvas. Nine rows in ten are boxes inside the canvas, zero-area points
    and boxes clipped on one of the four sides; the rest are wholly outside, inverted, or hold +-1e30, NaN or Inf.
    Scores are multiples of 1/1024 in (0, 1]. With `kinds` the k-th row is of kind kinds[k % len(kinds)]."""
    out = np.zeros((n, 5), np.float32)
    for k in range(n):
        if kinds is not None:
            kind = kinds[k % len(kinds)]
        else:
            u = rng.rand()
            kind = KINDS[int(u / 0.9 * 6)] if u < 0.9 else KINDS[6 + int((u - 0.9) / 0.1 * 5)]
        x1, y1 = rng.uniform(0, max(W - 1, 0)), rng.uniform(0, max(H - 1, 0))
        x2, y2 = x1 + rng.uniform(0, W / 2.0), y1 + rng.uniform(0, H / 2.0)
        if kind == "inside":
            x2, y2 = min(x2, W - 1), min(y2, H - 1)
        elif kind == "point":
            x2, y2 = x1, y1
        elif kind == "left":
            x1 = -rng.uniform(1, W)
        elif kind == "right":
            x2 = W + rng.uniform(1, W)
        elif kind == "top":
            y1 = -rng.uniform(1, H)
        elif kind == "bottom":
            y2 = H + rng.uniform(1, H)
        elif kind == "outside":
            x1, x2 = x1 + 2 * W + 40, x2 + 2 * W + 40
        elif kind == "inverted":
            x1, x2 = x2 + 1.5, x1
        elif kind == "huge":
            x1, x2 = (-1e30, 1e30) if k % 2 else (x1, 1e30)
        elif kind == "nan":
            y1 = np.nan
        elif kind == "inf":
            x2 = np.inf if k % 2 else -np.inf
        out[k] = (x1, y1, x2, y2, (1 + rng.randint(1024)) / 1024.0)
    return out
