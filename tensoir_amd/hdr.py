"""Radiance RGBE pictures (`.hdr`) on the standard library and numpy: the environment maps TensoIR is relit with, and the file
mesh.export_environment writes the recovered light to.

    rgb = read_hdr("city.hdr")              # float32 [H, W, 3]
    write_hdr("light.hdr", rgb)

File: the line `#?RADIANCE`, header lines up to an empty one -- `FORMAT=32-bit_rle_rgbe` is required, `EXPOSURE=` and `#` comment
lines are ignored --, the resolution line `-Y H +X W` (rows from the top, columns from the left; any other order is refused), then H
scanlines of four bytes per pixel (r, g, b, e).  A scanline is either flat, W x 4 bytes, or new-style run-length coded: the marker
2 2 hi lo with (hi << 8 | lo) == W, 8 <= W <= 32767, then the four channels one after the other, each a sequence of
{n > 128, value}: n - 128 copies of value, or {1 <= n <= 128, n bytes}: those bytes.

Encoding of a pixel, v = max(r, g, b): v < 1e-32 -> (0, 0, 0, 0); otherwise (m, e) = frexp(v), each channel byte = floor(c * m * 256 / v)
(= floor(c * 2^(8 - e))) and the exponent byte = e + 128.
Decoding: c = (byte + 0.5) * 2^(E - 136), and E == 0 -> 0.  The + 0.5 puts the value in the middle of the interval the byte stands
for (Radiance's own colr_color; OpenCV's reader omits it and returns the interval's lower end).  It halves the worst error of a
round trip -- |read - x| <= max(r, g, b) / 256 instead of / 128 -- and makes write(read(file)) reproduce the file's pixel bytes,
since floor(byte + 0.5) = byte.  Negative and non-finite channels are written as 0."""
from __future__ import annotations

import numpy as np

MIN_RLE, MAX_RLE = 8, 32767


def _header(buf):
    """-> (H, W, offset of the first scanline)."""
    pos, lines = 0, []
    while True:
        end = buf.find(b"\n", pos)
        if end < 0:
            raise ValueError("hdr: truncated header")
        line = buf[pos:end].rstrip(b"\r")
        pos = end + 1
        if not lines and not line.startswith(b"#?"):
            raise ValueError("hdr: not a Radiance picture (no #? line)")
        if line == b"" and lines:
            break
        lines.append(line)
    fmt = [l.split(b"=", 1)[1].strip() for l in lines if l.startswith(b"FORMAT=")]
    if fmt != [b"32-bit_rle_rgbe"]:
        raise ValueError("hdr: FORMAT=32-bit_rle_rgbe expected")
    end = buf.find(b"\n", pos)
    if end < 0:
        raise ValueError("hdr: truncated header")
    res = buf[pos:end].split()
    if len(res) != 4 or res[0] != b"-Y" or res[2] != b"+X":
        raise ValueError(f"hdr: resolution line {buf[pos:end]!r}: only '-Y H +X W' is read")
    try:
        H, W = int(res[1]), int(res[3])
    except ValueError:
        raise ValueError(f"hdr: resolution line {buf[pos:end]!r}") from None
    if H < 1 or W < 1:
        raise ValueError("hdr: empty picture")
    return H, W, end + 1


def _rle_scanline(buf, pos, W, out):
    """One run-length scanline starting behind its marker -> out [W, 4]; returns the offset behind it."""
    n = len(buf)
    for ch in range(4):
        x = 0
        while x < W:
            if pos >= n:
                raise ValueError("hdr: truncated scanline")
            c = buf[pos]
            pos += 1
            if c > 128:
                c -= 128
                if pos >= n:
                    raise ValueError("hdr: truncated scanline")
                if x + c > W:
                    raise ValueError("hdr: a run overruns its scanline")
                out[x:x + c, ch] = buf[pos]
                pos += 1
            else:
                if c == 0:
                    raise ValueError("hdr: empty span in a run-length scanline")
                if x + c > W:
                    raise ValueError("hdr: a run overruns its scanline")
                if pos + c > n:
                    raise ValueError("hdr: truncated scanline")
                out[x:x + c, ch] = np.frombuffer(buf, np.uint8, c, pos)
                pos += c
            x += c
    return pos


def read_rgbe(path):
    """The picture's pixel bytes, uint8 [H, W, 4] = (r, g, b, e), scanlines decompressed."""
    with open(path, "rb") as fh:
        buf = fh.read()
    H, W, pos = _header(buf)
    out = np.empty((H, W, 4), np.uint8)
    for y in range(H):
        if MIN_RLE <= W <= MAX_RLE and buf[pos:pos + 2] == b"\x02\x02" and len(buf) >= pos + 4 and (buf[pos + 2] << 8 | buf[pos + 3]) == W:
            pos = _rle_scanline(buf, pos + 4, W, out[y])
        else:
            if pos + 4 * W > len(buf):
                raise ValueError("hdr: truncated scanline")
            out[y] = np.frombuffer(buf, np.uint8, 4 * W, pos).reshape(W, 4)
            pos += 4 * W
    return out


def decode_rgbe(rgbe):
    """uint8 [..., 4] -> float32 [..., 3]: (byte + 0.5) * 2^(E - 136), 0 where E == 0 (exact in float32)."""
    rgbe = np.asarray(rgbe, np.uint8)
    e = rgbe[..., 3:4].astype(np.int32)
    val = np.ldexp(rgbe[..., :3].astype(np.float64) + 0.5, e - 136)
    return np.where(e == 0, 0.0, val).astype(np.float32)


def encode_rgbe(rgb):
    """float [..., 3] -> uint8 [..., 4] (module docstring)."""
    c = np.asarray(rgb, np.float64)
    if c.shape[-1] != 3:
        raise ValueError("hdr: [..., 3] colours expected")
    c = np.where(np.isfinite(c) & (c > 0), c, 0.0)
    v = c.max(-1, keepdims=True)
    _, e = np.frexp(v)
    live = v >= 1e-32
    byte = np.floor(np.ldexp(c, 8 - e))                  # c * m * 256 / v with v = m 2^e; < 256 since m < 1
    out = np.concatenate([byte, e + 128.0], -1)
    return np.where(live, out, 0.0).astype(np.uint8)


def _rle_channel(row):
    """One channel of a scanline -> its run-length bytes: runs of at least 4 equal bytes (at most 127 per run), everything else in
    literal spans of at most 128."""
    out = bytearray()
    W = len(row)
    change = np.flatnonzero(row[1:] != row[:-1]) + 1
    starts = np.concatenate([[0], change]).tolist()
    ends = np.concatenate([change, [W]]).tolist()
    lit = 0                                                # start of the pending literal span

    def flush(upto):
        nonlocal lit
        while lit < upto:
            n = min(128, upto - lit)
            out.append(n)
            out.extend(row[lit:lit + n].tobytes())
            lit += n

    for a, b in zip(starts, ends):
        if b - a >= 4:
            flush(a)
            value = int(row[a])
            while a < b:
                n = min(127, b - a)
                out.append(128 + n)
                out.append(value)
                a += n
            lit = b
    flush(W)
    return bytes(out)


def write_rgbe(path, rgbe):
    """uint8 [H, W, 4] pixel bytes -> the file; run-length scanlines for 8 <= W <= 32767, flat ones otherwise."""
    rgbe = np.ascontiguousarray(rgbe, np.uint8)
    if rgbe.ndim != 3 or rgbe.shape[2] != 4 or rgbe.shape[0] < 1 or rgbe.shape[1] < 1:
        raise ValueError("hdr: [H, W, 4] pixel bytes expected")
    H, W = rgbe.shape[:2]
    parts = [b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n", f"-Y {H} +X {W}\n".encode()]
    for y in range(H):
        if MIN_RLE <= W <= MAX_RLE:
            parts.append(bytes((2, 2, W >> 8, W & 255)))
            parts.extend(_rle_channel(rgbe[y, :, ch]) for ch in range(4))
        else:
            parts.append(rgbe[y].tobytes())
    with open(path, "wb") as fh:
        fh.write(b"".join(parts))


def read_hdr(path):
    """-> float32 [H, W, 3], linear RGB, row 0 at the top."""
    return decode_rgbe(read_rgbe(path))


def write_hdr(path, rgb):
    """rgb [H, W, 3] (array or tensor, linear) -> a Radiance picture at path."""
    if hasattr(rgb, "detach"):
        rgb = rgb.detach().cpu().numpy()
    rgb = np.asarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("hdr: [H, W, 3] expected")
    write_rgbe(path, encode_rgbe(rgb))
