"""PNG files on the host with the standard library only (zlib, struct): the encoder behind every picture floodgan
writes (floodgan.render), and a decoder for tests and for machines without PIL.

  write_png   8-bit RGB / RGBA, filter type 0 on every row, non-interlaced, optional tEXt chunks
  read_png    8-bit greyscale / RGB / RGBA, non-interlaced, all five filter types, CRCs checked: correct, not fast
  read_image  a user's picture as uint8 H x W x C: PIL when it is importable, read_png otherwise
"""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
_CHANNELS = {0: 1, 2: 3, 6: 4}          # colour type -> samples per pixel


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path, image, text=None, level=6):
    """image: uint8 numpy array [H, W, 3] or [H, W, 4] (any strides); text: {keyword: string} written as tEXt
    chunks (Latin-1, keywords of 1..79 characters)."""
    a = np.asarray(image)
    if a.dtype != np.uint8:
        raise TypeError(f"write_png: image must be uint8 (got {a.dtype})")
    if a.ndim != 3 or a.shape[2] not in (3, 4) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png: image must be [H, W, 3] or [H, W, 4] with H, W >= 1 (got shape {a.shape})")
    h, w, c = a.shape
    rows = np.zeros((h, 1 + w * c), dtype=np.uint8)            # filter type 0 in front of every row
    rows[:, 1:] = a.reshape(h, w * c)
    out = bytearray(SIGNATURE)
    out += _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 6, 0, 0, 0))
    for key, value in (text or {}).items():
        k = key.encode("latin-1")
        if not 1 <= len(k) <= 79 or b"\x00" in k:
            raise ValueError(f"write_png: bad tEXt keyword {key!r}")
        out += _chunk(b"tEXt", k + b"\x00" + str(value).encode("latin-1"))
    out += _chunk(b"IDAT", zlib.compress(rows.tobytes(), level))
    out += _chunk(b"IEND", b"")
    with open(path, "wb") as f:
        f.write(bytes(out))


def _unfilter(raw, h, w, c):
    stride = w * c
    if len(raw) != h * (stride + 1):
        raise ValueError(f"read_png: {len(raw)} bytes of image data for {h} rows of {stride + 1}")
    out = np.zeros((h, stride), dtype=np.uint8)
    prev = np.zeros(stride, dtype=np.int64)
    for y in range(h):
        ft = raw[y * (stride + 1)]
        line = np.frombuffer(raw, dtype=np.uint8, count=stride, offset=y * (stride + 1) + 1).astype(np.int64)
        if ft == 0:
            cur = line
        elif ft == 1:                                          # Sub: a running sum per sample position
            cur = np.cumsum(line.reshape(w, c), axis=0).reshape(stride) & 255
        elif ft == 2:                                          # Up
            cur = (line + prev) & 255
        elif ft in (3, 4):
            cur = np.zeros(stride, dtype=np.int64)
            lst, prv = line.tolist(), prev.tolist()
            res = [0] * stride
            for i in range(stride):
                left = res[i - c] if i >= c else 0
                up = prv[i]
                if ft == 3:                                    # Average
                    pred = (left + up) >> 1
                else:                                          # Paeth
                    ul = prv[i - c] if i >= c else 0
                    p = left + up - ul
                    pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
                    pred = left if pa <= pb and pa <= pc else (up if pb <= pc else ul)
                res[i] = (lst[i] + pred) & 255
            cur[:] = res
        else:
            raise ValueError(f"read_png: unknown filter type {ft} on row {y}")
        out[y] = cur
        prev = cur
    return out.reshape(h, w, c)


def read_png(path):
    """(uint8 [H, W, C] array, {keyword: string} of the tEXt chunks); C = 1, 3 or 4.  Raises ValueError on a bad
    signature, a CRC mismatch or a format outside 8-bit greyscale / RGB / RGBA non-interlaced."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != SIGNATURE:
        raise ValueError(f"read_png: {path} is not a PNG file")
    pos, header, idat, text, ended = 8, None, [], {}, False
    while pos < len(data):
        if pos + 12 > len(data):
            raise ValueError("read_png: truncated chunk")
        (n,), kind = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        if len(body) != n or pos + 12 + n > len(data):
            raise ValueError("read_png: truncated chunk")
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        if crc != (zlib.crc32(kind + body) & 0xFFFFFFFF):
            raise ValueError(f"read_png: CRC mismatch in chunk {kind!r}")
        pos += 12 + n
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"tEXt":
            k, _, v = body.partition(b"\x00")
            text[k.decode("latin-1")] = v.decode("latin-1")
        elif kind == b"IEND":
            ended = True
            break
    if header is None or not idat or not ended:
        raise ValueError("read_png: missing IHDR, IDAT or IEND")
    w, h, depth, ctype, comp, filt, interlace = header
    if depth != 8 or ctype not in _CHANNELS or comp != 0 or filt != 0 or interlace != 0:
        raise ValueError(f"read_png: unsupported format (bit depth {depth}, colour type {ctype}, interlace "
                         f"{interlace}); 8-bit greyscale / RGB / RGBA non-interlaced only")
    return _unfilter(zlib.decompress(b"".join(idat)), h, w, _CHANNELS[ctype]), text


def read_image(path):
    """A user's picture as uint8 [H, W, C]: through PIL (any format it knows) when PIL is importable, else read_png."""
    try:
        from PIL import Image
    except ImportError:
        return read_png(path)[0]
    with Image.open(path) as im:
        if im.mode not in ("L", "RGB", "RGBA"):
            im = im.convert("RGBA" if "A" in im.mode or "transparency" in im.info else "RGB")
        a = np.asarray(im, dtype=np.uint8)
    return a[:, :, None] if a.ndim == 2 else a
