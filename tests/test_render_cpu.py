"""Pictures, host side (no GPU): the numpy oracle of the imsave byte rules against the matplotlib golden and, where
matplotlib is installed, against a live plt.imsave; the colormap tables; the PNG writer / reader; the sheet layout."""
import json
import os
import struct

import numpy as np
import pytest

import render_oracle as RO

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_imsave.npz")


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD, allow_pickle=False)
    return {k: z[k] for k in z.files}


def test_golden_holds_the_edge_values(gold):
    for key, edges in (("rgb_in", RO.edge_values_rgb()), ("gray_r_in", RO.edge_values_scalar())):
        a = gold[key]
        assert a.dtype == np.float32 and not np.isnan(a).any()
        assert a.shape[0] <= 48 and a.shape[1] <= 80
        have = set(a.reshape(-1).view(np.uint32).tolist())          # bit patterns: -0.0 and the denormal count
        assert set(edges.view(np.uint32).tolist()) <= have, key


def test_oracle_reproduces_every_golden_byte(gold):
    assert np.array_equal(RO.rgb_bytes(gold["rgb_in"], "signed"), gold["rgb_out"])
    assert np.array_equal(RO.scalar_bytes(gold["gray_r_in"], "gray_r", "unit"), gold["gray_r_out"])
    assert np.array_equal(RO.scalar_bytes(gold["gray_in"], "gray", "unit"), gold["gray_out"])
    # a 0/1 image is its own threshold mask: the "mask_true" rule writes the same file
    assert np.array_equal(RO.scalar_bytes(gold["gray_in"], "gray", "threshold"), gold["gray_out"])


def test_colormap_lut_equals_matplotlib_tables(gold):
    from floodgan.render import colormap_lut
    for name in ("gray", "gray_r"):
        assert np.array_equal(colormap_lut(name), gold["lut_" + name]), name
        assert np.array_equal(RO.lut(name), gold["lut_" + name]), name
    # the tables are not i / 255 - i
    i = np.arange(256)
    assert int((colormap_lut("gray")[:, 0] != i).sum()) == 24
    assert int((colormap_lut("gray_r")[:, 0] != 255 - i).sum()) == 38
    with pytest.raises(NotImplementedError):
        colormap_lut("viridis")


def test_oracle_equals_live_imsave(tmp_path):
    matplotlib = pytest.importorskip("matplotlib")
    Image = pytest.importorskip("PIL.Image")
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    def imsave(img, **kw):
        p = str(tmp_path / "a.png")
        plt.imsave(p, img, vmin=0, vmax=1, **kw)
        with Image.open(p) as im:
            return np.asarray(im, dtype=np.uint8).copy()

    rng = np.random.default_rng()
    x = rng.uniform(-1.3, 1.3, (37, 53, 3)).astype(np.float32)
    assert np.array_equal(RO.rgb_bytes(x, "signed"), imsave(np.clip((x + 1) * 0.5, 0, 1)))
    u = rng.uniform(-0.3, 1.3, (37, 53, 3)).astype(np.float32)
    assert np.array_equal(RO.rgb_bytes(u, "unit"), imsave(np.clip(u, 0, 1)))
    m = rng.uniform(-0.3, 1.3, (41, 29)).astype(np.float32)
    assert np.array_equal(RO.scalar_bytes(m, "gray_r", "unit"), imsave(m, cmap="gray_r"))
    assert np.array_equal(RO.scalar_bytes(m, "gray", "unit"), imsave(m, cmap="gray"))
    t = (m > 0.5).astype(np.float32)
    assert np.array_equal(RO.scalar_bytes(m, "gray", "threshold"), imsave(t, cmap="gray"))


def test_oracle_own_rules():
    x = np.array([[[np.nan, 0.0, 1.0], [np.inf, -np.inf, np.nan]]], dtype=np.float32)
    assert RO.rgb_bytes(x).tolist() == [[[0, 127, 255, 255], [255, 0, 0, 255]]]
    s = np.array([[np.nan, np.inf, -np.inf, -0.0]], dtype=np.float32)
    assert RO.scalar_bytes(s, "gray").tolist() == [[[0, 0, 0, 0], [255, 255, 255, 255], [0, 0, 0, 255], [0, 0, 0, 255]]]
    z = np.array([[0.0, 1e-3, -1e-3, np.nan]], dtype=np.float32)
    assert RO.scalar_bytes(z, "gray", "logit")[0, :, 0].tolist() == [0, 255, 0, 0]
    assert RO.scalar_bytes(z + np.float32(0.5), "gray", "threshold")[0, :, 0].tolist() == [0, 255, 0, 0]


# ------------------------------------------------------------------------------------------ PNG

SIZES = [(1, 1), (3, 5), (64, 67), (2, 20000)]


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("c", [3, 4])
def test_png_round_trip(tmp_path, h, w, c):
    from floodgan.png import read_png, write_png
    rng = np.random.default_rng(h * 131 + w + c)
    img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    text = {"floodgan:panels": json.dumps({"columns": ["Input (a_0)", "Generator Output"], "rows": ["a_0"]}),
            "Comment": "x"}
    path = str(tmp_path / "a.png")
    write_png(path, img, text=text)
    got, got_text = read_png(path)
    assert got.dtype == np.uint8 and got.shape == (h, w, c) and np.array_equal(got, img)
    assert got_text == text and json.loads(got_text["floodgan:panels"])["rows"] == ["a_0"]
    # a strided view is written as what it shows
    write_png(path, img[:, ::-1], text=None)
    assert np.array_equal(read_png(path)[0], img[:, ::-1]) and read_png(path)[1] == {}


def test_png_rejects_a_corrupted_crc(tmp_path):
    from floodgan.png import read_png, write_png
    path = str(tmp_path / "a.png")
    write_png(path, np.full((4, 4, 3), 9, dtype=np.uint8), text={"k": "v"})
    data = bytearray(open(path, "rb").read())
    read_png(path)
    for pos in (8 + 8 + 13 + 3,            # the last CRC byte of IHDR
                len(data) - 12 - 1):       # the last CRC byte of IDAT
        bad = bytearray(data)
        bad[pos] ^= 0x01
        with open(path, "wb") as f:
            f.write(bytes(bad))
        with pytest.raises(ValueError, match="CRC"):
            read_png(path)
    bad = bytearray(data)
    (n,) = struct.unpack(">I", data[8:12])
    bad[8 + 8] ^= 0x01                      # a payload byte of IHDR under the old CRC
    assert n == 13
    with open(path, "wb") as f:
        f.write(bytes(bad))
    with pytest.raises(ValueError, match="CRC"):
        read_png(path)
    with open(path, "wb") as f:
        f.write(b"not a png at all")
    with pytest.raises(ValueError, match="not a PNG"):
        read_png(path)


def test_png_rejects_bad_input(tmp_path):
    from floodgan.png import write_png
    path = str(tmp_path / "a.png")
    with pytest.raises(TypeError):
        write_png(path, np.zeros((4, 4, 3), dtype=np.float32))
    with pytest.raises(TypeError):
        write_png(path, np.zeros((4, 4, 3), dtype=np.int16))
    for shape in ((4, 4), (4, 4, 1), (4, 4, 2), (1, 4, 4, 3), (0, 4, 3)):
        with pytest.raises(ValueError):
            write_png(path, np.zeros(shape, dtype=np.uint8))
    assert not os.path.exists(path)


@pytest.mark.parametrize("h,w", SIZES[:3])
def test_png_against_pil(tmp_path, h, w):
    Image = pytest.importorskip("PIL.Image")
    from floodgan.png import read_image, read_png, write_png
    rng = np.random.default_rng(h + w)
    path = str(tmp_path / "a.png")
    for c, mode in ((3, "RGB"), (4, "RGBA")):
        img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        write_png(path, img, text={"k": "v"})
        with Image.open(path) as im:
            assert im.mode == mode and np.array_equal(np.asarray(im), img)
            assert im.text == {"k": "v"}
        # smooth content makes PIL's encoder pick the Sub / Up / Average / Paeth filters
        yy, xx = np.mgrid[0:h, 0:w]
        smooth = np.stack([(yy * 3 + xx * (k + 1)) % 256 for k in range(c)], -1).astype(np.uint8)
        smooth[h // 2:] = img[h // 2:]
        Image.fromarray(smooth).save(path)
        assert np.array_equal(read_png(path)[0], smooth)
        assert np.array_equal(read_image(path), smooth)
    grey = rng.integers(0, 256, (h, w), dtype=np.uint8)
    Image.fromarray(grey).save(path)
    assert np.array_equal(read_png(path)[0], grey[:, :, None])


def test_read_png_every_filter_type(tmp_path):
    """rows filtered by hand with each of the five types decode to the image"""
    import zlib

    from floodgan.png import SIGNATURE, _chunk, read_png
    rng = np.random.default_rng(3)
    h, w, c = 10, 7, 3
    img = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    flat = img.reshape(h, w * c).astype(np.int64)
    raw = bytearray()
    for y in range(h):
        ft = y % 5
        up = flat[y - 1] if y else np.zeros(w * c, dtype=np.int64)
        left = np.concatenate([np.zeros(c, dtype=np.int64), flat[y][:-c]])
        ul = np.concatenate([np.zeros(c, dtype=np.int64), up[:-c]])
        if ft == 0:
            pred = 0
        elif ft == 1:
            pred = left
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (left + up) // 2
        else:
            p = left + up - ul
            pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
        raw += bytes([ft]) + ((flat[y] - pred) & 255).astype(np.uint8).tobytes()
    path = str(tmp_path / "f.png")
    with open(path, "wb") as f:
        f.write(SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                + _chunk(b"IDAT", zlib.compress(bytes(raw)[:40])) + _chunk(b"IDAT", b"")
                + _chunk(b"IEND", b""))
    with pytest.raises(Exception):
        read_png(path)                                 # a truncated stream is an error, not a short image
    z = zlib.compress(bytes(raw))
    with open(path, "wb") as f:
        f.write(SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                + _chunk(b"IDAT", z[:11]) + _chunk(b"IDAT", z[11:]) + _chunk(b"IEND", b""))
    assert np.array_equal(read_png(path)[0], img)
    with open(path, "wb") as f:
        f.write(SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 1))
                + _chunk(b"IDAT", z) + _chunk(b"IEND", b""))
    with pytest.raises(ValueError, match="unsupported"):
        read_png(path)


# ------------------------------------------------------------------------------------------ sheets

@pytest.mark.parametrize("rows,cols,h,w", [(1, 3, 64, 64), (2, 4, 64, 64), (5, 6, 33, 130)])
def test_sheet_layout(rows, cols, h, w):
    from floodgan.render import sheet_layout
    height, width, off = sheet_layout(rows, cols, h, w)
    assert (height, width) == (rows * h + 8 * (rows - 1), cols * w + 8 * (cols - 1))
    assert len(off) == rows and all(len(r) == cols for r in off)
    assert off[0][0] == (0, 0)                                       # no outer margin
    assert off[rows - 1][cols - 1] == (height - h, width - w)
    for r in range(rows):
        for c in range(cols):
            assert off[r][c] == (r * (h + 8), c * (w + 8))
    # panels are disjoint and a gutter apart
    cover = np.zeros((height, width), dtype=np.int32)
    for r in range(rows):
        for c in range(cols):
            y, x = off[r][c]
            cover[y:y + h, x:x + w] += 1
    assert cover.max() == 1 and int(cover.sum()) == rows * cols * h * w
    assert sheet_layout(rows, cols, h, w, gutter=0)[:2] == (rows * h, cols * w)
    with pytest.raises(ValueError):
        sheet_layout(0, 3, 8, 8)


def test_new_names_are_exported():
    import floodgan
    for name in ("Canvas", "save_image", "save_sheet", "sheet_layout", "colormap_lut", "write_png", "read_png",
                 "compare_output_images"):
        assert name in floodgan.__all__ and hasattr(floodgan, name), name


@pytest.mark.parametrize("over", [dict(save_images_interval=5), dict(plot_mask_image="tile.png")])
def test_segmentation_constructor_accepts_the_plot_keywords(tmp_path, over):
    """segment.py passes both with its data_path: the interval is honoured by save_results, the picture's path is
    kept for the caller.  Without a data_path there is nowhere to write, and the constructor still raises."""
    from floodgan.segmentation import SegmentationModel
    m = SegmentationModel(device="cpu", train=False, verbose=False, data_path=str(tmp_path), **over)
    assert m.save_images_interval == over.get("save_images_interval", 0)
    assert m.mask_image_path == over.get("plot_mask_image")
    assert callable(m.plot_mask_image) and callable(m.plot_sample_images)
    with pytest.raises(NotImplementedError, match="data_path"):
        SegmentationModel(device="cpu", train=False, verbose=False, **over)
