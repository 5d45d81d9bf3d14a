"""The baseline JPEG encoder's contract (include/pienerf_hip.h: pn_jpeg_encode) restated in numpy float32: the same operations in the same order, each
rounded once, with the DCT matrix of tools/gen_jpeg_tables.py (the values of csrc/pn_jpeg_tables.h) and the tables of pienerf_amd/video.py.  The
kernels' bytes equal this module's bytes (tests/test_gpu_video.py); this module's files are checked against Pillow (tests/test_video_host.py)."""
import functools
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from gen_jpeg_tables import dct_matrix  # noqa: E402
from pienerf_amd import video  # noqa: E402

f32 = np.float32
SUBS = ("420", "444")
# (W, H): what the kernels are compared on byte for byte (tests/test_gpu_video.py) — one pixel, one block, padding on both axes, more blocks in an
# interval than a wave has lanes (272 x 48: 17 MCUs), a restart counter that wraps (16 x 272: 17 MCU rows in 4:2:0)
PARITY_SIZES = ((1, 1), (8, 8), (17, 33), (48, 64), (272, 48), (16, 272))
PARITY_QUALITIES = (50, 95)


def test_image(H, W, seed):
    """[H, W, 3] fp32: a smooth sinusoid in R and G, an 8-pixel checker in B, a uniform-noise rectangle over rows H/4..H/2 and columns W/4..W/2, the top
    H/8 rows at exactly 1.0, and a handful of entries at -0.5, 1.5 and NaN."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.zeros((H, W, 3), np.float32)
    img[..., 0] = 0.5 + 0.5 * np.sin(x / 7.0 + y / 11.0 + seed)
    img[..., 1] = 0.5 + 0.5 * np.cos(x / 5.0 - y / 13.0)
    img[..., 2] = ((x // 8 + y // 8) % 2)
    img[H // 4:H // 2, W // 4:W // 2] = rng.random((H // 2 - H // 4, W // 2 - W // 4, 3), dtype=np.float32)
    img[:H // 8] = 1.0
    flat = img.reshape(-1)
    at = rng.choice(flat.size, size=min(9, flat.size), replace=False)
    flat[at] = np.resize(np.array([-0.5, 1.5, np.nan], np.float32), at.size)
    return img
test_image.__test__ = False   # a helper, not a test


def truncate(image):
    """The 8-bit pixels as fp32: c = isnan(v) ? 0 : min(max(v, 0), 1), p = floor(c * 255)."""
    v = np.asarray(image, np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(v), f32(0), np.minimum(np.maximum(v, f32(0)), f32(1)))
    return np.floor(c * f32(255))


def _tiles(plane, my, mx):
    return plane.reshape(my, 8, mx, 8).transpose(0, 2, 1, 3)


def coefficients(pixels, qtabs, subsampling):
    """int [MCU rows, MCUs per row, blocks per MCU, 64]: the quantised coefficients in zigzag order, blocks in scan order."""
    p = np.asarray(pixels, np.float32)
    H, W = p.shape[:2]
    m, mx, my, bpm, _ = video.geometry(W, H, subsampling)
    p = p[np.minimum(np.arange(my * m), H - 1)][:, np.minimum(np.arange(mx * m), W - 1)]   # the last row and column replicated
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = f32(0.299) * R + f32(0.587) * G + f32(0.114) * B - f32(128.0)
    Cb = f32(-0.168735892) * R - f32(0.331264108) * G + f32(0.5) * B
    Cr = f32(0.5) * R - f32(0.418687589) * G - f32(0.081312411) * B
    assert Y.dtype == Cb.dtype == Cr.dtype == np.float32
    if bpm == 6:
        sub = lambda c: ((c[0::2, 0::2] + c[0::2, 1::2]) + (c[1::2, 0::2] + c[1::2, 1::2])) * f32(0.25)   # noqa: E731
        y4 = Y.reshape(my, 2, 8, mx, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(my, mx, 4, 8, 8)
        s = np.concatenate([y4, _tiles(sub(Cb), my, mx)[:, :, None], _tiles(sub(Cr), my, mx)[:, :, None]], axis=2)
        chroma = np.array([0, 0, 0, 0, 1, 1])
    else:
        s = np.stack([_tiles(Y, my, mx), _tiles(Cb, my, mx), _tiles(Cr, my, mx)], axis=2)
        chroma = np.array([0, 1, 1])
    C = dct_matrix()
    t = s[..., :, 0, None] * C[:, 0]                      # t[y][u] = sum_x s[y][x] C[u][x]
    for x in range(1, 8):
        t = t + s[..., :, x, None] * C[:, x]
    d = C[:, 0][:, None] * t[..., 0, None, :]             # d[v][u] = sum_y C[v][y] t[y][u]
    for yy in range(1, 8):
        d = d + C[:, yy][:, None] * t[..., yy, None, :]
    assert d.dtype == np.float32
    Q = np.array(qtabs, np.float32).reshape(2, 8, 8)[chroma]          # [bpm, 8, 8]
    q = np.rint(d / Q).reshape(my, mx, bpm, 64)[..., list(video.ZIGZAG)]
    q[..., 1:] = np.clip(q[..., 1:], -1023, 1023)
    return q.astype(np.int64)


def _size(v):
    return int(abs(v)).bit_length()


def _value(codes, symbol, v, size):
    code, length = codes[symbol]
    out = format(code, f"0{length}b")
    if size:
        out += format((v - 1 if v < 0 else v) & ((1 << size) - 1), f"0{size}b")
    return out


def scan(coef, subsampling, stats=None):
    """The entropy-coded scan of coefficients(): restart intervals of one MCU row, padded with 1-bits, stuffed, RSTm between them."""
    my, mx, bpm, _ = coef.shape
    comp = (0, 0, 0, 0, 1, 2) if bpm == 6 else (0, 1, 2)
    dc = [video.huffman_codes(*video.HUFFMAN[n]) for n in ("dc_luma", "dc_chroma")]
    ac = [video.huffman_codes(*video.HUFFMAN[n]) for n in ("ac_luma", "ac_chroma")]
    st = stats if stats is not None else {}
    for key in ("stuffed", "zrl", "no_eob", "dc_negative", "dc_zero", "restarts", "longest_block_bits"):
        st.setdefault(key, 0)
    out = bytearray()
    for r in range(my):
        pred, bits = [0, 0, 0], []
        for mcu in range(mx):
            for k in range(bpm):
                c, ch = coef[r, mcu, k], comp[k] > 0
                diff = int(min(max(c[0] - pred[comp[k]], -2047), 2047))
                pred[comp[k]] = int(c[0])
                st["dc_negative"] += diff < 0
                st["dc_zero"] += diff == 0
                block = [_value(dc[ch], _size(diff), diff, _size(diff))]
                run = 0
                for v in c[1:]:
                    v = int(v)
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        block.append(_value(ac[ch], 0xF0, 0, 0))
                        st["zrl"] += 1
                        run -= 16
                    block.append(_value(ac[ch], (run << 4) | _size(v), v, _size(v)))
                    run = 0
                if run:
                    block.append(_value(ac[ch], 0x00, 0, 0))
                else:
                    st["no_eob"] += 1
                block = "".join(block)
                st["longest_block_bits"] = max(st["longest_block_bits"], len(block))
                bits.append(block)
        bits = "".join(bits)
        bits += "1" * (-len(bits) % 8)
        seg = int(bits, 2).to_bytes(len(bits) // 8, "big")
        st["stuffed"] += seg.count(b"\xff")
        out += seg.replace(b"\xff", b"\xff\x00")
        if r + 1 < my:
            out += bytes([0xFF, 0xD0 + (r & 7)])
            st["restarts"] += 1
    return bytes(out)


def encode_pixels(pixels, quality, subsampling, stats=None):
    """The JPEG file of 8-bit pixels [H, W, 3] (any dtype holding 0 .. 255)."""
    p = np.asarray(pixels).astype(np.float32)
    H, W = p.shape[:2]
    qtabs = video.quant_tables(quality)
    return video.jpeg_header(W, H, qtabs, subsampling) + scan(coefficients(p, qtabs, subsampling), subsampling, stats) + b"\xff\xd9"


def encode(image, quality, subsampling, stats=None):
    """The JPEG file of an fp32 frame [H, W, 3], what JpegEncoder.encode returns for it."""
    return encode_pixels(truncate(image), quality, subsampling, stats)


@functools.lru_cache(maxsize=None)
def reference(W, H, quality, subsampling, seed=None):
    """(file bytes, the coder's statistics) of the test image of this size, computed once per session; the image's seed is W + H unless given."""
    stats = {}
    return encode(test_image(H, W, W + H if seed is None else seed), quality, subsampling, stats), stats


def decode(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        im.load()
        return np.asarray(im.convert("RGB")), dict(im.quantization)


def psnr(a, b):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 ** 2 / mse)
