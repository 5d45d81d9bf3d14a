"""Video writing on CPU (no kernel is launched): the numpy restatement of the JPEG encoder's contract (tests/jpeg_reference.py) against Pillow's decoder
and Pillow's own encoder, the quantisation tables, the generated table header, the branches the parity set reaches, the AVI container, the C ABI's
refusals and main_render's flags (pienerf_amd/video.py, csrc/pn_jpeg.hip, tools/gen_jpeg_tables.py)."""
import ctypes
import io
import os
import struct
import tempfile

import numpy as np
import pytest

import jpeg_reference as R
from gen_jpeg_tables import HEADER, code_words, dct_matrix, header_text
from pienerf_amd import video

PN_ERR_ARG = 1
SUBS, PARITY_SIZES, PARITY_QUALITIES, reference = R.SUBS, R.PARITY_SIZES, R.PARITY_QUALITIES, R.reference


# ---------------------------------------------------------------- the restatement against Pillow
@pytest.mark.parametrize("W,H", ((1, 1), (8, 8), (16, 16), (17, 33), (40, 56), (48, 64)))
def test_pillow_decodes_the_restatement(W, H):
    for q in (50, 95):
        for sub in SUBS:
            data, _ = reference(W, H, q, sub)
            assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
            pixels, _ = R.decode(data)
            assert pixels.shape == (H, W, 3), (W, H, q, sub)


def _pillow_encoding(pixels8, q, sub):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(pixels8, "RGB").save(buf, "JPEG", quality=q, subsampling=2 if sub == "420" else 0)
    return buf.getvalue()


@pytest.mark.parametrize("W,H", ((17, 33), (40, 56), (48, 64), (128, 96)))
def test_quality_and_size_match_pillows_encoder(W, H):
    """PSNR to the truncated 8-bit source at least Pillow's own quality=q encoding of the same pixels minus 0.1 dB, and a file at most 1.10 x Pillow's.
    Measured with this restatement (fp32 DCT, both subsamplings, these four sizes, q = 25, 75, 95): PSNR -0.061 .. +0.139 dB, size 0.997 .. 1.064 x."""
    src = R.truncate(R.test_image(H, W, W + H)).astype(np.uint8)
    for q in (25, 75, 95):
        for sub in SUBS:
            ours, _ = reference(W, H, q, sub)
            theirs = _pillow_encoding(src, q, sub)
            p_ours, p_theirs = R.psnr(R.decode(ours)[0], src), R.psnr(R.decode(theirs)[0], src)
            print(f"{W}x{H} q={q} {sub}: PSNR {p_ours:.3f} dB (Pillow {p_theirs:.3f}), size {len(ours) / len(theirs):.3f} x")
            assert p_ours >= p_theirs - 0.1, (W, H, q, sub, p_ours, p_theirs)
            assert len(ours) <= 1.10 * len(theirs), (W, H, q, sub, len(ours), len(theirs))


def test_quantisation_tables_are_libjpegs():
    from PIL import Image
    for q in (1, 25, 50, 75, 90, 100):
        _, ours = R.decode(reference(16, 16, q, "420")[0])
        with Image.open(io.BytesIO(_pillow_encoding(np.zeros((16, 16, 3), np.uint8), q, "420"))) as im:
            theirs = dict(im.quantization)
        assert {k: list(v) for k, v in ours.items()} == {k: list(v) for k, v in theirs.items()}, q
    luma, chroma = video.quant_tables(50)
    assert luma == video.BASE_LUMA and chroma == video.BASE_CHROMA
    assert set(video.quant_tables(100)[0]) == {1} and max(video.quant_tables(1)[0]) == 255
    for bad in (0, 101, -3, 50.0, "50", True, None):
        with pytest.raises(ValueError):
            video.quant_tables(bad)


def test_header_segments():
    qt = video.quant_tables(75)
    h = video.jpeg_header(272, 48, qt, "420")
    assert h[:4] == b"\xff\xd8\xff\xe0" and h[6:11] == b"JFIF\x00"
    markers, at = [], 2
    while at < len(h):
        assert h[at] == 0xFF
        n = struct.unpack_from(">H", h, at + 2)[0]
        markers.append((h[at + 1], h[at + 4:at + 2 + n]))
        at += 2 + n
    assert [m for m, _ in markers] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    sof = markers[3][1]
    assert struct.unpack_from(">BHHB", sof) == (8, 48, 272, 3) and sof[6:] == bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])
    assert struct.unpack(">H", markers[8][1]) == (17,)   # one MCU row per restart interval
    assert struct.unpack(">H", [p for m, p in _segments(video.jpeg_header(272, 48, qt, "444")) if m == 0xDD][0]) == (34,)
    for bad in ((0, 8), (8, 0), (65536, 8)):
        with pytest.raises(ValueError):
            video.jpeg_header(*bad, qt, "420")
    with pytest.raises(ValueError):
        video.jpeg_header(8, 8, qt, "422")
    with pytest.raises(ValueError):
        video.jpeg_header(8, 8, (qt[0], (0,) * 64), "420")


def _segments(h):
    at = 2
    while at < len(h):
        n = struct.unpack_from(">H", h, at + 2)[0]
        yield h[at + 1], h[at + 4:at + 2 + n]
        at += 2 + n


# ---------------------------------------------------------------- the generated tables
def test_committed_table_header_is_the_generators_output():
    assert open(HEADER).read() == header_text(), "pienerf_amd/csrc/pn_jpeg_tables.h is stale: python tools/gen_jpeg_tables.py"
    C = dct_matrix().astype(np.float64)
    assert C.shape == (8, 8) and np.abs(C @ C.T - np.eye(8)).max() < 1e-6   # orthonormal
    assert sorted(video.ZIGZAG) == list(range(64)) and video.ZIGZAG[:6] == (0, 1, 8, 16, 9, 2) and video.ZIGZAG[-1] == 63


def test_huffman_tables_are_prefix_free_with_annex_k_counts():
    counts = {"dc_luma": (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), "dc_chroma": (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0),
              "ac_luma": (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125), "ac_chroma": (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119)}
    for name, (bits, vals) in video.HUFFMAN.items():
        assert tuple(bits) == counts[name] and len(set(vals)) == len(vals) == sum(bits)
        codes = video.huffman_codes(bits, vals)
        assert [sum(1 for c, n in codes.values() if n == length) for length in range(1, 17)] == list(bits)
        words = sorted(format(c, f"0{n}b") for c, n in codes.values())
        assert all(not b.startswith(a) for a, b in zip(words, words[1:])), name   # sorted: a prefix sorts directly in front of a word it begins
        assert all("0" in w for w in words), name                                   # no code of 1-bits alone (T.81 C.2)
        packed = code_words(name)
        assert len(packed) == (12 if name.startswith("dc") else 256)
        assert {s: (w & 0xFFFF, w >> 16) for s, w in enumerate(packed) if w} == codes
    ac = video.huffman_codes(*video.AC_LUMA)
    assert 0x00 in ac and 0xF0 in ac and len(ac) == 162 and max(n for _, n in ac.values()) == 16


# ---------------------------------------------------------------- the branches the parity set takes
def test_parity_set_reaches_every_branch_of_the_coder():
    """A condition on the inputs of the byte comparison with the kernels, asserted on the restatement's own output."""
    from pienerf_amd import _lib
    total, longest = {}, 0
    for W, H in PARITY_SIZES:
        for q in PARITY_QUALITIES:
            for sub in SUBS:
                data, st = reference(W, H, q, sub)
                for k, v in st.items():
                    total[k] = total.get(k, 0) + v
                longest = max(longest, st["longest_block_bits"])
                scan = data[len(video.jpeg_header(W, H, video.quant_tables(q), sub)):-2]
                assert len(scan) <= _lib.lib().pn_jpeg_stream_capacity(W, H, int(sub))
    assert total["stuffed"] >= 1 and total["zrl"] >= 1 and total["no_eob"] >= 1 and total["dc_negative"] >= 1 and total["dc_zero"] >= 1
    assert longest <= 20 + 63 * 26
    data, st = reference(16, 272, 50, "420")
    assert st["restarts"] == 16
    scan = data[len(video.jpeg_header(16, 272, video.quant_tables(50), "420")):-2]
    markers = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7]
    assert markers == [0xD0 + (r & 7) for r in range(16)]   # the counter wraps: ... D7 D0 ...
    data, _ = reference(17, 33, 95, "420")
    assert b"\xff\x00" in data[len(video.jpeg_header(17, 33, video.quant_tables(95), "420")):]


def test_truncation_is_save_images():
    """Frame f of a video is the JPEG of img_f.png's pixels: the restatement's 8-bit pixels are io.save_image's wherever the frame is a number."""
    from pienerf_amd.io import save_image
    img = R.test_image(33, 17, 5)
    ok = ~np.isnan(img)
    with tempfile.TemporaryDirectory() as d:
        data = save_image(np.where(ok, img, 0), os.path.join(d, "a.png"), 17, 33)
    assert np.array_equal(R.truncate(img)[ok], data.astype(np.float32)[ok])
    assert np.all(R.truncate(img)[~ok] == 0)


# ---------------------------------------------------------------- AVI
def test_avi_round_trip(tmp_path):
    frames = [reference(17, 33, 50, "420")[0], reference(17, 33, 95, "420")[0], b"\xff\xd8odd\xff\xd9", b"\xff\xd8even\xff\xd9"]
    assert any(len(f) & 1 for f in frames) and any(not len(f) & 1 for f in frames)
    path = str(tmp_path / "sub" / "a.avi")
    with video.AviWriter(path, 17, 33, fps=24) as w:
        for f in frames:
            w.add(f)
    info, back = video.read_avi(path)
    assert back == frames
    assert (info["width"], info["height"], info["frames"], info["stream_frames"], info["fps"]) == (17, 33, 4, 4, 24.0)
    assert info["stream_type"] == b"vids" and info["handler"] == b"MJPG" and info["compression"] == b"MJPG" and info["bit_count"] == 24
    assert info["bitmap_size"] == (17, 33) and info["usec_per_frame"] == round(1e6 / 24)
    assert info["max_bytes_per_sec"] == round(sum(map(len, frames)) * 24 / 4)
    raw = open(path, "rb").read()
    assert info["riff_size"] == len(raw) - 8 and len(raw) % 2 == 0
    assert [o for o, _ in info["index"]] == info["chunk_offsets"] and [s for _, s in info["index"]] == [len(f) for f in frames]
    for (off, size), f in zip(info["index"], frames):
        assert raw[off:off + 4] == b"00dc" and struct.unpack_from("<I", raw, off + 4)[0] == size and raw[off + 8:off + 8 + size] == f
    with pytest.raises(ValueError):
        w.add(b"late")


def test_avi_without_frames_is_a_valid_riff(tmp_path):
    path = str(tmp_path / "empty.avi")
    video.AviWriter(path, 8, 8, 30).close()
    info, frames = video.read_avi(path)
    assert frames == [] and info["frames"] == 0 and info["index"] == [] and info["riff_size"] == len(open(path, "rb").read()) - 8


def test_avi_refuses_to_pass_the_riff_limit(tmp_path, monkeypatch):
    assert video.RIFF_LIMIT == 0xFFFFFFFF
    monkeypatch.setattr(video, "RIFF_LIMIT", 4096)   # the same check against a limit a test can reach
    path = str(tmp_path / "small.avi")
    w = video.AviWriter(path, 8, 8, 30)
    w.add(b"x" * 1000)
    w.add(b"y" * 1000)
    with pytest.raises(ValueError, match="past RIFF"):
        w.add(b"z" * 3000)
    w.close()
    info, frames = video.read_avi(path)
    assert [len(f) for f in frames] == [1000, 1000] and info["riff_size"] + 8 <= 4096


def test_extract_writes_the_chunks(tmp_path):
    frames = [reference(8, 8, 50, "444")[0], reference(8, 8, 95, "444")[0]]
    with video.AviWriter(str(tmp_path / "a.avi"), 8, 8) as w:
        for f in frames:
            w.add(f)
    assert video.main([str(tmp_path / "a.avi"), "--extract", str(tmp_path / "out")]) == 0
    assert [open(tmp_path / "out" / f"frame_{i}.jpg", "rb").read() for i in range(2)] == frames
    with pytest.raises(ValueError):
        (tmp_path / "bad.avi").write_bytes(b"RIFF\x04\x00\x00\x00WAVE")
        video.read_avi(str(tmp_path / "bad.avi"))


# ---------------------------------------------------------------- C ABI
def test_c_abi_is_declared_exported_and_bound():
    from pienerf_amd import _lib, build
    text = open(build.HERE + "/../include/pienerf_hip.h").read()
    h = _lib.lib()
    for name in ("pn_jpeg_stream_capacity", "pn_jpeg_work_bytes", "pn_jpeg_encode"):
        assert name + "(" in text and name in _lib.SIGNATURES and hasattr(h, name)
    assert build.UNITS["pn_jpeg.hip"] == ["-ffp-contract=off"]
    assert _lib.SIGNATURES["pn_jpeg_encode"] == (_lib.i32, [_lib.P, _lib.u32, _lib.u32, _lib.i32, _lib.P, _lib.P, _lib.P, _lib.P, _lib.u64, _lib.P, _lib.P])


def test_sizes_and_refusals():
    from pienerf_amd import _lib
    h = _lib.lib()
    n_blocks, rows = 50 * 50 * 6, 50
    assert h.pn_jpeg_stream_capacity(800, 800, 420) == n_blocks * 416 + 2 * (rows - 1)
    assert h.pn_jpeg_stream_capacity(17, 33, 444) == 3 * 5 * 3 * 416 + 2 * 4
    assert h.pn_jpeg_work_bytes(800, 800, 420) >= n_blocks * (128 + 208 + 416) and h.pn_jpeg_work_bytes(1, 1, 444) > 0
    for W, H, sub in ((0, 8, 420), (8, 0, 420), (65536, 8, 420), (8, 65536, 444), (8, 8, 422), (8, 8, 0), (65535, 65535, 444)):
        assert h.pn_jpeg_stream_capacity(W, H, sub) == 0 and h.pn_jpeg_work_bytes(W, H, sub) == 0, (W, H, sub)

    # never dereferenced: every call below is refused before anything is enqueued
    image, work, stream, count = (ctypes.c_void_p(a) for a in (0x10000000, 0x20000000, 0x30000000, 0x40000000))
    good = (ctypes.c_uint8 * 64)(*video.quant_tables(90)[0])
    zero = (ctypes.c_uint8 * 64)(*([7] * 63 + [0]))
    W, H, sub = 48, 64, 420
    cap = h.pn_jpeg_stream_capacity(W, H, sub)
    wb = h.pn_jpeg_work_bytes(W, H, sub)

    def call(**kw):
        a = dict(image=image, W=W, H=H, sub=sub, ql=good, qc=good, work=work, stream=stream, cap=cap, count=count)
        a.update(kw)
        rc = h.pn_jpeg_encode(a["image"], a["W"], a["H"], a["sub"], a["ql"], a["qc"], a["work"], a["stream"], a["cap"], a["count"], None)
        return rc, h.pn_last_error().decode()

    for k in ("image", "ql", "qc", "work", "stream", "count"):
        assert call(**{k: None})[0] == PN_ERR_ARG, k
    for kw in (dict(W=0), dict(H=0), dict(W=65536), dict(H=65536), dict(sub=422), dict(sub=2)):
        rc, msg = call(**kw)
        assert rc == PN_ERR_ARG and "pn_jpeg_geometry" in msg, kw
    for kw in (dict(ql=zero), dict(qc=zero)):
        rc, msg = call(**kw)
        assert rc == PN_ERR_ARG and "!= 0" in msg, kw
    rc, msg = call(cap=cap - 1)
    assert rc == PN_ERR_ARG and "capacity" in msg
    overlaps = (dict(work=image), dict(stream=image), dict(count=image), dict(stream=work), dict(count=work), dict(count=stream),
                dict(work=ctypes.c_void_p(image.value + W * H * 12 - 16)), dict(stream=ctypes.c_void_p(work.value + wb - 1)),
                dict(count=ctypes.c_void_p(stream.value + cap - 1)), dict(image=ctypes.c_void_p(stream.value + cap - 1)))
    for kw in overlaps:
        rc, msg = call(**kw)
        assert rc == PN_ERR_ARG and "disjoint" in msg, kw


# ---------------------------------------------------------------- main_render
def test_main_render_flags_parse(tmp_path):
    from pienerf_amd import main_render as mr
    d = mr.parser().parse_args([])
    assert d.video is None and d.fps == 30 and d.video_quality == 90 and d.video_subsampling == "420" and d.no_png is False
    assert mr.video_path(d) is None
    mr.check_video_args(d)
    a = mr.parser().parse_args(["--video", "--out", "o"])
    assert a.video == "" and mr.video_path(a).replace("\\", "/") == "o/video.avi"
    b = mr.parser().parse_args(["--video", "x.avi", "--fps", "24", "--video_quality", "75", "--video_subsampling", "444", "--no_png"])
    assert (mr.video_path(b), b.fps, b.video_quality, b.video_subsampling, b.no_png) == ("x.avi", 24, 75, "444", True)
    mr.check_video_args(b)
    run = lambda *argv: mr.run(mr.parser().parse_args(list(argv) + ["--out", str(tmp_path / "o"), "--device", "cpu"]))   # noqa: E731
    with pytest.raises(SystemExit, match="--no_png needs --video"):
        run("--no_png")
    with pytest.raises(SystemExit, match="--video_quality"):
        run("--video", "--video_quality", "0")
    with pytest.raises(SystemExit, match="--fps"):
        run("--video", "--fps", "0")
    with pytest.raises(SystemExit):
        mr.parser().parse_args(["--video_subsampling", "422"])
