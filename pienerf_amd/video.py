"""A run as a video: baseline JPEG frames encoded on the device (csrc/pn_jpeg.hip) in an MJPEG AVI that any player opens.

    enc = JpegEncoder(W, H, quality=90, subsampling="420")
    with AviWriter("run.avi", W, H, fps=30) as avi:
        for ...:
            avi.add(enc.encode(out["image"]))        # out: what SimRenderHarness.step returns, still on the device
    python -m pienerf_amd.video run.avi --extract DIR   # frame_{f}.jpg, the chunks as they lie in the file

The device does the per-pixel work (colour transform, 8 x 8 DCT, quantisation) and the entropy coding (one restart interval per MCU row, coded in
parallel inside the interval); the finished scan — tens of kilobytes for an 800 x 800 frame — crosses to the host, which prepends a header built once per run
(`jpeg_header`) and appends one AVI chunk.  The arithmetic is fixed operation by operation (include/pienerf_hip.h: pn_jpeg_encode) and restated in
numpy by tests/jpeg_reference.py, byte for byte.  Pixels are truncated to 8 bits as io.save_image does: frame f of the video is the JPEG of
img_f.png's pixels.  The Huffman tables are the typical ones of ITU-T T.81 Annex K (K.3 - K.6), the quantisation tables its K.1 / K.2 scaled by
libjpeg's quality rule.  No torch at import: the tables, the header and the AVI container are plain Python.
"""
import os
import struct

# ITU-T T.81 Annex K.1 / K.2: the base quantisation tables, natural (row-major) order
BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32

# natural index of the k-th coefficient in zigzag order
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)

# Annex K.3 - K.6 as (BITS: codes per length 1..16, HUFFVAL: the symbols in code order)
_AC_TAIL = tuple((r << 4) | s for r in range(16) for s in range(1, 11))   # every run / size pair; the tables order them by frequency
DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d),
           (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
            0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
            0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
            0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
            0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
            0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
            0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa))
AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77),
             (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
              0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
              0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
              0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
              0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
              0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
              0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa))
HUFFMAN = {"dc_luma": DC_LUMA, "ac_luma": AC_LUMA, "dc_chroma": DC_CHROMA, "ac_chroma": AC_CHROMA}
assert all(sum(b) == len(v) for b, v in HUFFMAN.values()) and sorted(AC_LUMA[1]) == sorted(AC_CHROMA[1]) == sorted(_AC_TAIL + (0x00, 0xf0))

SUBSAMPLINGS = {"420": 420, "444": 444, 420: 420, 444: 444}


def huffman_codes(bits, vals):
    """T.81 Annex C: {symbol: (code, length)} of a table given as BITS / HUFFVAL."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def subsampling_code(subsampling):
    try:
        return SUBSAMPLINGS[subsampling]
    except (KeyError, TypeError):
        raise ValueError(f"subsampling is '420' or '444', not {subsampling!r}") from None


def geometry(W, H, subsampling):
    """(mcu size in pixels, MCUs per row, MCU rows, blocks per MCU, blocks) of a frame."""
    sub = subsampling_code(subsampling)
    m, bpm = (16, 6) if sub == 420 else (8, 3)
    mx, my = (W + m - 1) // m, (H + m - 1) // m
    return m, mx, my, bpm, mx * my * bpm


def quant_tables(quality):
    """(luma, chroma): 64 entries each in natural order, libjpeg's jpeg_set_quality (baseline) on the Annex K tables."""
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError(f"quality is an integer in 1 .. 100, not {quality!r}")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(tuple(min(max((b * scale + 50) // 100, 1), 255) for b in base) for base in (BASE_LUMA, BASE_CHROMA))


def _check_qtabs(qtabs):
    luma, chroma = (tuple(int(v) for v in t) for t in qtabs)
    if len(luma) != 64 or len(chroma) != 64 or not all(1 <= v <= 255 for v in luma + chroma):
        raise ValueError("a quantisation table has 64 entries in 1 .. 255")
    return luma, chroma


def _segment(marker, payload):
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def jpeg_header(W, H, qtabs, subsampling):
    """Everything in front of the scan: SOI, JFIF APP0, DQT x 2, SOF0, DHT x 4, DRI (one MCU row), SOS."""
    if not (1 <= W <= 65535 and 1 <= H <= 65535):
        raise ValueError("a baseline JPEG is 1 .. 65535 pixels wide and high")
    luma, chroma = _check_qtabs(qtabs)
    _, mx, _, _, _ = geometry(W, H, subsampling)
    hv = 0x22 if subsampling_code(subsampling) == 420 else 0x11
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    for tid, tab in ((0, luma), (1, chroma)):
        out.append(_segment(0xDB, bytes([tid]) + bytes(tab[n] for n in ZIGZAG)))
    out.append(_segment(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, hv, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for tc_th, name in ((0x00, "dc_luma"), (0x10, "ac_luma"), (0x01, "dc_chroma"), (0x11, "ac_chroma")):
        bits, vals = HUFFMAN[name]
        out.append(_segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals)))
    out.append(_segment(0xDD, struct.pack(">H", mx)))
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b"".join(out)


class JpegEncoder:
    """Frames of one size as baseline JPEGs, encoded by pn_jpeg_encode.  Owns the launch's work area, a device buffer of the scan's proven bound and a
    pinned host buffer of the same size.  enqueue() makes no host wait and is legal inside a stream capture; fetch() is the host wait."""

    def __init__(self, W, H, quality=90, subsampling="420", device="cuda"):
        import ctypes
        import torch
        from ._lib import lib
        self.W, self.H, self.sub = int(W), int(H), subsampling_code(subsampling)
        self.qtabs = quant_tables(quality)
        self.header = jpeg_header(self.W, self.H, self.qtabs, self.sub)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("JpegEncoder runs on the GPU only (HIP kernels); there is no CPU fallback")
        h = lib()
        self.capacity = int(h.pn_jpeg_stream_capacity(self.W, self.H, self.sub))
        work = int(h.pn_jpeg_work_bytes(self.W, self.H, self.sub))
        if self.capacity == 0 or work == 0:
            raise ValueError(f"a frame of {W} x {H} cannot be encoded")
        self._q = tuple((ctypes.c_uint8 * 64)(*t) for t in self.qtabs)
        self._work = torch.empty((work + 15) // 16 * 2, dtype=torch.int64, device=self.device)
        self._stream = torch.empty(self.capacity, dtype=torch.uint8, device=self.device)
        self._nbytes = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._host = torch.empty(self.capacity, dtype=torch.uint8, pin_memory=True)
        self._host_n = torch.zeros(1, dtype=torch.int32, pin_memory=True)

    def enqueue(self, image):
        """Launches the encode of `image` ([..., H, W, 3] fp32, contiguous, on this encoder's device) on the current stream."""
        import torch
        from ._lib import check, lib, ptr, stream_ptr
        if not (torch.is_tensor(image) and image.dtype == torch.float32 and image.is_contiguous() and image.numel() == self.H * self.W * 3
                and image.device == self._stream.device):
            raise ValueError(f"a frame is a contiguous fp32 tensor of {self.H} x {self.W} x 3 elements on {self._stream.device}")
        with torch.cuda.device(image.device):
            check(lib().pn_jpeg_encode(ptr(image), self.W, self.H, self.sub, self._q[0], self._q[1], ptr(self._work), ptr(self._stream), self.capacity,
                                       ptr(self._nbytes), stream_ptr()), "jpeg encode")

    def fetch(self):
        """The last enqueued frame as a complete JPEG file: waits for the count, then copies exactly that many bytes."""
        import torch
        with torch.cuda.device(self._stream.device):
            self._host_n.copy_(self._nbytes, non_blocking=True)
            torch.cuda.current_stream().synchronize()
            n = int(self._host_n[0])
            if not 0 < n <= self.capacity:
                raise RuntimeError(f"jpeg: the device reports a scan of {n} bytes (capacity {self.capacity})")
            self._host[:n].copy_(self._stream[:n], non_blocking=True)
            torch.cuda.current_stream().synchronize()
        self.last_scan_bytes = n
        return self.header + self._host[:n].numpy().tobytes() + b"\xff\xd9"

    def encode(self, image):
        self.enqueue(image)
        return self.fetch()


RIFF_LIMIT = 0xFFFFFFFF   # a RIFF chunk's size field


class AviWriter:
    """RIFF 'AVI ' with one MJPG video stream: hdrl (avih, strl: strh + a BITMAPINFOHEADER), LIST movi of 00dc chunks, idx1.  The counts and sizes that
    are only known at the end are patched by close()."""

    _HDRL = 4 + (8 + 56) + (12 + (8 + 56) + (8 + 40))   # 'hdrl' + avih + LIST strl

    def __init__(self, path, W, H, fps=30):
        if not (W > 0 and H > 0 and fps > 0):
            raise ValueError("AviWriter: W, H and fps are positive")
        self.path, self.W, self.H, self.fps = path, int(W), int(H), float(fps)
        self.index, self.max_chunk, self.closed = [], 0, False
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self.f = open(path, "wb")
        self.f.write(self._headers())
        self.movi = self.f.tell() - 4   # the 'movi' fourcc: idx1's offsets count from here

    def _headers(self):
        n, rate = len(self.index), int(round(self.fps * 1000))
        total = sum(size for _, size in self.index)
        bps = int(round(total * self.fps / n)) if n else 0
        movi_size = 4 + sum(8 + size + (size & 1) for _, size in self.index)
        riff_size = 4 + (8 + self._HDRL) + (8 + movi_size) + (8 + 16 * n)
        avih = struct.pack("<14I", int(round(1e6 / self.fps)), min(bps, RIFF_LIMIT), 0, 0x10, n, 0, 1, self.max_chunk, self.W, self.H, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIiI4h", b"vids", b"MJPG", 0, 0, 0, 0, 1000, rate, 0, n, self.max_chunk, -1, 0, 0, 0, self.W, self.H)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.W, self.H, 1, 24, b"MJPG", self.W * self.H * 3, 0, 0, 0, 0)
        strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + \
            b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + strl
        assert len(hdrl) == self._HDRL
        return b"RIFF" + struct.pack("<I", riff_size) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl + \
            b"LIST" + struct.pack("<I", movi_size) + b"movi"

    def add(self, jpeg_bytes):
        if self.closed:
            raise ValueError("AviWriter: the file is closed")
        size = len(jpeg_bytes)
        end = self.f.tell() + 8 + size + (size & 1) + 8 + 16 * (len(self.index) + 1)   # the file's length if this frame were the last
        if end - 8 > RIFF_LIMIT:
            raise ValueError(f"AviWriter: frame {len(self.index)} would take {self.path} past RIFF's {RIFF_LIMIT} bytes")
        self.index.append((self.f.tell() - self.movi, size))
        self.f.write(b"00dc" + struct.pack("<I", size))
        self.f.write(jpeg_bytes)
        if size & 1:
            self.f.write(b"\x00")
        self.max_chunk = max(self.max_chunk, size)

    def close(self):
        if self.closed:
            return
        self.closed = True
        self.f.write(b"idx1" + struct.pack("<I", 16 * len(self.index)))
        for off, size in self.index:
            self.f.write(struct.pack("<4sIII", b"00dc", 0x10, off, size))
        self.f.seek(0)
        self.f.write(self._headers())
        self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _chunks(buf, start, end):
    """(fourcc, data start, size) of the chunks lying in buf[start:end]."""
    at = start
    while at + 8 <= end:
        cc, size = buf[at:at + 4], struct.unpack_from("<I", buf, at + 4)[0]
        if at + 8 + size > end:
            raise ValueError(f"AVI: chunk {cc!r} at {at} runs past its parent")
        yield cc, at + 8, size
        at += 8 + size + (size & 1)


def read_avi(path):
    """(info, [the 00dc chunks' bytes]) of a file AviWriter wrote (or any AVI with one video stream): walks the chunks, decodes nothing.
    info: width, height, fps, frames (avih's count), handler, compression, bit_count, max_bytes_per_sec, chunk_offsets (file offsets of the chunk
    headers), index ([(file offset, size)] from idx1) and riff_size."""
    with open(path, "rb") as f:
        buf = f.read()
    if len(buf) < 12 or buf[:4] != b"RIFF" or buf[8:12] != b"AVI ":
        raise ValueError(f"{path}: not a RIFF AVI file")
    riff_size = struct.unpack_from("<I", buf, 4)[0]
    if riff_size + 8 > len(buf):
        raise ValueError(f"{path}: RIFF says {riff_size + 8} bytes, the file has {len(buf)}")
    info, frames, offsets, movi = {"riff_size": riff_size, "index": []}, [], [], None
    for cc, at, size in _chunks(buf, 12, 8 + riff_size):
        if cc == b"LIST" and buf[at:at + 4] == b"hdrl":
            for c2, a2, s2 in _chunks(buf, at + 4, at + size):
                if c2 == b"avih":
                    us, bps, _, _, n, _, _, _, w, h = struct.unpack_from("<10I", buf, a2)
                    info.update(width=w, height=h, frames=n, max_bytes_per_sec=bps, usec_per_frame=us)
                elif c2 == b"LIST" and buf[a2:a2 + 4] == b"strl":
                    for c3, a3, s3 in _chunks(buf, a2 + 4, a2 + s2):
                        if c3 == b"strh":
                            typ, handler = buf[a3:a3 + 4], buf[a3 + 4:a3 + 8]
                            scale, rate, _, length = struct.unpack_from("<4I", buf, a3 + 20)
                            info.update(stream_type=typ, handler=handler, fps=rate / scale, stream_frames=length)
                        elif c3 == b"strf":
                            _, bw, bh, _, bits, comp = struct.unpack_from("<IiiHH4s", buf, a3)
                            info.update(compression=comp, bit_count=bits, bitmap_size=(bw, bh))
        elif cc == b"LIST" and buf[at:at + 4] == b"movi":
            movi = at
            for c2, a2, s2 in _chunks(buf, at + 4, at + size):
                if c2 == b"00dc":
                    offsets.append(a2 - 8)
                    frames.append(bytes(buf[a2:a2 + s2]))
        elif cc == b"idx1":
            if movi is None:
                raise ValueError(f"{path}: idx1 in front of movi")
            for i in range(size // 16):
                _, _, off, sz = struct.unpack_from("<4sIII", buf, at + 16 * i)
                info["index"].append((movi + off, sz))
    if "width" not in info or movi is None:
        raise ValueError(f"{path}: no avih header or no movi list")
    info["chunk_offsets"] = offsets
    return info, frames


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Show an MJPEG AVI's header, or write its frames out as JPEG files")
    ap.add_argument("file")
    ap.add_argument("--extract", metavar="DIR", default=None, help="write the frames as DIR/frame_{f}.jpg")
    args = ap.parse_args(argv)
    info, frames = read_avi(args.file)
    print(f"{args.file}: {info['width']} x {info['height']}, {len(frames)} frames at {info['fps']:g} fps, {sum(map(len, frames))} bytes of "
          f"{info['handler'].decode(errors='replace')}")
    if args.extract:
        os.makedirs(args.extract, exist_ok=True)
        for f, data in enumerate(frames):
            with open(os.path.join(args.extract, f"frame_{f}.jpg"), "wb") as fh:
                fh.write(data)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
