"""The JPEG encoder on the device (pienerf_amd/video.py over csrc/pn_jpeg.hip) against the numpy restatement of its contract (tests/jpeg_reference.py,
itself checked against Pillow in tests/test_video_host.py): the bytes are equal, with no tolerance — the contract fixes every operation and
-ffp-contract=off makes it reachable.  Then the buffers' bounds, determinism, reuse, graph capture and main_render --video end to end."""
import ctypes
import os

import numpy as np
import pytest
import torch

import jpeg_reference as R
from pienerf_amd import _lib, video

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _frame(W, H, seed=None):
    return torch.from_numpy(R.test_image(H, W, W + H if seed is None else seed)).to(DEV)


# ---------------------------------------------------------------- byte parity
@pytest.mark.parametrize("W,H", R.PARITY_SIZES, ids=[f"{w}x{h}" for w, h in R.PARITY_SIZES])
def test_bytes_equal_the_restatement(W, H):
    img = _frame(W, H)
    for sub in R.SUBS:
        for q in R.PARITY_QUALITIES:
            enc = video.JpegEncoder(W, H, quality=q, subsampling=sub, device=DEV)
            got, (want, _) = enc.encode(img), R.reference(W, H, q, sub)
            assert enc.last_scan_bytes == len(want) - len(enc.header) - 2, (W, H, sub, q)
            if got != want:
                first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
                raise AssertionError(f"{W}x{H} {sub} q={q}: {len(got)} bytes against {len(want)}, first difference at byte {first} "
                                     f"(the header has {len(enc.header)})")
            assert R.decode(got)[0].shape == (H, W, 3)


def test_batched_image_tensor_and_refused_tensors():
    W, H = 17, 33
    enc = video.JpegEncoder(W, H, quality=50, subsampling="420", device=DEV)
    img = _frame(W, H)
    assert enc.encode(img.unsqueeze(0)) == R.reference(W, H, 50, "420")[0]   # [1, H, W, 3], as a harness step returns it
    for bad in (img.cpu(), img.double(), img[:, :-1], img.transpose(0, 1), img.half(), np.zeros((H, W, 3), np.float32)):
        with pytest.raises(ValueError):
            enc.enqueue(bad)
    with pytest.raises(ValueError):
        video.JpegEncoder(W, H, quality=0, device=DEV)
    with pytest.raises(ValueError):
        video.JpegEncoder(W, H, subsampling="422", device=DEV)


# ---------------------------------------------------------------- bounds
def test_nothing_is_written_outside_the_buffers():
    """Bytes of stream_out beyond the count may be anything; a 64-byte sentinel behind the capacity and sentinels around the work area stay untouched."""
    h = _lib.lib()
    for (W, H), sub in (((17, 33), 420), ((272, 48), 444)):
        cap, wb = int(h.pn_jpeg_stream_capacity(W, H, sub)), int(h.pn_jpeg_work_bytes(W, H, sub))
        wb16 = (wb + 15) // 16 * 16
        work = torch.full((64 + wb16 + 64,), 0xA5, dtype=torch.uint8, device=DEV)
        stream = torch.full((64 + cap + 64,), 0x5A, dtype=torch.uint8, device=DEV)
        count = torch.full((3,), 0x77777777, dtype=torch.int32, device=DEV)
        img = _frame(W, H)
        q = tuple((ctypes.c_uint8 * 64)(*t) for t in video.quant_tables(95))
        assert work.data_ptr() % 16 == 0
        _lib.check(h.pn_jpeg_encode(_lib.ptr(img), W, H, sub, q[0], q[1], ctypes.c_void_p(work.data_ptr() + 64), ctypes.c_void_p(stream.data_ptr() + 64),
                                    cap, ctypes.c_void_p(count.data_ptr() + 4), _lib.stream_ptr()), "jpeg encode")
        torch.cuda.synchronize()
        work, stream, count = work.cpu().numpy(), stream.cpu().numpy(), count.cpu().numpy()
        assert (work[:64] == 0xA5).all() and (work[64 + wb:] == 0xA5).all()
        assert (stream[:64] == 0x5A).all() and (stream[64 + cap:] == 0x5A).all()
        assert count[0] == 0x77777777 and count[2] == 0x77777777
        want, _ = R.reference(W, H, 95, str(sub))
        scan = want[len(video.jpeg_header(W, H, video.quant_tables(95), sub)):-2]
        assert count[1] == len(scan) and stream[64:64 + len(scan)].tobytes() == scan


# ---------------------------------------------------------------- determinism, reuse
def test_two_encodes_are_identical_and_an_encoder_is_reusable():
    W, H = 272, 48
    enc = video.JpegEncoder(W, H, quality=95, subsampling="420", device=DEV)
    a, b = _frame(W, H), _frame(W, H, seed=7)
    first = enc.encode(a)
    assert enc.encode(a) == first == R.reference(W, H, 95, "420")[0]
    assert enc.encode(b) == R.reference(W, H, 95, "420", 7)[0]      # another frame, longer and shorter intervals: nothing is left in the staging areas
    assert enc.encode(torch.zeros(H, W, 3, device=DEV)) == R.encode(np.zeros((H, W, 3), np.float32), 95, "420")   # the shortest scan there is
    assert enc.encode(a) == first


# ---------------------------------------------------------------- graph capture
def test_captured_launch_follows_the_image_buffer():
    W, H = 48, 64
    enc = video.JpegEncoder(W, H, quality=50, subsampling="444", device=DEV)
    buf = _frame(W, H).clone()
    enc.encode(buf)   # everything lazy (module load, pinned buffers) happens before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # one capture stream; the count's read-back (fetch) stays outside
        enc.enqueue(buf)
    buf.copy_(_frame(W, H, seed=11))
    g.replay()
    assert enc.fetch() == R.reference(W, H, 50, "444", 11)[0]
    buf.copy_(_frame(W, H))
    g.replay()
    assert enc.fetch() == R.reference(W, H, 50, "444")[0]


# ---------------------------------------------------------------- main_render --video
def test_main_render_writes_the_run_as_a_video(tmp_path, small_cloud):
    from PIL import Image
    from pienerf_amd import main_render, scene
    scene.write_ply(str(tmp_path / "chair.ply"), small_cloud)
    base = ["--ply", str(tmp_path / "chair.ply"), "--W", "48", "--H", "48", "--sim_dx", "0.1", "--sim_iters", "4", "--frames", "3", "--unpin",
            "--floor", "-0.95", "--contact_thickness", "0.1", "--draw_colliders", "--quiet", "--video"]
    files = main_render.run(main_render.parser().parse_args(base + ["--out", str(tmp_path / "both")]))
    assert [os.path.basename(f) for f in files] == [f"img_{f}.png" for f in range(3)]
    info, frames = video.read_avi(str(tmp_path / "both" / "video.avi"))
    assert (info["width"], info["height"], info["frames"], info["fps"], len(frames)) == (48, 48, 3, 30.0, 3)
    for f, data in enumerate(frames):
        assert R.decode(data)[0].shape == (48, 48, 3)
        with Image.open(files[f]) as png:
            pixels = np.asarray(png.convert("RGB"))
        assert data == R.encode_pixels(pixels, 90, "420"), f"frame {f} of the video is not the JPEG of img_{f}.png"
    assert len({bytes(f) for f in frames}) > 1   # the chair falls: the frames differ

    other = str(tmp_path / "elsewhere" / "run.avi")
    none = main_render.run(main_render.parser().parse_args(base + [other, "--no_png", "--out", str(tmp_path / "video_only")]))
    assert none == [] and not [f for f in os.listdir(tmp_path / "video_only") if f.endswith(".png")]
    assert open(other, "rb").read() == open(tmp_path / "both" / "video.avi", "rb").read()

    plain = main_render.run(main_render.parser().parse_args(base[:-1] + ["--out", str(tmp_path / "plain")]))   # without --video: the same PNGs, no AVI
    assert [open(a, "rb").read() for a in plain] == [open(b, "rb").read() for b in files]
    assert not os.path.exists(tmp_path / "plain" / "video.avi")
