"""numpy restatement of the point overlay's law (include/pienerf_hip.h: pn_draw_points; csrc/pn_points_overlay.hip), in fp32 operation by operation — the
launch pair is compared with it bit for bit — and a restatement of what the reference's point painting does (nerf/gui.py: overlay_point_buffer with
world_to_screen; restated here because gui.py cannot be imported without dearpygui), to compare pixel sets with.

The test inputs are built FROM pixels (``point_at``): x = o + t d(px + 1/2 + dx, py + 1/2 + dy) with |dx|, |dy| <= 0.3, so the pixel a point falls on
is beyond doubt in any rounding and no case needs excluding.
"""
import numpy as np

f32 = np.float32
EMPTY = 0xffffffffffffffff
FLAT, STRAIN, VOLUME, VALUES = 0, 1, 2, 3
MODES = {"flat": FLAT, "strain": STRAIN, "volume": VOLUME, "values": VALUES}

# the standard camera of the tests: 24 x 16 (not square: a row / column swap shows), looking at the origin from an oblique direction
W, H = 24, 16
INTR = (20.0, 20.0, 12.0, 8.0)
T_MIN = 0.2
BIAS = 0.02


def look_at(eye, target=(0.0, 0.0, 0.0)):
    """A c2w pose [4,4] float32, the camera at `eye` looking along +z at `target`, y down."""
    eye = np.asarray(eye, np.float64)
    z = np.asarray(target, np.float64) - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, [0.0, 1.0, 0.0])
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, y, z, eye
    return pose.astype(np.float32)


POSE = look_at((1.1, 0.7, -2.3))


def point_at(pose, intr, px, py, t, dx=0.0, dy=0.0):
    """The world point at distance t from the camera on the ray through (px + 1/2 + dx, py + 1/2 + dy), built in float64 and rounded to fp32 once."""
    P = np.asarray(pose, np.float64).reshape(4, 4)
    fx, fy, cx, cy = (float(v) for v in intr)
    d = np.array([(px + 0.5 + dx - cx) / fx, (py + 0.5 + dy - cy) / fy, 1.0])
    d /= np.linalg.norm(d)
    return (P[:3, 3] + t * (P[:3, :3] @ d)).astype(np.float32)


def style(radius=0, mode="flat", xray=False, rgb=(0.0, 0.0, 1.0), ramp=((0.1, 0.2, 0.9), (0.95, 0.95, 0.95), (0.9, 0.15, 0.1)), lo=0.0, hi=1.0,
          alpha=1.0, hidden_alpha=0.0, bias=BIAS, marker_radius=10.0, marker_thickness=5.0):
    return dict(radius=int(radius), mode=MODES[mode], xray=bool(xray), rgb=np.asarray(rgb, f32), ramp=np.asarray(ramp, f32), lo=f32(lo), hi=f32(hi),
                alpha=f32(alpha), hidden_alpha=f32(hidden_alpha), bias=f32(bias), marker_radius=f32(marker_radius), marker_thickness=f32(marker_thickness))


def project(pose, intr, x, dtype=np.float32):
    """The header's projection of the points x [n,3]: (u, v, t, drawable), every operation rounded once in `dtype`."""
    P = np.asarray(pose, dtype).reshape(4, 4)
    fx, fy, cx, cy = (dtype(v) for v in intr)
    x = np.asarray(x, dtype).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d0, d1, d2 = x[:, 0] - P[0, 3], x[:, 1] - P[1, 3], x[:, 2] - P[2, 3]
        xc = P[0, 0] * d0 + P[1, 0] * d1 + P[2, 0] * d2
        yc = P[0, 1] * d0 + P[1, 1] * d1 + P[2, 1] * d2
        zc = P[0, 2] * d0 + P[1, 2] * d1 + P[2, 2] * d2
        t = np.sqrt(d0 * d0 + d1 * d1 + d2 * d2)
        u = xc / zc * fx + cx
        v = yc / zc * fy + cy
        ok = np.isfinite(x).all(axis=1) & (zc > 0) & np.isfinite(t) & np.isfinite(u) & np.isfinite(v)
    return u, v, t, ok


def splat(pos, pose, intr, Wd, Hd, t_min, radius):
    """The key buffer after the splat launch, as a list of Python ints: per pixel the smallest (bits(t) << 32) | index, EMPTY where none."""
    keys = [EMPTY] * (Wd * Hd)
    pos = np.asarray(pos, f32).reshape(-1, 3)
    if pos.shape[0] == 0:
        return keys
    u, v, t, ok = project(pose, intr, pos)
    with np.errstate(all="ignore"):
        fpx, fpy = np.floor(u), np.floor(v)
        ok = ok & (t > f32(t_min)) & (fpx >= -9) & (fpx <= Wd + 8) & (fpy >= -9) & (fpy <= Hd + 8)
    r2 = radius * radius
    for i in np.nonzero(ok)[0]:
        px, py = int(fpx[i]), int(fpy[i])
        key = (int(t[i:i + 1].view(np.uint32)[0]) << 32) | int(i)
        for dy in range(-radius, radius + 1):
            y = py + dy
            if y < 0 or y >= Hd:
                continue
            for dx in range(-radius, radius + 1):
                xx = px + dx
                if xx < 0 or xx >= Wd or dx * dx + dy * dy > r2:
                    continue
                p = y * Wd + xx
                if key < keys[p]:
                    keys[p] = key
    return keys


def point_scalar(mode, F, values, i):
    if mode == VALUES:
        return f32(values[i])
    f = np.asarray(F, f32).reshape(-1, 9)[i]
    with np.errstate(all="ignore"):
        if mode == VOLUME:
            det = f[0] * (f[4] * f[8] - f[5] * f[7]) - f[1] * (f[3] * f[8] - f[5] * f[6]) + f[2] * (f[3] * f[7] - f[4] * f[6])
            return f32(det - f32(1))
        total = f32(0)
        for a in range(3):
            for b in range(3):
                C = f[a] * f[b] + f[3 + a] * f[3 + b] + f[6 + a] * f[6 + b]
                E = f32(0.5) * (C - f32(1 if a == b else 0))
                total = f32(total + E * E)
        return f32(np.sqrt(total))


def point_colour(st, F, values, i):
    if st["mode"] == FLAT:
        return st["rgb"].copy()
    with np.errstate(all="ignore"):
        v = point_scalar(st["mode"], F, values, i)
        u = np.fmin(np.fmax((v - st["lo"]) / (st["hi"] - st["lo"]), f32(0)), f32(1))
        if u < f32(0.5):
            w, r0, r1 = u * f32(2), st["ramp"][0], st["ramp"][1]
        else:
            w, r0, r1 = (u - f32(0.5)) * f32(2), st["ramp"][1], st["ramp"][2]
        return (r0 + w * (r1 - r0)).astype(f32)


def draw(pos, F, values, pose, intr, Wd, Hd, t_min, weights_sum, depth_0, collider_t, drag, st, image):
    """The law: returns (image [W H,3], point_id [W H] int32, point_t [W H]); nothing in place.  `drag`: None or dict(vid, active, target[3] float64).
    Pixels the law leaves alone keep the bits of `image`."""
    N = Wd * Hd
    out = np.array(image, f32).reshape(N, 3).copy()
    pid = np.full(N, -1, np.int32)
    pt = np.full(N, np.inf, f32)
    pos = np.asarray(pos, f32).reshape(-1, 3)
    n = pos.shape[0]
    keys = splat(pos, pose, intr, Wd, Hd, t_min, st["radius"])
    s_all, d_all = np.asarray(weights_sum, f32).reshape(N), np.asarray(depth_0, f32).reshape(N)
    ct = None if collider_t is None else np.asarray(collider_t, f32).reshape(N)
    one = f32(1)
    with np.errstate(all="ignore"):
        for p in range(N):
            key = keys[p]
            if key == EMPTY:
                continue
            i = key & 0xffffffff
            t = np.array([key >> 32], np.uint32).view(f32)[0]
            s = s_all[p]
            t_obj = d_all[p] / s if s > f32(1e-4) else f32(np.inf)
            t_front = np.fmin(t_obj, ct[p]) if ct is not None else t_obj
            visible = st["xray"] or bool(t <= f32(t_front + st["bias"]))
            if not visible and st["hidden_alpha"] == 0:
                continue
            a = st["alpha"] if visible else f32(st["alpha"] * st["hidden_alpha"])
            c = point_colour(st, F, values, i)
            out[p] = a * c + (one - a) * out[p]
            pid[p], pt[p] = i, t
        if drag is not None and drag["active"]:
            vid = int(drag["vid"])
            a_ok = b_ok = False
            if 0 <= vid < n:
                au, av, _, ok = project(pose, intr, pos[vid])
                a_ok, ax, ay = bool(ok[0]), au[0], av[0]
            bu, bv, _, ok = project(pose, intr, np.asarray(drag["target"], np.float64).astype(f32))
            b_ok, bx, by = bool(ok[0]), bu[0], bv[0]
            idx = np.arange(N)
            qx, qy = (idx % Wd).astype(f32) + f32(0.5), (idx // Wd).astype(f32) + f32(0.5)
            rr = st["marker_radius"] * st["marker_radius"]
            if a_ok:
                dx, dy = qx - ax, qy - ay
                out[dx * dx + dy * dy <= rr] = (1.0, 0.0, 0.0)
            if b_ok:
                dx, dy = qx - bx, qy - by
                out[dx * dx + dy * dy <= rr] = (0.0, 0.0, 1.0)
            if a_ok and b_ok:
                ex, ey = bx - ax, by - ay
                dx, dy = qx - ax, qy - ay
                L2 = ex * ex + ey * ey
                h = np.fmin(np.fmax((dx * ex + dy * ey) / L2, f32(0)), one) if L2 > 0 else np.zeros(N, f32)
                gx, gy = dx - h * ex, dy - h * ey
                half = f32(0.5) * st["marker_thickness"]
                m = gx * gx + gy * gy <= half * half
                keep = one - f32(100) / f32(255)
                out[m] = keep * out[m]
    return out, pid, pt


def reference_pixels(points, pose, intr, rows, cols):
    """What the reference's point painting does to a buffer of `rows` x `cols` pixels, as the set of (row, column) it paints blue: every point goes through
    the inverse of the pose in float64, is divided by its camera z and scaled by the intrinsics, both screen coordinates are truncated with int(), and the
    buffer is indexed [int(y screen), int(x screen)] (the reference swaps the pair twice) when that lies inside it.  No test of the sign of z."""
    inv = np.linalg.inv(np.asarray(pose, np.float64).reshape(4, 4))
    fx, fy, cx, cy = (float(v) for v in intr)
    painted = set()
    for x in np.asarray(points, np.float64).reshape(-1, 3):
        cam = inv @ np.array([x[0], x[1], x[2], 1.0])
        xs, ys = cam[0] / cam[2] * fx + cx, cam[1] / cam[2] * fy + cy
        row, col = int(ys), int(xs)
        if 0 <= row < rows and 0 <= col < cols:
            painted.add((row, col))
    return painted


# ---------------------------------------------------------------- shared test inputs
def frame_inputs(Wd=W, Hd=H, seed=5):
    """A frame to paint onto: image [N,3] in (0, 1), weights_sum with exact zeros and ones and values between, depth_0 = weights_sum t_obj with t_obj one of
    2 and 3 — and a collider_t of 2.5 on a third of the pixels, +inf elsewhere.  So t_front + BIAS is one of 2.02, 2.52, 3.02 or +inf."""
    rng = np.random.default_rng(seed)
    N = Wd * Hd
    image = rng.uniform(0.05, 0.95, (N, 3)).astype(f32)
    s = rng.uniform(0.2, 0.95, N).astype(f32)
    kind = rng.integers(0, 4, N)
    s[kind == 0] = 0.0
    s[kind == 1] = 1.0
    t_obj = np.where(rng.integers(0, 2, N) == 0, 2.0, 3.0).astype(f32)
    d0 = (s * t_obj).astype(f32)
    ct = np.where(rng.integers(0, 3, N) == 0, 2.5, np.inf).astype(f32)
    return image, s, d0, ct


THRESHOLDS = (2.02, 2.52, 3.02)


def t_ladder(count, first=1.2, last=3.8, margin=0.012):
    """`count` distances from `first` to about `last` — on both sides of every threshold — each at least 1.004 (> 1 + 1e-3) times the one before, none
    within `margin` (> 1e-2) of a depth-test threshold."""
    ratio = max(1.004, (last / first) ** (1.0 / max(count, 1)))
    out, t = [], first
    while len(out) < count:
        if all(abs(t - th) > margin for th in THRESHOLDS):
            out.append(t)
        t *= ratio
    return out


def cloud(n, seed=1, pose=POSE, intr=INTR, Wd=W, Hd=H, borders=True, rejects=True, duplicates=True):
    """`n` drawable points on random pixels of the image at the ladder's distances, then (borders) points on each border and in a corner, so that discs of
    radius 2 and 8 are cut there, (duplicates) exact copies of two points under higher indices, and (rejects) points the law drops: behind the camera,
    nearer than t_min, off-screen, non-finite.  Returns pos [m,3] fp32."""
    rng = np.random.default_rng(seed)
    extra = [(0, 5), (Wd - 1, 7), (9, 0), (11, Hd - 1), (0, 0), (Wd - 1, Hd - 1)] if borders else []
    ts = t_ladder(n + len(extra))
    rng.shuffle(ts)
    pts = []
    for k in range(n):
        px, py = int(rng.integers(0, Wd)), int(rng.integers(0, Hd))
        pts.append(point_at(pose, intr, px, py, ts[k], *rng.uniform(-0.3, 0.3, 2)))
    for k, (px, py) in enumerate(extra):
        pts.append(point_at(pose, intr, px, py, ts[n + k], *rng.uniform(-0.3, 0.3, 2)))
    if duplicates and n >= 2:
        pts += [pts[1].copy(), pts[0].copy()]
    if rejects:
        pts.append(point_at(pose, intr, 7, 7, -1.7))                      # behind the camera: the reference would mirror it onto the picture
        pts.append(point_at(pose, intr, 8, 3, 0.5 * T_MIN))               # nearer than t_min
        pts.append(point_at(pose, intr, -5, 3, 1.9))                      # off-screen to the left
        pts.append(point_at(pose, intr, Wd + 3, Hd + 4, 2.2))             # ... and past the far corner
        pts.append(point_at(pose, intr, -1, -1, 2.3, 0.2, 0.2))           # u, v in (-1, 0): the reference's int() puts it on the border, floor does not
        pts.append(np.array([np.nan, 0.0, 0.0], f32))
        pts.append(np.array([0.1, np.inf, 0.0], f32))
    return np.stack(pts).astype(f32)


def gradients(n, seed=2):
    """F [n,9] fp32: rotations times (I + eps A), eps = 0.01 for even points (near a rotation) and 0.5 for odd ones (far from one)."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, 9), f32)
    for i in range(n):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        eps = 0.01 if i % 2 == 0 else 0.5
        out[i] = (q @ (np.eye(3) + eps * rng.uniform(-1, 1, (3, 3)))).reshape(9)
    return out
