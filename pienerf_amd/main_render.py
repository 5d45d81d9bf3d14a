"""Headless simulate-and-render front end: what ``main_gui.py`` does with the window closed and ``main_render.py``
does for one frame — load a point cloud and a checkpoint, step the simulator, render every frame, write PNGs (and optionally the
deformed point cloud and the per-frame IP state the reference's ``main_render.py`` reads back from ``./debug``).

    python -m pienerf_amd.main_render --frames 30 --out output_img/chair [--ply model/chair_0.ply] [--ckpt ws/checkpoints/ngp_ep0300.pth]
           [--W 800 --H 800] [--radius 5 --azimuth 0 --elevation 0 --fovy 50] [--force fx fy fz | --drag X0 Y0 X1 Y1] [--pin_shake AX AY AZ HZ] [--pin_twist NX NY NZ DEG HZ [--pin_centre X Y Z]] [--save_ply] [--save_ip_state]
           [--floor Y] [--collide_sphere CX CY CZ R]... [--collide_inside CX CY CZ R] [--collide_box CX CY CZ HX HY HZ]...
           [--collide_capsule AX AY AZ BX BY BZ R]... [--contact_stiffness 0.5 --contact_damping 0.5 --friction 0.5
           --contact_thickness DX/2] [--unpin] [--ball CX CY CZ R MASS [VX VY VZ]]... [--ball_damping C]
           [--collide_mesh PLY [DX DY DZ]]... [--mesh_collider_res 64]
           [--wind WX WY WZ [--wind_drag 2] [--gust G HZ] [--gust_wave KX KY KZ]] [--air_drag C] [--vortex PX PY PZ NX NY NZ OMEGA RADIUS]...
           [--blast CX CY CZ STRENGTH RADIUS T0 T1]...
           [--self_contact [--self_thickness H] [--self_exclusion R] [--self_stiffness 0.5] [--self_damping 0.5] [--self_friction 0]]
           [--draw_colliders [--collider_color R G B]... [--checker S]
           [--shadows [--light X Y Z] [--shadow_strength 0.6] [--shadow_res 256]]]
           [--draw_points [--point_radius 1] [--point_color R G B] [--point_mode flat|strain|volume] [--point_range LO HI] [--point_xray]
           [--point_alpha 1] [--point_hidden_alpha 0] [--no_drag_marker]]
           [--save_mesh [--mesh_resolution 128] [--mesh_threshold 10] [--mesh_con 0] [--mesh_normals] [--mesh_color]]
           [--video [PATH] [--fps 30] [--video_quality 90] [--video_subsampling 420|444] [--no_png]]
           [--diagnostics [CSV]] [--until_rest KE]

Without --ply / --ckpt the synthetic chair of pienerf_amd.scene is used (there are no assets on the GPU box).
--save_mesh writes the deforming surface: the model's density level set, meshed once at rest, bound to the simulator (Simulator.bind_points) and warped
by its GMLS field before every frame's substep, as OUT/mesh_{f}.ply with the same triangles in every file — mesh f shows the state img_f.png shows.
--pin_shake / --pin_twist move the pinned points of the cloud (Simulator.enable_pin_motion): a sinusoidal translation with amplitude (AX, AY, AZ) at HZ,
a rotation about the axis (NX, NY, NZ) through --pin_centre (default: the pins' centroid) by DEG sin(2 pi HZ t) degrees; they compose with each other and
with --force / --drag, and images, --save_ply and --save_mesh follow the moving object.
--floor / --collide_sphere / --collide_inside / --collide_box / --collide_capsule give the object something to meet (Simulator.enable_contact;
DESIGN.md 4.10): a floor at height Y, solid spheres (repeatable), a container sphere the object stays inside, solid axis-aligned boxes with centre
(CX, CY, CZ) and half-extents (HX, HY, HZ) (repeatable: a table, a step, a ledge), solid capsules of radius R about the segment from (AX, AY, AZ) to
(BX, BY, BZ) (repeatable: a rod); --unpin clears every pin of the cloud, so the object can be dropped.  They compose with
--force, --drag, --pin_*, --save_ply and --save_mesh.
--collide_mesh gives it an arbitrary static shape (Simulator.add_mesh_collider; repeatable, at most 4): the closed triangle mesh in
PLY (--save_mesh's file, or python -m pienerf_amd.sdf --terrain), moved by (DX, DY, DZ), becomes a signed-distance grid with --mesh_collider_res nodes
along its longest axis, built on the device in nodes x triangles work.  It enables contact by itself; the balls ignore it and it is not drawn.
--ball adds a dynamic ball the object pushes back (Simulator.enable_bodies / add_body; repeatable): a solid sphere of radius R and mass
MASS at (CX, CY, CZ), thrown with (VX, VY, VZ) when given, slowed by --ball_damping per second; it falls under the simulator's gravity, meets the floor
and the other colliders, and --draw_colliders / --shadows draw it where it is.  It enables contact by itself and composes with every other flag.
--wind / --air_drag / --vortex / --blast put force fields on the whole body (Simulator.enable_fields): a wind of velocity (WX, WY, WZ)
that drags the object along at --wind_drag per second, gusting by --gust G HZ (and travelling through space with --gust_wave); still air that damps it
at --air_drag per second; vortices (repeatable) and blasts with a time window (repeatable).  They compose with everything else.
--self_contact keeps the body out of itself and lets the separate pieces of one cloud collide (Simulator.enable_self_contact): integration
points closer than --self_thickness (default sim_dx) that were at least --self_exclusion apart at rest (default 3 x the thickness) repel each other.  It
composes with every other flag.
--draw_colliders draws those colliders into every frame (SimRenderHarness.draw_colliders): a shaded floor with a checker pattern of
--checker world units (default 2 sim_dx; 0: none), shaded spheres and capsules and boxes whose faces carry the checker, depth-tested against the object; --collider_color (repeatable) colours them in slot order
(the floor first, then the spheres, the container, the boxes, the capsules, then the balls).  It composes with --bg_radius, --force, --drag, --pin_*, --save_ply and --save_mesh.
--shadows lets the object (and the solid spheres, boxes and capsules) cast a shadow onto the drawn colliders (SimRenderHarness.cast_shadows): a directional
light from --light (a vector from the scene towards the light, default 0.4 1 0.3), darkening by --shadow_strength at most, through an opacity map of
--shadow_res texels per side rendered from the light every frame.
--draw_points paints the simulator's integration points into every frame (SimRenderHarness.draw_points), the reference's "render IPs"
checkbox: discs of --point_radius pixels in --point_color, or coloured by --point_mode strain (|1/2 (F^T F - I)|) or volume (det F - 1) over --point_range,
hidden behind the object and the drawn colliders unless --point_xray (--point_hidden_alpha > 0 shows the hidden ones faintly); with --drag the dragged
point and the cursor get the reference's red and blue discs and the line between them (--no_drag_marker: not).  It composes with --drag, --force,
--pin_*, --floor, --draw_colliders, --shadows, --bg_radius and --save_*.
--video writes the run as one MJPEG AVI (pienerf_amd/video.py; default OUT/video.avi) that any player opens: every frame is encoded as a
baseline JPEG on the device, from the tensor the step returns, and only the finished bitstream crosses to the host; frame f of the video is the JPEG of
img_f.png's pixels.  --no_png leaves the PNGs out, and then the fp32 image is not copied to the host at all.  It composes with every other flag (the
overlays are part of the image).  python -m pienerf_amd.video OUT/video.avi --extract DIR writes the frames out as .jpg files.
--diagnostics measures every frame's state on the device (Simulator.record_diagnostics; default CSV: OUT/diagnostics.csv): mass, centre of
mass, momenta, kinetic / gravitational / elastic energy, the extrema of the singular values, det F, strain and speed with their integration points, and the
counts of non-finite and inverted points.  Row f is recorded immediately before frame f's step — the state img_f.png shows — with no synchronisation in
the loop; one read after it writes the CSV and reports the first frame with a non-finite or inverted point.  --until_rest KE stops the run after the
first frame whose kinetic energy is below KE (one 8-byte host read per frame) and implies --diagnostics.  They compose with every other flag.
Without --ckpt a --save_mesh run renders and meshes the SHAPED synthetic checkpoint (its density field has the solid's shape; the plain one's does not).
Reference: main_gui.py:20-66 (model + simulator construction), nerf/gui.py:556-645 (test_step: IP info -> substep -> render),
main_render.py:47-104 (frame loop, save_image), simulator/solver.py:109-113 (OutputToPly).
"""
import argparse
import os
import time

import numpy as np
import torch

from . import io, scene
from .harness import SimRenderHarness


def build_harness(args):
    opt = scene.default_opt(W=args.W, H=args.H, radius=args.radius, fovy=args.fovy, sim_dx=args.sim_dx, sim_iters=args.sim_iters,
                            max_iter_num=args.max_iter_num, num_seek_IP=args.num_seek_IP, bound=args.bound, dt_gamma=args.dt_gamma,
                            max_steps=args.max_steps, T_thresh=args.T_thresh, bg_radius=args.bg_radius)
    # the simulator's kernel grid and global solve: keys the harness reads with their defaults, not part of scene.default_opt
    opt.update(sim_kres=getattr(args, "sim_kres", 7), sim_solver=getattr(args, "sim_solver", "dense"), pcg_tol=getattr(args, "pcg_tol", 1e-10),
               pcg_max_iters=getattr(args, "pcg_max_iters", 576))
    cloud = scene.cloud_from_ply(args.ply) if args.ply else None
    if args.unpin:   # every pin of the loaded cloud cleared: nothing holds the object (drop it onto --floor)
        cloud = dict(cloud if cloud is not None else scene.make_chair_points(hgs=opt["hash_grid_size"], bound=opt["bound"]))
        cloud["pin"] = np.zeros_like(np.asarray(cloud["pin"]))
    ckpt = None
    if args.save_mesh and not args.ckpt:   # a density field with the solid's shape, as python -m pienerf_amd.mesh uses: the plain synthetic field has no surface
        ckpt = scene.make_checkpoint(bound=args.bound, shaped=True, bg_radius=args.bg_radius)
    h = SimRenderHarness(opt, cloud=cloud, ckpt=ckpt, device=args.device)
    if args.ckpt:
        path = args.ckpt if os.path.isfile(args.ckpt) else io.latest_checkpoint(args.ckpt)
        if path is None:
            raise FileNotFoundError(f"no checkpoint under {args.ckpt}")
        io.load_checkpoint(h.model, path, model_only=True, allow_pickle=args.trust_ckpt)
    return h


def bind_rest_mesh(h, args):
    """The rest mesh of the harness's model (extract_geometry over aabb_infer) bound to its simulator: (binding, triangles, colors or None)."""
    from .mesh import density_query, vertex_colors, vertex_normals
    from .nerf.utils import extract_geometry
    m = h.model
    vertices, triangles = extract_geometry(m.aabb_infer[:3], m.aabb_infer[3:], args.mesh_resolution, args.mesh_threshold, density_query(m),
                                           components=args.mesh_con)
    if len(vertices) == 0:
        raise SystemExit(f"--save_mesh: the density field has no level set at --mesh_threshold {args.mesh_threshold}")
    normals = vertex_normals(vertices, triangles) if (args.mesh_normals or args.mesh_color) else None
    colors = vertex_colors(m, vertices, normals) if args.mesh_color else None
    binding = h.sim.bind_points(vertices, normals if args.mesh_normals else None)
    return binding, triangles, colors


def wants_analytic_collider(args):
    return (args.floor is not None or bool(args.collide_sphere) or args.collide_inside is not None or bool(getattr(args, "collide_box", None))
            or bool(getattr(args, "collide_capsule", None)) or bool(getattr(args, "ball", None)))


def wants_contact(args):
    return wants_analytic_collider(args) or bool(getattr(args, "collide_mesh", None))


def mesh_collider_specs(args):
    """--collide_mesh / --mesh_collider_res as a list of (path, offset); SystemExit for a --collide_mesh that has not 1 or 4 values, a fifth one, an
    offset that is no number, a resolution out of range or --mesh_collider_res without --collide_mesh."""
    specs = getattr(args, "collide_mesh", None) or []
    res = getattr(args, "mesh_collider_res", None)
    if not specs:
        if res is not None:
            raise SystemExit("--mesh_collider_res needs --collide_mesh")
        return []
    if len(specs) > 4:
        raise SystemExit(f"--collide_mesh: at most 4 mesh colliders, got {len(specs)}")
    if res is not None and not 6 <= res <= 512:
        raise SystemExit(f"--mesh_collider_res: 6 .. 512 nodes along the longest axis, got {res}")
    out = []
    for m in specs:
        if len(m) not in (1, 4):
            raise SystemExit(f"--collide_mesh takes PLY [DX DY DZ]: 1 or 4 values, got {len(m)}")
        try:
            off = tuple(float(v) for v in m[1:]) if len(m) == 4 else (0.0, 0.0, 0.0)
        except ValueError:
            raise SystemExit(f"--collide_mesh: the offset DX DY DZ must be numbers, got {m[1:]!r}")
        out.append((m[0], off))
    return out


def add_mesh_colliders(sim, args):
    """Every --collide_mesh as a grid built on the simulator's device and placed with add_mesh_collider: --mesh_collider_res nodes
    (default 64) along the mesh's longest axis, the box its bounds plus two voxels plus the contact thickness.  Behind enable_contact().  Returns
    the mesh colliders' indices."""
    from . import scene
    from .sdf import SdfGrid
    ids = []
    res = getattr(args, "mesh_collider_res", None) or 64
    for path, off in mesh_collider_specs(args):
        try:
            v, t = scene.read_mesh_ply(path)
        except (OSError, ValueError) as e:
            raise SystemExit(f"--collide_mesh: {e}")
        h = float(sim._contact_params[3])
        ext = float((v.max(axis=0) - v.min(axis=0)).max()) if len(v) else 0.0
        s = (ext + 2.0 * h) / (res - 1 - 4)   # (res - 1) s = ext + 2 (2 s + h)
        grid = SdfGrid.from_mesh(v, t, spacing=s, margin=2.0 * s + h, device=sim.device)
        print(f"--collide_mesh {path}: {grid.triangles} triangles ({grid.dropped} dropped), grid {grid.res[0]} x {grid.res[1]} x {grid.res[2]}, "
              f"spacing {grid.spacing:.4g}, closedness {grid.closedness:.2e}")
        ids.append(sim.add_mesh_collider(grid, offset=off))
    return ids


def ball_specs(args):
    """--ball / --ball_damping as a list of add_body's arguments; SystemExit for a --ball that has not 5 or 8 numbers or --ball_damping without one."""
    balls = getattr(args, "ball", None) or []
    damping = getattr(args, "ball_damping", None)
    if not balls:
        if damping is not None:
            raise SystemExit("--ball_damping needs --ball")
        return []
    out = []
    for b in balls:
        if len(b) not in (5, 8):
            raise SystemExit(f"--ball takes CX CY CZ R MASS [VX VY VZ]: 5 or 8 numbers, got {len(b)}")
        out.append(dict(centre=tuple(b[:3]), radius=b[3], mass=b[4], velocity=tuple(b[5:8]) if len(b) == 8 else None,
                        damping=0.0 if damping is None else damping))
    return out


def configure_contact(sim, args):
    """--floor / --collide_sphere / --collide_inside / --collide_box / --collide_capsule and the contact parameters as calls on `sim`; returns the colliders' indices.  Nothing is called
    without a collider argument."""
    if not wants_contact(args):
        if any(v is not None for v in (args.contact_stiffness, args.contact_damping, args.friction, args.contact_thickness)):
            raise SystemExit("--contact_stiffness / --contact_damping / --friction / --contact_thickness need --floor, --collide_sphere, --collide_inside "
                             "or --ball (or --collide_box, --collide_capsule)")
        return []
    d = lambda v, dflt: dflt if v is None else v
    ids = []
    try:
        sim.enable_contact(stiffness=d(args.contact_stiffness, 0.5), damping=d(args.contact_damping, 0.5), friction=d(args.friction, 0.5),
                           thickness=args.contact_thickness)
        if args.floor is not None:
            ids.append(sim.add_plane((0.0, args.floor, 0.0), (0.0, 1.0, 0.0)))
        for c in args.collide_sphere or []:
            ids.append(sim.add_sphere(c[:3], c[3]))
        if args.collide_inside is not None:
            ids.append(sim.add_sphere(args.collide_inside[:3], args.collide_inside[3], inside=True))
        for c in getattr(args, "collide_box", None) or []:   # behind the older shapes: existing command lines keep their slots
            ids.append(sim.add_box(c[:3], c[3:6]))
        for c in getattr(args, "collide_capsule", None) or []:
            ids.append(sim.add_capsule(c[:3], c[3:6], c[6]))
        balls = ball_specs(args)
        if balls:   # behind the static colliders: --collider_color's slot order stays floor, spheres, container, boxes, capsules, then the balls
            sim.enable_bodies()
            ids.extend(sim.add_body(**b) for b in balls)
        add_mesh_colliders(sim, args)   # slots of their own (0 .. 3): not among the indices returned
    except ValueError as e:   # a parameter out of range, a radius <= 0, a mass <= 0, a ninth collider
        raise SystemExit(f"contact: {e}")
    return ids


def wants_fields(args):
    return args.wind is not None or args.air_drag is not None or bool(args.vortex) or bool(args.blast)


def configure_fields(sim, args):
    """--wind / --air_drag / --vortex / --blast as calls on `sim`, in that order; returns the fields' indices.  Nothing is called without one of them."""
    if not wants_fields(args) or args.wind is None:
        if any(v is not None for v in (args.wind_drag, args.gust, args.gust_wave)):
            raise SystemExit("fields: --wind_drag / --gust / --gust_wave belong to --wind")
        if not wants_fields(args):
            return []
    ids = []
    try:
        sim.enable_fields()
        if args.wind is not None:
            g, hz = args.gust if args.gust is not None else (0.0, 0.0)
            ids.append(sim.add_wind(args.wind, drag=2.0 if args.wind_drag is None else args.wind_drag, gust=g, hz=hz,
                                    wave=args.gust_wave if args.gust_wave is not None else (0.0, 0.0, 0.0)))
        if args.air_drag is not None:
            ids.append(sim.add_air_drag(args.air_drag))
        for v in args.vortex or []:
            ids.append(sim.add_vortex(v[0:3], v[3:6], v[6], v[7]))
        for b in args.blast or []:
            ids.append(sim.add_radial(b[0:3], b[3], b[4], start=b[5], stop=b[6]))
    except ValueError as e:   # a value out of range, a zero axis, a ninth field
        raise SystemExit(str(e) if str(e).startswith("fields: ") else f"fields: {e}")
    return ids


def check_self_contact_args(args):
    """What configure_self_contact refuses, before anything is built."""
    opts = (args.self_thickness, args.self_exclusion, args.self_stiffness, args.self_damping, args.self_friction)
    if not args.self_contact and any(v is not None for v in opts):
        raise SystemExit("--self_thickness / --self_exclusion / --self_stiffness / --self_damping / --self_friction need --self_contact")


def configure_self_contact(sim, args):
    """--self_contact and its options as one call on `sim`; nothing is called without the flag."""
    check_self_contact_args(args)
    if not args.self_contact:
        return False
    d = lambda v, dflt: dflt if v is None else v
    try:
        sim.enable_self_contact(stiffness=d(args.self_stiffness, 0.5), damping=d(args.self_damping, 0.5), friction=d(args.self_friction, 0.0),
                                thickness=args.self_thickness, exclusion=args.self_exclusion)
    except ValueError as e:   # a value out of range
        raise SystemExit(str(e))
    return True


def configure_overlay(h, args):
    """--draw_colliders / --collider_color / --checker as one call on the harness, behind configure_contact."""
    if not args.draw_colliders:
        if args.collider_color or args.checker is not None:
            raise SystemExit("--collider_color / --checker need --draw_colliders")
        return None
    if not wants_contact(args):
        raise SystemExit("--draw_colliders needs --floor, --collide_sphere, --collide_inside or --ball (or --collide_box, --collide_capsule)")
    from .colliders import collider_style
    try:
        style = collider_style(rgb=args.collider_color, types=h.sim.collider_types(), checker=2.0 * args.sim_dx if args.checker is None else args.checker)
    except ValueError as e:
        raise SystemExit(f"--draw_colliders: {e}")
    h.draw_colliders(style)
    configure_shadows(h, args)
    return style


def configure_shadows(h, args):
    """--shadows / --light / --shadow_strength / --shadow_res as one call on the harness, behind draw_colliders."""
    if not args.shadows:
        return
    d = lambda v, dflt: dflt if v is None else v
    try:
        h.cast_shadows(direction=d(args.light, (0.4, 1.0, 0.3)), strength=d(args.shadow_strength, 0.6), resolution=d(args.shadow_res, 256))
    except ValueError as e:
        raise SystemExit(f"--shadows: {e}")


def point_args_given(args):
    return (args.point_radius is not None or args.point_color is not None or args.point_mode is not None or args.point_range is not None
            or args.point_xray or args.point_alpha is not None or args.point_hidden_alpha is not None or args.no_drag_marker)


def point_style_from(args):
    """--point_* as a PointStyle; SystemExit for a value point_style refuses."""
    from .points_overlay import POINT_RGB, point_style
    d = lambda v, dflt: dflt if v is None else v
    lo, hi = args.point_range if args.point_range is not None else (None, None)
    try:
        return point_style(radius=d(args.point_radius, 1), mode=d(args.point_mode, "flat"), rgb=d(args.point_color, POINT_RGB), lo=lo, hi=hi,
                           xray=args.point_xray, alpha=d(args.point_alpha, 1.0), hidden_alpha=d(args.point_hidden_alpha, 0.0))
    except ValueError as e:
        raise SystemExit(f"--draw_points: {e}")


def configure_points(h, args):
    """--draw_points and its options as one call on the harness, behind enable_drag (the handle reads the drag state) and the colliders' overlay."""
    if not args.draw_points:
        return None
    style = point_style_from(args)
    h.draw_points(style, markers=not args.no_drag_marker)
    return style


def check_overlay_args(args):
    """What configure_overlay refuses, before anything is built."""
    mesh_collider_specs(args)
    if args.draw_colliders and wants_contact(args) and not wants_analytic_collider(args):
        raise SystemExit("--draw_colliders draws the analytic colliders (DESIGN.md 4.11): a --collide_mesh collides but is not drawn")
    if args.draw_colliders and not wants_contact(args):
        raise SystemExit("--draw_colliders needs --floor, --collide_sphere, --collide_inside or --ball (or --collide_box, --collide_capsule)")
    if not args.draw_colliders and (args.collider_color or args.checker is not None):
        raise SystemExit("--collider_color / --checker need --draw_colliders")
    if args.shadows and not args.draw_colliders:
        raise SystemExit("--shadows needs --draw_colliders")
    if not args.shadows and (args.light is not None or args.shadow_strength is not None or args.shadow_res is not None):
        raise SystemExit("--light / --shadow_strength / --shadow_res need --shadows")
    if not args.draw_points and point_args_given(args):
        raise SystemExit("--point_* / --no_drag_marker need --draw_points")
    if args.draw_points:
        point_style_from(args)


def check_video_args(args):
    """What --video and its options refuse, before anything is built."""
    if args.video is None:
        if args.no_png:
            raise SystemExit("--no_png needs --video: the run would write no frame at all")
        return
    from .video import quant_tables
    try:
        quant_tables(args.video_quality)
    except ValueError as e:
        raise SystemExit(f"--video_quality: {e}")
    if not args.fps > 0:
        raise SystemExit("--fps is positive")


def check_diagnostics_args(args):
    """What --until_rest refuses, before anything is built."""
    ke = getattr(args, "until_rest", None)
    if ke is not None and not (np.isfinite(ke) and ke > 0):
        raise SystemExit(f"--until_rest: KE is a positive finite kinetic energy, got {ke!r}")


def diagnostics_path(args):
    """Where --diagnostics writes: its argument, or OUT/diagnostics.csv; None without --diagnostics and without --until_rest."""
    if getattr(args, "diagnostics", None) is None and getattr(args, "until_rest", None) is None:
        return None
    return getattr(args, "diagnostics", None) or os.path.join(args.out, "diagnostics.csv")


def report_diagnostics(rows):
    """The line a --diagnostics run prints: the first frame with a non-finite or inverted point (or that there is none), the last frame's energies."""
    from .simulator.diagnostics import DIAG_FIELDS
    col = {n: i for i, n in enumerate(DIAG_FIELDS)}
    bad = [f for f, r in enumerate(rows) if r[col["nonfinite"]] > 0 or r[col["inverted"]] > 0]
    if bad:
        r = rows[bad[0]]
        first = f"first frame with a non-finite or inverted point: {bad[0]} ({int(r[col['nonfinite']])} non-finite, {int(r[col['inverted']])} inverted)"
    else:
        first = "no frame with a non-finite or inverted point"
    last = rows[-1]
    return f"diagnostics: {len(rows)} frames, {first}; last frame: kinetic {last[col['kinetic']]:.6g}, elastic {last[col['elastic']]:.6g}"


def video_path(args):
    """Where --video writes: its argument, or OUT/video.avi; None without --video."""
    if args.video is None:
        return None
    return args.video or os.path.join(args.out, "video.avi")


class FrameVideo:
    """The frames of a run as a video file: add(image) encodes the device tensor a step returned (JpegEncoder) and appends the JPEG (AviWriter)."""

    def __init__(self, path, W, H, fps=30, quality=90, subsampling="420", device="cuda"):
        from .video import AviWriter, JpegEncoder
        self.encoder = JpegEncoder(W, H, quality=quality, subsampling=subsampling, device=device)
        self.avi = AviWriter(path, W, H, fps)
        self.path, self.bytes = path, 0

    def add(self, image):
        data = self.encoder.encode(image)
        self.avi.add(data)
        self.bytes += len(data)
        return data

    def close(self):
        self.avi.close()


def open_video(args, device):
    """--video and its options as a FrameVideo; None without --video."""
    path = video_path(args)
    if path is None:
        return None
    return FrameVideo(path, args.W, args.H, fps=args.fps, quality=args.video_quality, subsampling=args.video_subsampling, device=device)


def run(args):
    check_video_args(args)
    check_diagnostics_args(args)
    if args.pin_centre is not None and args.pin_twist is None:
        raise SystemExit("--pin_centre is the centre of --pin_twist")
    check_overlay_args(args)
    check_self_contact_args(args)
    ball_specs(args)
    h = build_harness(args)
    pose = scene.orbit_pose(args.radius, args.azimuth, args.elevation)
    os.makedirs(args.out, exist_ok=True)
    if args.force is not None:
        vid = args.force_vid if args.force_vid >= 0 else h.sim.IP_pos.shape[0] // 2
        h.sim.update_force(vid, torch.tensor(args.force, dtype=torch.float64, device=h.device))
    if args.drag is not None:  # a scripted mouse drag (gui.py:556-586, :833-841): pick at (X0, Y0) on frame 0, the cursor moves linearly to (X1, Y1)
        if args.force is not None:
            raise SystemExit("--drag and --force both set the force: choose one")
        h.enable_drag(args.drag_scale)
        h.step(pose=pose, simulate=False)   # the frame the first pick is unprojected against (not written)
    if args.pin_shake is not None or args.pin_twist is not None:   # kinematic pins: shake the object by its base, twist it by its handle
        sh, tw = args.pin_shake, args.pin_twist
        try:
            h.sim.enable_pin_motion()
            h.sim.set_pin_motion(translate=(sh[:3], sh[3]) if sh is not None else None,
                                 rotate=(tw[:3], tw[3], tw[4], 0.0, args.pin_centre) if tw is not None else None)
        except ValueError as e:   # a cloud without pinned points, a zero axis, a non-finite value
            raise SystemExit(f"--pin_shake / --pin_twist: {e}")
    configure_contact(h.sim, args)
    configure_fields(h.sim, args)
    configure_self_contact(h.sim, args)
    configure_overlay(h, args)
    configure_points(h, args)
    if args.save_mesh:
        binding, triangles, colors = bind_rest_mesh(h, args)
        if not args.quiet:
            print(f"mesh: {binding.V} vertices, {len(triangles)} triangles; {binding.n_fallback} vertices bound through their nearest integration point")
    video = open_video(args, h.device)
    diag_csv, diag_log = diagnostics_path(args), None
    if diag_csv is not None:
        from .simulator.diagnostics import DIAG_FIELDS, DiagnosticsLog
        diag_log = DiagnosticsLog(max(args.frames, 1), h.device)
        ke_col = DIAG_FIELDS.index("kinetic")
    written, t0, done = [], time.time(), 0
    for f in range(args.frames):
        done = f + 1
        if args.drag is not None:
            x0, y0, x1, y1 = args.drag
            t = f / max(args.frames - 1, 1)
            x, y = x0 + t * (x1 - x0), y0 + t * (y1 - y0)
            if f == 0:
                vid = h.drag(x, y)
                if not args.quiet:
                    print(f"drag: picked IP {vid} at pixel ({x:.1f}, {y:.1f})")
            else:
                h.move(x, y)
        if args.save_mesh:   # BEFORE the step: a frame renders the pre-step state (harness.py), so mesh f shows what img_f.png shows
            h.synchronize()  # the previous frame's substep runs on the harness's side stream
            w = binding.warp()
            pos, nrm = w if args.mesh_normals else (w, None)
            scene.write_mesh_ply(os.path.join(args.out, f"mesh_{f}.ply"), pos.cpu().numpy(), triangles,
                                 normals=nrm.cpu().numpy() if nrm is not None else None, colors=colors)
        if diag_log is not None:   # BEFORE the step, like the mesh: row f is the state img_f.png shows; enqueued between two substeps, no synchronisation
            h.sim.record_diagnostics(diag_log)
        out = h.step(pose=pose, collect_stats=True)
        if video is not None:   # from the device tensor, before the host copy: the bitstream crosses, not the floats
            video.add(out["image"])
        if not args.no_png:
            out = h.to_host(out)
            path = os.path.join(args.out, f"img_{f}.png")
            io.save_image(out["image"], path, args.W, args.H)
            written.append(path)
        if args.save_ip_state:  # what gui.py dumps and main_render.py:90-100 reads back
            m = h.model
            for name, t in (("ip_pos", m.p_def), ("ip_F", m.IP_F), ("ip_dF", m.IP_dF)):
                np.save(os.path.join(args.out, f"{name}_{f}.npy"), t.detach().cpu().numpy())
        if args.save_ply:
            h.synchronize()
            h.sim.OutputToPly(os.path.join(args.out, f"points_{f}.ply"))
        if args.until_rest is not None:   # the one 8-byte read of the frame: row f's kinetic energy
            if h.sim._host_read(lambda: float(diag_log.rows[f, ke_col].item())) < args.until_rest:
                if not args.quiet:
                    print(f"until_rest: the kinetic energy of frame {f} is below {args.until_rest:g}: stopping")
                break
    h.synchronize()
    if diag_log is not None:
        rows = diag_log.to_numpy()   # the one read
        diag_log.write_csv(diag_csv, rows)
        if not args.quiet and len(rows):
            print(report_diagnostics(rows) + f" -> {os.path.abspath(diag_csv)}")
    if video is not None:
        video.close()
        if not args.quiet:
            print(f"video: {done} frames, {video.bytes} bytes of JPEG -> {os.path.abspath(video.path)}")
    if h.sim.contact_enabled and not args.quiet:
        print(f"contact: {h.sim.contact_count()} of {h.sim.n_IP} integration points in contact in the last substep")
    if h.sim.bodies_enabled and not args.quiet:
        for i, b in h.sim.body_state().items():
            print(f"ball {i}: centre ({b['centre'][0]:.4f}, {b['centre'][1]:.4f}, {b['centre'][2]:.4f}), speed {float(np.linalg.norm(b['velocity'])):.4f}, "
                  f"{b['clamped']} substeps clamped")
    if h.sim.self_contact_enabled and not args.quiet:
        print(f"self-contact: {h.sim.self_contact_count()} of {h.sim.n_IP} integration points in contact with the body itself in the last substep, "
              f"{h.sim.self_contact_overflows()} substeps over the bucket cap")
    if h.sim.solver == "pcg":   # printed whatever --quiet says: an unconverged solve is a result, not progress
        st = h.sim.pcg_stats()
        print(f"pcg: kres {h.sim.kres}, {h.sim.n_k} kernels ({int(h.sim.active_kernels.numel())} active), {int(h.sim.bsr_col.numel())} blocks; {st['solves']} solves, "
              f"{st['unconverged']} unconverged columns; CG iterations in the last substep: max {st['iterations_max']}, "
              f"mean {float(st['iterations'].mean()):.1f} per column (tol {h.sim.pcg_tol:g}, cap {h.sim.pcg_max_iters})")
    if not args.quiet:
        print(f"{done} frames -> {os.path.abspath(args.out)} in {time.time() - t0:.2f} s; last frame: {h.model.last_stats}")
    return written


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ply", default=None, help="simulation point cloud (x,y,z,mass,mu,lam,pin vertex properties); default: synthetic chair")
    ap.add_argument("--trust-ckpt", dest="trust_ckpt", action="store_true",
                    help="allow a checkpoint that needs arbitrary pickle globals (runs code from the file; default: tensors and plain scalars only)")
    ap.add_argument("--ckpt", default=None, help="a reference-format .pth or a checkpoints directory; default: synthetic chair checkpoint")
    ap.add_argument("--out", default="output_img/run")
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--W", type=int, default=800)
    ap.add_argument("--H", type=int, default=800)
    ap.add_argument("--radius", type=float, default=5.0)
    ap.add_argument("--azimuth", type=float, default=0.0)
    ap.add_argument("--elevation", type=float, default=0.0)
    ap.add_argument("--fovy", type=float, default=50.0)
    ap.add_argument("--bound", type=float, default=1.0)
    ap.add_argument("--bg_radius", type=float, default=-1, help="> 0: the checkpoint's background model colours each ray where it leaves the sphere of this radius")
    ap.add_argument("--dt_gamma", type=float, default=0.0)
    ap.add_argument("--max_steps", type=int, default=1024)
    ap.add_argument("--T_thresh", type=float, default=1e-2)
    ap.add_argument("--sim_dx", type=float, default=0.05)
    ap.add_argument("--sim_iters", type=int, default=10)
    ap.add_argument("--sim_kres", type=int, default=7, help="GMLS kernels per axis of the simulator's kernel grid, >= 2 (the reference: 7); beyond 7 use --sim_solver pcg")
    ap.add_argument("--sim_solver", choices=("dense", "pcg"), default="dense",
                    help="the global step: the pre-inverted dense matrix, or a block-sparse preconditioned CG solve that builds no dense matrix (DESIGN.md 4.19)")
    ap.add_argument("--pcg_tol", type=float, default=1e-10, help="--sim_solver pcg stops a column at |r| <= tol |b|")
    ap.add_argument("--pcg_max_iters", type=int, default=576, help="--sim_solver pcg: CG iterations per solve at the most")
    ap.add_argument("--max_iter_num", type=int, default=1)
    ap.add_argument("--num_seek_IP", type=int, default=3)
    ap.add_argument("--force", type=float, nargs=3, default=None, help="constant force on one IP (gui.py drag), e.g. 300 100 -200")
    ap.add_argument("--force_vid", type=int, default=-1)
    ap.add_argument("--drag", type=float, nargs=4, default=None, metavar=("X0", "Y0", "X1", "Y1"),
                    help="scripted mouse drag: pick the IP under pixel (X0, Y0) on frame 0, move the cursor linearly to (X1, Y1) over the frames")
    ap.add_argument("--drag_scale", type=float, default=1.0, help="the GUI's force_scale of the drag (mouse wheel, gui.py:857-865)")
    ap.add_argument("--pin_shake", type=float, nargs=4, default=None, metavar=("AX", "AY", "AZ", "HZ"),
                    help="move the pinned points by (AX, AY, AZ) sin(2 pi HZ t)")
    ap.add_argument("--pin_twist", type=float, nargs=5, default=None, metavar=("NX", "NY", "NZ", "DEG", "HZ"),
                    help="rotate the pinned points about the axis (NX, NY, NZ) by DEG sin(2 pi HZ t) degrees")
    ap.add_argument("--pin_centre", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="a point on --pin_twist's axis (default: the pins' centroid)")
    ap.add_argument("--floor", type=float, default=None, metavar="Y", help="a floor at height Y for the object to land on (contact, DESIGN.md 4.10)")
    ap.add_argument("--collide_sphere", type=float, nargs=4, action="append", default=None, metavar=("CX", "CY", "CZ", "R"),
                    help="a solid sphere the object collides with; repeatable")
    ap.add_argument("--collide_inside", type=float, nargs=4, default=None, metavar=("CX", "CY", "CZ", "R"), help="a container sphere the object stays inside")
    ap.add_argument("--collide_box", type=float, nargs=6, action="append", default=None, metavar=("CX", "CY", "CZ", "HX", "HY", "HZ"),
                    help="a solid axis-aligned box with centre (CX, CY, CZ) and half-extents (HX, HY, HZ) the object collides with; repeatable")
    ap.add_argument("--collide_capsule", type=float, nargs=7, action="append", default=None, metavar=("AX", "AY", "AZ", "BX", "BY", "BZ", "R"),
                    help="a solid capsule of radius R about the segment from (AX, AY, AZ) to (BX, BY, BZ) the object collides with; repeatable")
    ap.add_argument("--ball", type=float, nargs="+", action="append", default=None, metavar="N",
                    help="CX CY CZ R MASS [VX VY VZ]: a dynamic ball the object pushes back (DESIGN.md 4.17); repeatable")
    ap.add_argument("--ball_damping", type=float, default=None, metavar="C", help="linear damping of every --ball, 1/s, >= 0 (default 0)")
    ap.add_argument("--contact_stiffness", type=float, default=None, help="share of a penetration removed per substep, in (0, 1] (default 0.5)")
    ap.add_argument("--contact_damping", type=float, default=None, help="share of the approach velocity removed per substep, in [0, 1] (default 0.5)")
    ap.add_argument("--friction", type=float, default=None, help="Coulomb friction coefficient of the colliders, >= 0 (default 0.5)")
    ap.add_argument("--collide_mesh", nargs="+", action="append", default=None, metavar="PLY [DX DY DZ]",
                    help="collide with the closed triangle mesh in PLY (write_mesh_ply's layout: main_render --save_mesh, python -m pienerf_amd.sdf --terrain), "
                         "moved by DX DY DZ: a signed-distance grid built on the device (DESIGN.md 4.20); repeatable, at most 4")
    ap.add_argument("--mesh_collider_res", type=int, default=None, help="nodes of a --collide_mesh grid along the mesh's longest axis (default 64)")
    ap.add_argument("--contact_thickness", type=float, default=None, help="contact begins this far outside a collider (default: sim_dx / 2)")
    ap.add_argument("--unpin", action="store_true", help="clear every pin of the cloud: the object falls (give it a --floor or a --collide_box)")
    ap.add_argument("--wind", type=float, nargs=3, default=None, metavar=("WX", "WY", "WZ"), help="a wind of this velocity blows on the object (force fields, DESIGN.md 4.15)")
    ap.add_argument("--wind_drag", type=float, default=None, metavar="C", help="how hard --wind drags the object along, 1/s, >= 0 (default 2)")
    ap.add_argument("--gust", type=float, nargs=2, default=None, metavar=("G", "HZ"), help="--wind's velocity varies by 1 + G sin(2 pi HZ t), G in [0, 1]")
    ap.add_argument("--gust_wave", type=float, nargs=3, default=None, metavar=("KX", "KY", "KZ"), help="the gust travels through space with this wave vector (cycles per unit)")
    ap.add_argument("--air_drag", type=float, default=None, metavar="C", help="still air: mass-proportional damping of C per second, so a released object settles")
    ap.add_argument("--vortex", type=float, nargs=8, action="append", default=None, metavar=("PX", "PY", "PZ", "NX", "NY", "NZ", "OMEGA", "RADIUS"),
                    help="a vortex about the axis (NX, NY, NZ) through (PX, PY, PZ), OMEGA rad/s, nothing beyond RADIUS; repeatable")
    ap.add_argument("--blast", type=float, nargs=7, action="append", default=None, metavar=("CX", "CY", "CZ", "STRENGTH", "RADIUS", "T0", "T1"),
                    help="an acceleration of STRENGTH away from (CX, CY, CZ), nothing beyond RADIUS, while T0 <= t < T1 seconds; repeatable")
    ap.add_argument("--self_contact", action="store_true", help="the body collides with itself and with its own pieces (DESIGN.md 4.16)")
    ap.add_argument("--self_thickness", type=float, default=None, metavar="H", help="two integration points touch at this distance, > 0 (default: sim_dx)")
    ap.add_argument("--self_exclusion", type=float, default=None, metavar="R", help="points closer than this at rest never repel each other (default: 3 H)")
    ap.add_argument("--self_stiffness", type=float, default=None, metavar="K", help="share of an overlap removed per substep, in (0, 1] (default 0.5)")
    ap.add_argument("--self_damping", type=float, default=None, metavar="B", help="share of the approach velocity removed per substep, in [0, 1] (default 0.5)")
    ap.add_argument("--self_friction", type=float, default=None, metavar="MU", help="friction between the touching parts, >= 0 (default 0)")
    ap.add_argument("--draw_colliders", action="store_true", help="draw the colliders into every frame (DESIGN.md 4.11); needs --floor, --collide_sphere, --collide_inside, --collide_box, --collide_capsule or --ball")
    ap.add_argument("--collider_color", type=float, nargs=3, action="append", default=None, metavar=("R", "G", "B"),
                    help="a collider's colour, in slot order; repeatable (default: a light grey for a plane, a mid grey otherwise)")
    ap.add_argument("--checker", type=float, default=None, metavar="S", help="cell size of the floor's checker pattern (default: 2 sim_dx; 0: none)")
    ap.add_argument("--shadows", action="store_true", help="the object casts a shadow onto the drawn colliders (DESIGN.md 4.12); needs --draw_colliders")
    ap.add_argument("--light", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"), help="a vector from the scene towards the light (default: 0.4 1 0.3)")
    ap.add_argument("--shadow_strength", type=float, default=None, metavar="F", help="how dark a full shadow is, in [0, 1] (default 0.6)")
    ap.add_argument("--shadow_res", type=int, default=None, metavar="S", help="texels per side of the light's opacity map, 2 .. 4096 (default 256)")
    ap.add_argument("--draw_points", action="store_true", help="paint the simulator's integration points (and the drag handle) into every frame (DESIGN.md 4.13)")
    ap.add_argument("--point_radius", type=int, default=None, metavar="R", help="a point's footprint in pixels, 0 .. 8 (default 1)")
    ap.add_argument("--point_color", type=float, nargs=3, default=None, metavar=("R", "G", "B"), help="the points' colour in the flat mode (default: 0 0 1)")
    ap.add_argument("--point_mode", choices=("flat", "strain", "volume"), default=None, help="one colour, or a ramp over the strain norm / the volume change")
    ap.add_argument("--point_range", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="the ramp's range (default: 0 0.25 for strain, -0.25 0.25 for volume)")
    ap.add_argument("--point_xray", action="store_true", help="draw every point, also those behind the object (the reference's behaviour)")
    ap.add_argument("--point_alpha", type=float, default=None, metavar="A", help="the points' opacity, in [0, 1] (default 1)")
    ap.add_argument("--point_hidden_alpha", type=float, default=None, metavar="A", help="factor on the opacity of a hidden point, in [0, 1] (default 0: not drawn)")
    ap.add_argument("--no_drag_marker", action="store_true", help="with --drag: no red / blue discs and line on the dragged point")
    ap.add_argument("--save_ply", action="store_true")
    ap.add_argument("--save_ip_state", action="store_true")
    ap.add_argument("--save_mesh", action="store_true", help="write the deforming surface mesh of every frame as OUT/mesh_{f}.ply (rest mesh bound to the simulator, "
                    "warped in one HIP launch per frame); without --ckpt the run uses the shaped synthetic checkpoint")
    ap.add_argument("--mesh_resolution", type=int, default=128, help="lattice nodes per axis of the rest mesh")
    ap.add_argument("--mesh_threshold", type=float, default=10.0, help="density level of the surface")
    ap.add_argument("--mesh_con", type=int, default=0, help="mesh only this many largest connected components (0: everything)")
    ap.add_argument("--mesh_normals", action="store_true", help="write per-frame vertex normals (rest normals pushed forward by cof(F))")
    ap.add_argument("--mesh_color", action="store_true", help="write vertex colours, computed once at rest (the model's colour seen along -normal)")
    ap.add_argument("--video", nargs="?", const="", default=None, metavar="PATH",
                    help="write the run as an MJPEG AVI, every frame JPEG-encoded on the device (DESIGN.md 4.14); default PATH: OUT/video.avi")
    ap.add_argument("--fps", type=float, default=30, help="the video's frame rate")
    ap.add_argument("--video_quality", type=int, default=90, help="JPEG quality of the video's frames, 1 .. 100 (libjpeg's scale)")
    ap.add_argument("--video_subsampling", choices=("420", "444"), default="420", help="chroma at half resolution on both axes, or at full resolution")
    ap.add_argument("--no_png", action="store_true", help="with --video: write no img_{f}.png, and copy no fp32 image to the host")
    ap.add_argument("--diagnostics", nargs="?", const="", default=None, metavar="CSV",
                    help="measure every frame's state on the device (energies, momenta, strain extrema; DESIGN.md 4.18) and write one row per frame; "
                    "default CSV: OUT/diagnostics.csv")
    ap.add_argument("--until_rest", type=float, default=None, metavar="KE",
                    help="stop after the first frame whose kinetic energy is below KE > 0; costs one 8-byte host read per frame; implies --diagnostics")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--quiet", action="store_true")
    return ap


if __name__ == "__main__":
    run(parser().parse_args())
