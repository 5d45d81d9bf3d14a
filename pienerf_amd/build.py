"""Builds libpienerf_hip.so (hand-written HIP, gfx950 only) with hipcc.

    python -m pienerf_amd.build [--force] [--save-temps]

hipcc cross-compiles without a GPU.  The library is built in-tree (pienerf_amd/lib/) so that it
travels with the source tree; `*.so` is git-ignored.
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "lib", "obj")
LIB = os.path.join(HERE, "lib", "libpienerf_hip.so")
TEMPS = os.path.join(HERE, "..", "build", "temps")
ARCH = "gfx950"

# -fno-slp-vectorize: -O3 does not pack adjacent scalar fp32 adds / multiplies into v_pk_{add,mul,fma}_f32 on its own.  Beside MFMA chains
# (the network kernels) each packed op costs ~20 extra cycles (MI355X_MICROARCH.md, fillers beside MFMAs), and the bit-exact ray-side code
# wants the operation order of its source.  (Packed fp32 written explicitly for the march's candidate scan — quads of candidates in SoA
# form, two distances per instruction — was measured and is no faster: the padding it needs costs what the packing saves.  The network kernels' hash-grid
# phase, fenced from the MFMA layers by scheduling barriers, does use explicit v_pk_mul_f32 / v_pk_fma_f32 for the corner weights and channel sums: 2 %.)  Round 1 justified the flag with a suspected gfx950 erratum (packed VALU corrupting another wave's
# bf16 MFMA); tools/repro_pk_mfma.hip did not reproduce it (profiles/r02_repro_pk_mfma.json) and the claim is withdrawn.
COMMON = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize", "-Wall",
          "-Wno-unused-function", "-Wno-unused-variable"]
# per-translation-unit flags: the ray-side kernels round every operation once, in source order (bit-exact integer
# decisions vs the CPU oracle); the encoder/MLP and the fp64 simulator let the compiler contract to FMA.
UNITS = {
    "pn_render_ops.hip": ["-ffp-contract=off"],
    # the stand-alone ray ops: near/far and the static march share their arithmetic with pn_render_ops.hip (pn_near_far.h, pn_march_static.h), get_rays
    # with pn_train_batch.hip (pn_ray_dir.h) and sph_from_ray with pn_background.hip (pn_sph.h), bit for bit
    "pn_ray_ops.hip": ["-ffp-contract=off"],
    "pn_train_ops.hip": ["-ffp-contract=off"],
    "pn_grid_state.hip": ["-ffp-contract=off"],
    "pn_nerf_forward.hip": ["-ffp-contract=fast"],   # level table, SH forward, the fused network
    "pn_encoder_grad.hip": ["-ffp-contract=fast"],   # SH dy_dx and backward
    # the stand-alone hash-grid op, D = 2..5: forward, dy_dx, backward, total variation.  Contracts like nvcc does, so forward and dy_dx equal the
    # reference kernel's contracting build bit for bit
    "pn_grid_op.hip": ["-ffp-contract=fast"],
    "pn_background.hip": ["-ffp-contract=off"],  # shares pn_sph.h with pn_ray_ops.hip (the coordinate bit for bit) and blends with two roundings; the network tile contracts inside itself
    # NeRFRenderer.run fused + the masked colour query: the ray-side arithmetic (z, positions, deltas, alpha, the cdf's interpolation, the blend's two
    # roundings) rounds once per operation like the torch op sequence it restates (run_ops); tolerance work, so this is a choice of the closer restatement,
    # not a bit-exactness requirement.  The network tile contracts inside itself.
    "pn_hier.hip": ["-ffp-contract=off"],
    "pn_sim.hip": ["-ffp-contract=fast"],
    "pn_drag.hip": ["-ffp-contract=fast"],   # shares pn_sim_ip.h with pn_sim.hip: the same contraction, the same bits
    "pn_pins.hip": ["-ffp-contract=fast"],   # fp64 sums in a fixed order: contraction does not touch the order, only the rounding of each step
    # contact, force fields, self-contact: one source for a point's state and for the per-kernel sum (pn_sim_rhs.h, on top of pn_sim_ip.h, which
    # pn_sim.hip shares: a point's position as update_F sums it), so the three contract alike and the bits agree; fp64 sums in a fixed order
    "pn_contact.hip": ["-ffp-contract=fast"],
    "pn_fields.hip": ["-ffp-contract=fast"],
    # the rigid balls: the per-collider law (pn_contact_law.h) and a point's state (pn_sim_rhs.h) are contact's own lines, contracted alike, so slot
    # b's term at a point is the same bits on the object's side and in the ball's reaction
    "pn_bodies.hip": ["-ffp-contract=fast"],
    # mesh colliders: the grids' contact term is contact's own response (pn_contact_law.h) at pn_sim_rhs.h's point state, contracted as in the units
    # it shares them with; the builder's fp32 distances and winding terms are compared with tests/sdf_reference.py's fp64 by a measured bar
    "pn_sdf.hip": ["-ffp-contract=fast"],
    # the one decision self-contact takes in floating point (a pair's eligibility at rest) switches contraction off for itself
    "pn_selfcontact.hip": ["-ffp-contract=fast"],
    # the diagnostics readout: pn_sim_rhs.h's point state and pn_sim_svd.h's ip_F_partial / svd3, contracted as in the units it shares them with;
    # fp64 sums in fixed trees, compared with tests/diagnostics_reference.py by a derived tolerance
    "pn_diagnostics.hip": ["-ffp-contract=fast"],
    # the colliders drawn into a frame: per-ray fp32 with decisions in it (hit / miss, checker parity, in front of / behind the object), one rounding per
    # operation in source order, which tests/colliders_reference.py restates in numpy; a ray without a hit gets the frame epilogue's two roundings
    "pn_colliders.hip": ["-ffp-contract=off"],
    # the integration points and the drag handle drawn into a frame: per-point and per-pixel fp32 with decisions in it (the pixel a point falls on, in
    # front of / behind the object, inside a disc), one rounding per operation in source order, which tests/points_overlay_reference.py restates in numpy
    "pn_points_overlay.hip": ["-ffp-contract=off"],
    "pn_warp_points.hip": ["-ffp-contract=fast"],   # bound points warped by the GMLS field: pn_sim_ip.h's accumulation, contracted as in pn_sim.hip
    "pn_mesh.hip": ["-ffp-contract=off"],  # marching cubes: the vertex formula rounds as written (tests/mc_reference.py restates it bit for bit)
    # training batches: the pixel index restates separate torch ops (one rounding each), the keys of the weighted sampler are IEEE quotients, and a
    # pixel's ray is pn_ray_dir.h's, shared with pn_ray_ops.hip bit for bit
    "pn_train_batch.hip": ["-ffp-contract=off"],
    "pn_components.hip": ["-ffp-contract=off"],  # connected-component labelling: integers only, the flag has nothing to act on
    # SSIM (metrics.py): every moment is a sum of 11 products in tap order and sigma = E[xx] - mx^2 cancels, so each operation rounds once as written;
    # tests/ssim_reference.py's fp32 evaluation then has the same error size and sets the tests' tolerance
    "pn_ssim.hip": ["-ffp-contract=off"],
    # baseline JPEG of a frame (video.py): colour transform, DCT and quantisation decide integers, so every operation rounds once in source order;
    # tests/jpeg_reference.py restates them in numpy and the encoded bytes agree
    "pn_jpeg.hip": ["-ffp-contract=off"],
    "pn_copier.hip": [],  # host code only: frame copies through the HSA runtime (links libhsa-runtime64)
}


def source_hash():
    """SHA-1 over the kernel sources, headers and compile flags: identifies the code a measurement was taken on (profiles/pmc_traffic.json is
    stamped with it; bench.py refuses a stamp that does not match the tree it runs from)."""
    import hashlib
    h = hashlib.sha1()
    files = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))) 
    for f in files:
        h.update(f.encode())
        with open(os.path.join(CSRC, f), "rb") as fh:
            h.update(fh.read())
    with open(os.path.join(HERE, "..", "include", "pienerf_hip.h"), "rb") as fh:
        h.update(fh.read())
    h.update(repr((COMMON, sorted(UNITS.items()))).encode())
    return h.hexdigest()


def hipcc():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: libpienerf_hip.so cannot be built (there is no CPU fallback)")


def _stale(out, deps):
    return (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


def build(force=False, save_temps=False, verbose=False):
    os.makedirs(OBJ, exist_ok=True)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [os.path.join(HERE, "..", "include", "pienerf_hip.h"),
                                                                                     os.path.abspath(__file__)]
    cc = hipcc()
    objs = []
    for src, extra in UNITS.items():
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + headers):
            cmd = [cc] + COMMON + extra + ["-c", s, "-o", o]
            cwd = OBJ
            if save_temps:  # intermediates (.hipi/.bc/.s) go to <repo>/build/temps: git-ignored AND gpurun-ignored, never beside the objects
                cwd = TEMPS
                os.makedirs(TEMPS, exist_ok=True)
                cmd += ["-save-temps=cwd", "-Rpass-analysis=kernel-resource-usage"]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True, cwd=cwd)
    if force or _stale(LIB, objs):
        rocm = os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(cc)))  # <rocm>/bin/hipcc
        cmd = [cc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + objs + ["-L" + os.path.join(rocm, "lib"), "-lhsa-runtime64", "-lpthread"]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, save_temps="--save-temps" in sys.argv, verbose=True))
