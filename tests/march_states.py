"""Named integration-point (IP) states for the ray march: bodies far rougher than the `deformed_ip_state` fixture every render test used
to march through (fullest hash cell 6 IPs, longest 27-cell candidate list 40 entries, every F well conditioned, no sample on an IP, no two
IPs in one place).  numpy + the CPU oracle only; a helper module, not a conftest.

Every builder takes the `deformed_ip_state` dict and the option dict and returns `(state, facts)`:
  state   a new dict with the same keys (p_def, p_ori, F, dF, IP_dx) plus `hash_grid_size`, every array finite float32;
  facts   what makes the state adversarial, measured with oracle.render_bbox / oracle.get_pnts_in_grids — `check_facts` asserts them, so a
          state that silently stops being adversarial fails its tests.

The paths of pienerf_amd/csrc/pn_march_window.h and pn_march_tables.h each state is there for:
  crowded     stage_lists<768>: candidate lists over the cap (the lanes of such a cell scan global memory beside lanes that scan LDS, and
              head_fetch then reuses the same LDS), lists of 256 .. 768 where the second or third distinct list of a wave overflows;
              k_frame_tables' one-thread insertion sort with > 100 entries per cell; and, the three copies being exact duplicates, an exact
              distance tie at EVERY sample: eval_scan's 64-bit keys must break it by list position as the sequential strict '<' does
  sparse      eval_scan<1>'s second loop (own cell empty, neighbours not), eval_scan<2,3> with fewer than K candidates (sentinel keys)
  singular    pack_ip_float with det F == 0 (F^-1 = 0: the sample maps to p_ori), rank 1 / rank 2 F, inverted F (det < 0)
  squashed    the body pressed flat against the floor: cells three times as full at the default hash cell size
  twisted     warp_record<true> where Newton really needs iterations 2 .. 5 and where the |p - p_ori| > IP_dx test rejects some of a sample's
              K warps but not others (n_IP shrinks, the 1 / 2 / 3-IP blends alternate)
  coincident  (op level) samples that lie ON an IP bit for bit: d == 0, two IPs at d == 0, and an IP at d^2 = 2^-140 (a float denormal) beside
              one at d == 0 — the keys of eval_scan are then denormal doubles
"""
import numpy as np

import oracle
from pienerf_amd import scene

NAMES = ("crowded", "sparse", "singular", "squashed", "twisted")   # the states a whole frame can be rendered from (`coincident` is op level only)
CAMERA = dict(radius=5.0, az=25.0, el=-15.0, fovy=50.0, W=48)       # the test camera of the op-level march tests
STAGE_CAP = 768                                                     # PN_STAGE_CAP (pn_march_window.h)
TWIST = 100.0                                                       # see twisted()


# ------------------------------------------------------------------------------------------------ measuring a state
def cell_table(p_def, hgs):
    """The spatial hash of p_def at cell size hgs (no --cut), the own-cell count and the 27-cell candidate list length of every cell."""
    hgs = np.float32(hgs)
    bbmin, bbmax, res = oracle.render_bbox(p_def, hgs)
    n_grid = int(res.prod())
    pig = oracle.get_pnts_in_grids(len(p_def), n_grid, p_def, bbmin, bbmax, hgs, res)
    own = pig[0].reshape(res[2], res[1], res[0]).astype(np.int64)
    pad = np.pad(own, 1)
    lists = np.zeros_like(own)
    for a in range(3):
        for b in range(3):
            for c in range(3):
                lists += pad[a:a + res[2], b:b + res[1], c:c + res[0]]
    return dict(hgs=hgs, bbmin=bbmin, bbmax=bbmax, res=res, n_grid=n_grid, pig=pig, own=own, lists=lists)


def march_inputs(state, W=CAMERA["W"], az=CAMERA["az"], el=CAMERA["el"]):
    """The rays of the test camera and the spatial hash of `state` — what the op-level march takes (test_gpu_parity._march_inputs, with the
    state's own hash cell size)."""
    o, d = oracle.get_rays(scene.orbit_pose(CAMERA["radius"], az, el), scene.orbit_intrinsics(W, W, CAMERA["fovy"]), W, W)
    t = cell_table(state["p_def"], state["hash_grid_size"])
    nears, fars = oracle.near_far_from_aabb(o, d, np.concatenate([t["bbmin"], t["bbmax"]]), 0.2)
    return dict(o=o, d=d, hgs=t["hgs"], bbmin=t["bbmin"], bbmax=t["bbmax"], res=t["res"], n_grid=t["n_grid"], pig=t["pig"], nears=nears, fars=fars)


def ray_points(m, max_steps=1024):
    """Every alive ray of `m` stepped from near to far at the march's fixed dt: the clamped points [n, 3] (raymarching.cu:1190-1200) and their
    cell coordinates [n, 3] as point_cell takes them."""
    alive = np.nonzero(m["nears"] < 1e30)[0]
    dt = np.float32(2 * 1.7320508075688772 / max_steps)
    n_max = int(np.ceil((m["fars"][alive] - m["nears"][alive]).max() / dt)) + 1
    t = np.cumsum(np.concatenate([m["nears"][alive][:, None], np.full((len(alive), n_max), dt, np.float32)], 1), axis=1, dtype=np.float32)
    keep = t < m["fars"][alive][:, None]
    ray = np.broadcast_to(alive[:, None], t.shape)[keep]
    x = m["o"][ray] + t[keep][:, None] * m["d"][ray]
    hi = (m["bbmax"].astype(np.float64) - 1e-6).astype(np.float32)
    x = np.minimum(np.maximum(x, m["bbmin"]), hi).astype(np.float32)
    g = np.floor((x - m["bbmin"]) / m["hgs"]).astype(np.int64)
    assert (g >= 0).all() and (g < m["res"]).all()
    return x, g


def det_f32(F):
    """det F per IP in float32, in the expression order of pnm::inv3x3 (one rounding per operation)."""
    A = [np.ascontiguousarray(F[:, j], np.float32) for j in range(9)]
    return A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6])


def occupied(ckpt, pts):
    """The density bit of the voxel each point lies in (one cascade: level 0), as the march looks it up."""
    assert ckpt["cascade"] == 1
    H = int(ckpt["grid_size"])
    n = np.clip(((np.asarray(pts, np.float32) / np.float32(ckpt["bound"]) + 1) * np.float32(0.5 * H)), 0, H - 1).astype(np.int32)
    vox = np.asarray(oracle.morton3D(n)).astype(np.int64)
    return (ckpt["density_bitfield"][vox // 8] >> (vox % 8)) & 1 != 0


def _copy(base, opt, **over):
    s = {k: np.array(base[k], np.float32, copy=True) for k in ("p_def", "p_ori", "F", "dF")}
    s["IP_dx"] = base["IP_dx"]
    s["hash_grid_size"] = float(opt["hash_grid_size"])
    s.update(over)
    return s


def _grid_facts(state):
    t = cell_table(state["p_def"], state["hash_grid_size"])
    return t, dict(n_IP=len(state["p_def"]), own_max=int(t["own"].max()), list_max=int(t["lists"].max()))


# ------------------------------------------------------------------------------------------------ the states
def crowded(base, opt):
    """The state three times over: duplicates under the ids i, i + n, i + 2n, in hash cells of 3.6 sim_dx.  Measured on the small chair:
    longest list 1080, 5 cells above 768, 24 cells in (256, 768], fullest cell 120.
    p_def, F and dF of the copies are exact duplicates, so every sample sees exact distance ties between them.  Their rest positions are not:
    copy k has p_ori.x moved by k 2^-9 (a fraction of a density voxel).  Were the copies the same in everything, whichever of them won a tie
    would give the same sample and a wrong tie-break could not show; as it is, two IPs sought must take copies 0 and 1, in that order."""
    s = _copy(base, opt, hash_grid_size=3.6 * float(opt["sim_dx"]))
    n = len(s["p_def"])
    for k in ("p_def", "p_ori", "F", "dF"):
        s[k] = np.ascontiguousarray(np.concatenate([s[k]] * 3, 0))
    s["p_ori"][:, 0] += np.repeat(np.arange(3, dtype=np.float32), n) * np.float32(2.0 ** -9)
    t, facts = _grid_facts(s)
    over = t["lists"] > STAGE_CAP
    x, g = ray_points(march_inputs(s))
    same = lambda k: all(np.array_equal(s[k][:n], s[k][c * n:(c + 1) * n]) for c in (1, 2))
    facts.update(cells_over_cap=int(over.sum()), cells_in_256_cap=int(((t["lists"] > 256) & ~over).sum()),
                 ray_points_in_cells_over_cap=int(over[g[:, 2], g[:, 1], g[:, 0]].sum()),
                 copies_tie=bool(same("p_def") and same("F") and same("dF")), p_ori_distinct=int(len(np.unique(s["p_ori"], axis=0))))
    return s, facts


def sparse(base, opt):
    """Every 7th IP only: most cells are empty beside occupied ones, lists of one and two entries exist."""
    s = _copy(base, opt)
    for k in ("p_def", "p_ori", "F", "dF"):
        s[k] = np.ascontiguousarray(s[k][::7])
    t, facts = _grid_facts(s)
    facts.update(cells_own0_list_pos=int(((t["own"] == 0) & (t["lists"] > 0)).sum()), cells_list1=int((t["lists"] == 1).sum()),
                 cells_list2=int((t["lists"] == 2).sum()))
    return s, facts


def singular(base, opt):
    """A fixed permutation picks four eighths of the IPs: F = 0; F with its third column zeroed (rank 2); an outer-product F (rank 1, with dyadic
    factors so that every product in det F is exact and the float32 determinant is exactly 0); F with its third column negated (det < 0).  The
    other half keeps its F.  (Column c of F is F[3c .. 3c + 3): mul31 reads F[c * 3 + r].)"""
    s = _copy(base, opt)
    n = len(s["F"])
    rng = np.random.default_rng(11)
    perm = rng.permutation(n)
    e = n // 8
    zero, rank2, rank1, flip = (perm[i * e:(i + 1) * e] for i in range(4))
    F = s["F"].reshape(n, 3, 3)    # [ip, column, row]
    det_before = det_f32(s["F"])
    F[zero] = 0
    F[rank2, 2, :] = 0
    u = (rng.integers(1, 7, (e, 3)) * rng.choice([-1, 1], (e, 3)) / 4).astype(np.float32)
    v = (rng.integers(1, 7, (e, 3)) * rng.choice([-1, 1], (e, 3)) / 4).astype(np.float32)
    F[rank1] = v[:, :, None] * u[:, None, :]
    F[flip, 2, :] = -F[flip, 2, :]
    s["F"] = np.ascontiguousarray(F.reshape(n, 9))
    _, facts = _grid_facts(s)
    det = det_f32(s["F"])
    facts.update(det_zero=int((det == 0).sum()), det_negative=int((det < 0).sum()), want_det_zero=3 * e,
                 want_det_negative=e + int((det_before[np.setdiff1d(np.arange(n), perm[:4 * e])] < 0).sum()))
    return s, facts


def squashed(base, opt):
    """The lower half of the body (p_def.y below the median y0) pressed flat against the plane y = y0: y -> y0 + 0.02 (y - y0), the second row of F
    (F[c * 3 + 1]) scaled by 0.02 with it.  The hash cell size stays the default one.  Measured on the small chair: fullest cell 18 against 6."""
    s = _copy(base, opt)
    y = s["p_def"][:, 1].copy()
    y0 = np.float32(np.median(y))
    low = y < y0
    s["p_def"][low, 1] = y0 + np.float32(0.02) * (y[low] - y0)
    s["F"][np.ix_(low, [1, 4, 7])] *= np.float32(0.02)
    _, facts = _grid_facts(s)
    facts.update(base_own_max=int(cell_table(base["p_def"], opt["hash_grid_size"])["own"].max()))
    return s, facts


def warp_shares(state, max_iter_num=5):
    """The Newton warps of the test camera's ray points through their three nearest IPs (oracle.warp_points, the march's own function): the share
    that runs >= 3 updates at `max_iter_num`, the share the IP_dx test rejects, the share of points with some but not all of their three warps
    rejected, and whether every result is finite.  Points whose third-nearest IP is a hash cell size or more away are left out: for the others the three nearest IPs
    overall lie in the point's 27 cells and are the march's candidates."""
    x, _ = ray_points(march_inputs(state))
    x = x[::5]
    p = state["p_def"].astype(np.float64)
    ids, d3 = np.empty((len(x), 3), np.int64), np.empty(len(x))
    for i in range(0, len(x), 4096):
        d2 = ((x[i:i + 4096, None, :].astype(np.float64) - p[None]) ** 2).sum(-1)
        ids[i:i + 4096] = np.argsort(d2, axis=1, kind="stable")[:, :3]
        d3[i:i + 4096] = np.sqrt(np.take_along_axis(d2, ids[i:i + 4096, 2:3], 1)[:, 0])
    near = d3 < float(state["hash_grid_size"])
    x, ids = x[near], ids[near]
    out, rej, upd = oracle.warp_points(np.repeat(x, 3, 0), ids.reshape(-1), state["p_ori"], state["p_def"], state["F"], state["dF"], max_iter_num,
                                       np.float32(state["IP_dx"]))
    out2, _, _ = oracle.warp_points(np.repeat(x, 3, 0), ids.reshape(-1), state["p_ori"], state["p_def"], state["F"], state["dF"], 2, np.float32(state["IP_dx"]))
    n_rej = rej.reshape(-1, 3).sum(1)
    return dict(warps=int(len(rej)), share_3_or_more_updates=float((upd >= 3).mean()), share_rejected=float(rej.mean()),
                share_moved_1e_4_after_update_2=float((np.abs(out - out2).max(1) > 1e-4).mean()),
                share_points_partly_rejected=float(((n_rej > 0) & (n_rej < 3)).mean()), finite=bool(np.isfinite(out).all()))


def twisted(base, opt):
    """dF scaled by TWIST = 100 (chosen among 1, 20, 100, 300 with warp_shares, below).  Measured on the small chair with the oracle's warp on
    the 7 254 warps of every fifth ray point of the test camera, max_iter_num = 5: every warp runs >= 3 Newton updates (but so do 99.5 % at
    TWIST = 1: the 1e-12 stopping test is that strict), 76.2 % end more than 1e-4 away from where two updates leave them (none at TWIST = 1, 18.9 %
    at 20) — those are the warps that NEED iterations 3 .. 5; 6.2 % are rejected by the IP_dx test, and 15.1 % of the points have some but not
    all of their three warps rejected; every result is finite."""
    s = _copy(base, opt)
    s["dF"] *= np.float32(TWIST)
    _, facts = _grid_facts(s)
    facts.update(warp_shares(s))
    return s, facts


def coincident(base, opt, ckpt):
    """32 IPs, each with one axis-parallel ray (both signs of all three axes) whose first sample o + t d equals the IP's p_def bit for bit.  The
    ray of IP i along axis a with sign s starts at o = p_def_i with o[a] = -4 s and has rays_t = fl(4 + s p_def_i[a]); o[a] + t s, in float32, is
    then written back into p_def_i[a].  (d has components 0 and +-1 only: t * d is exact, so a contracted multiply-add gives the same bits.)
      rays  0 .. 15   a second IP j (id >= i + 100, another p_ori) is moved to the same p_def: two candidates at d == 0, the lower id first
      rays 16 .. 23   rays_t = 4, so the sample's coordinate on the axis is 0; a second IP j with a LOWER id sits at 2^-70 on that axis,
                      d^2 = 2^-140: a float denormal that a flush to zero would turn into a tie, which the lower id would win
      rays 24 .. 31   the IP alone
    The IPs are taken from those whose REST position lies in an occupied density voxel (d == 0 warps the sample to p_ori exactly).
    Returns (state, rays, facts); rays = dict(o, d, t, nears, fars, alive) for n_step = 1."""
    s = _copy(base, opt)
    n = len(s["p_def"])
    occ = np.nonzero(occupied(ckpt, s["p_ori"]))[0]
    assert len(occ) >= 64
    rng = np.random.default_rng(13)
    low = occ[occ < n - 100]
    first = rng.choice(low[low >= 24], 24, replace=False)                 # ids with 100 higher ids above them (and 8 lower ones to spare)
    used = set(first.tolist())
    partner = []
    for i in first[:16]:                                                   # the nearest unused occupied IP at rest, 100 ids up
        cand = [j for j in occ if j >= i + 100 and j not in used]
        j = min(cand, key=lambda j: float(((s["p_ori"][j] - s["p_ori"][i]) ** 2).sum()))
        used.add(int(j))
        partner.append(int(j))
    for i in first[16:24]:                                                  # a lower id for the denormal neighbour
        j = max(j for j in range(int(i)) if j not in used)
        used.add(j)
        partner.append(j)
    last = rng.choice([j for j in occ if j not in used], 8, replace=False)
    ips = np.concatenate([first, last]).astype(np.int64)
    o, d, t = np.empty((32, 3), np.float32), np.zeros((32, 3), np.float32), np.empty(32, np.float32)
    for r, i in enumerate(ips):
        a, sg = r % 3, np.float32(1.0 if (r // 3) % 2 == 0 else -1.0)
        o[r] = s["p_def"][i]
        o[r, a] = np.float32(-4.0) * sg
        t[r] = np.float32(4.0) if 16 <= r < 24 else np.float32(4.0) + sg * s["p_def"][i, a]
        d[r, a] = sg
        s["p_def"][i] = o[r] + t[r] * d[r]
    for r, j in enumerate(partner):
        s["p_def"][j] = s["p_def"][ips[r]]
        if r >= 16:
            s["p_def"][j, r % 3] = np.float32(2.0 ** -70)
    sample = o + t[:, None] * d
    d2 = ((s["p_def"][partner] - sample[:24]) ** 2).sum(1, dtype=np.float32)
    t_hash = cell_table(s["p_def"], s["hash_grid_size"])
    x = np.minimum(np.maximum(sample, t_hash["bbmin"]), (t_hash["bbmax"].astype(np.float64) - 1e-6).astype(np.float32))
    facts = dict(samples_on_their_IP=int((sample.view(np.uint32) == s["p_def"][ips].view(np.uint32)).all(1).sum()),
                 samples_inside_the_box=int((x.view(np.uint32) == sample.view(np.uint32)).all(1).sum()),
                 partners_at_zero=int((d2[:16] == 0).sum()), partners_at_denormal=int((d2[16:] == np.float32(2.0 ** -140)).sum()),
                 partner_id_gap_min=int((np.array(partner[:16]) - ips[:16]).min()), denormal_partners_with_lower_id=int((np.array(partner[16:]) < ips[16:24]).sum()),
                 p_ori_distinct=int(len(np.unique(s["p_ori"], axis=0))), n_IP=n, axes_and_signs=len({(r % 3, (r // 3) % 2) for r in range(32)}))
    rays = dict(o=o, d=d, t=t, nears=t.copy(), fars=(t + np.float32(0.5)).astype(np.float32), alive=np.arange(32, dtype=np.int32), ips=ips,
                partner=np.array(partner))
    return s, rays, facts


BUILDERS = dict(crowded=crowded, sparse=sparse, singular=singular, squashed=squashed, twisted=twisted)


def build(name, base, opt):
    state, facts = BUILDERS[name](base, opt)
    for k in ("p_def", "p_ori", "F", "dF"):
        assert state[k].dtype == np.float32 and np.isfinite(state[k]).all(), (name, k)
    return state, facts


def check_facts(name, facts):
    """The properties each state is built for (the figures measured on the small chair are in the builders' docstrings)."""
    f = facts
    if name == "crowded":
        assert f["list_max"] > STAGE_CAP and f["cells_over_cap"] >= 1, f        # a list that never fits the wave's LDS
        assert f["cells_in_256_cap"] >= 1, f                                      # lists of which the second or third overflows
        assert f["own_max"] >= 100, f                                             # the insertion sort of a cell, the packed counters
        assert f["ray_points_in_cells_over_cap"] >= 1, f                          # ... and the test camera's rays really cross such a cell
        assert f["copies_tie"] and f["p_ori_distinct"] == f["n_IP"], f            # exact ties between copies that can be told apart
    elif name == "sparse":
        assert f["cells_own0_list_pos"] >= 1 and f["cells_list1"] >= 1 and f["cells_list2"] >= 1, f
    elif name == "singular":
        assert f["det_zero"] == f["want_det_zero"] > 0 and f["det_negative"] == f["want_det_negative"] > 0, f
    elif name == "squashed":
        assert f["own_max"] >= 3 * f["base_own_max"], f
    elif name == "twisted":
        assert f["share_3_or_more_updates"] >= 0.10 and f["share_moved_1e_4_after_update_2"] >= 0.10, f   # Newton really iterates
        assert 0.01 <= f["share_rejected"] <= 0.50 and f["share_points_partly_rejected"] >= 0.01 and f["finite"], f
    elif name == "coincident":
        assert f["samples_on_their_IP"] == 32 and f["samples_inside_the_box"] == 32 and f["axes_and_signs"] == 6, f
        assert f["partners_at_zero"] == 16 and f["partners_at_denormal"] == 8 and f["partner_id_gap_min"] >= 100, f
        assert f["denormal_partners_with_lower_id"] == 8 and f["p_ori_distinct"] == f["n_IP"], f
    else:
        raise KeyError(name)


def frame_opt(opt, state, **over):
    """The options of a whole frame rendered from `state`: its hash cell size, and whatever the test sets."""
    return dict(opt, hash_grid_size=state["hash_grid_size"], **over)


def oracle_march(state, m, ck, alive, num_seek_IP, max_iter_num, n_step, rays_t=None):
    """oracle.march_rays_quadratic_bending on a state, no --cut, fixed step: (xyzs, dirs, deltas)."""
    rays_t = m["nears"] if rays_t is None else rays_t
    return oracle.march_rays_quadratic_bending(*m["pig"], len(state["p_def"]), m["n_grid"], state["p_def"], state["p_ori"], state["F"], state["dF"],
                                               max_iter_num, m["bbmin"], m["bbmax"], m["hgs"], m["res"], num_seek_IP, np.float32(state["IP_dx"]), False,
                                               np.zeros(6, np.float32), len(alive), n_step, alive, rays_t, m["o"], m["d"], 1.0, ck["density_bitfield"],
                                               ck["cascade"], ck["grid_size"], m["nears"], m["fars"], 128, False, 0.0, 1024)


def coincident_inputs(state, rays):
    """The march inputs of the `coincident` state's 32 rays (the counterpart of march_inputs)."""
    t = cell_table(state["p_def"], state["hash_grid_size"])
    return dict(o=rays["o"], d=rays["d"], hgs=t["hgs"], bbmin=t["bbmin"], bbmax=t["bbmax"], res=t["res"], n_grid=t["n_grid"], pig=t["pig"],
                nears=rays["nears"], fars=rays["fars"])
