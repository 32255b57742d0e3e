"""Scenes whose colour camera differs from the depth camera -- another image size, another focal length, another principal point --
for tests/test_cpu_two_cameras.py and tests/test_gpu_two_cameras.py; the helpers that load them into the CPU oracle and into the HIP
backend; a census in numpy float64 of how much colour-invalid and border work a scene holds; and a plain float64 model of the
colour chain (depth pixel -> colour pixel -> bilinear luma samples -> descriptor residuals), written from CUDA's documented
texture rules and not from the oracle.  A plain module: no fixtures, no conftest.

Every other scene of the suite gives the colour image the depth image's size and the depth camera's parameters; the valid depth
region ends 2 px inside the image, so no pair there has an invalid colour pixel or a sample near the colour image's border.

Cameras are fx, fy, cx, cy (pixel-corner convention); the depth camera is synthetic.test_camera of the depth size.  Colour images
are rendered by synthetic.render_planes with the colour camera at the keyframe's ground-truth pose.

  scene       depth    colour image, colour camera                 keyframes, perturbation
  same        320x240  320x240, = depth                            4, seed 17; poses 5 mm / 1 mrad off, a cfactor image
  large       320x240  487x363, (181.8, 178.2, 246.3, 178.3)       (the same)
  crop_small  320x240  211x157, (108, 110, 100.8, 80.6)            (the same)
  tiny        70x45    53x38,   (20, 21, 24.8, 19.1)               (the same)
  crop        320x240  320x240, (168, 164.4, 165.8, 115.4)         6, small_scene(seed=3), as ..._vs_reference.py::_perturbed_oracle

Census (this module's census() on the oracle's surfels, measured on the CPU; "non-interior": colour-valid pairs with at least one of
the three sample points -- centre and the two tangent points -- outside 0 <= x - 0.5 < w, 0 <= y - 0.5 < h; "near border": colour-
valid pairs whose centre lies within 2 px of the colour image's border):

  scene       surfels  associated  colour-invalid  share    non-interior  near border
  same        31 057   96 191      0               0 %      17            0
  large       31 057   96 191      0               0 %      0             0
  crop_small  31 057   96 191      40 789          42.4 %   1 323         2 463
  tiny        1 142    3 489       318             9.1 %    225           426
  crop        45 065   178 299     69 034          38.7 %   1 999         2 588

The oracle's own evaluate_pairs gives the same associated and colour-invalid counts on all five.  The tests require the shares of
MIN_INVALID_SHARE and at least half the measured non-interior pairs (MIN_NON_INTERIOR) before they trust a scene.

The float64 model against the reference's own functions (oracle/ref_binding.py: evaluate_pairs) on the associated, colour-valid pairs
of crop_small and tiny: colour-valid decisions equal on every pair whose float64 colour pixel is further than 1e-3 px from a bound
(5 of 96 191 pairs are nearer on crop_small, none on tiny); largest descriptor-residual deviation 1.52e-3 on crop_small (7.7e-4 on
tiny), the oracle's 1.52e-3 (6.9e-4): REFERENCE_VS_MODEL = 1.52e-3, MODEL_RESIDUAL_BOUND = 4 x that = 6.08e-3.
"""
from dataclasses import dataclass

import numpy as np

from badslam_amd import se3, synthetic
from oracle import binding as ob
from tests import common

COLOUR = {
    "same": None,
    "large": (487, 363, (181.8, 178.2, 246.3, 178.3)),
    "crop_small": (211, 157, (108.0, 110.0, 100.8, 80.6)),
    "tiny": (53, 38, (20.0, 21.0, 24.8, 19.1)),
    "crop": (320, 240, (168.0, 164.4, 165.8, 115.4)),
}
# what the tests require of a scene before they trust it to exercise anything: the smallest share of colour-invalid pairs
# among the associated ones, and the smallest number of non-interior pairs (half of what census() measured; see the table)
MIN_INVALID_SHARE = {"same": 0.0, "large": 0.0, "crop_small": 0.20, "crop": 0.20, "tiny": 0.05}
MIN_NON_INTERIOR = {"same": 0, "large": 0, "crop_small": 661, "crop": 999, "tiny": 112}
MAX_SURFELS = {"same": 200000, "large": 200000, "crop_small": 200000, "tiny": 8000, "crop": 400000}


@dataclass
class TwoCameraScene:
    name: str
    scene: synthetic.Scene            # depth images at scene.width x scene.height; scene.rgb holds the COLOUR camera's images
    color_camera: np.ndarray          # fx, fy, cx, cy (float32)
    color_width: int
    color_height: int
    poses: list                       # the perturbed global_T_frame of every keyframe
    seed: int

    @property
    def max_surfels(self):
        return MAX_SURFELS[self.name]


def _with_colour_camera(name, scene, poses, seed):
    spec = COLOUR[name]
    if spec is None:
        return TwoCameraScene(name, scene, scene.camera.copy(), scene.width, scene.height, poses, seed)
    cw, ch, cam = spec
    cam = np.asarray(cam, np.float32)
    scene.rgb = [synthetic.render_planes(T, scene.planes, cam, cw, ch, scene.raw_to_float_depth)[1] for T in scene.poses_gt]
    return TwoCameraScene(name, scene, cam, cw, ch, poses, seed)


def build_scene(name):
    """The scene `name` of the table above: images and perturbed poses (no oracle, no GPU)."""
    if name == "crop":
        scene = common.small_scene(num_keyframes=6, seed=3)
        return _with_colour_camera(name, scene, list(scene.poses_gt), 3)
    width, height = (70, 45) if name == "tiny" else (320, 240)
    scene = synthetic.make_scene(4, width, height, seed=17, cell=2, translation_range=0.6, rotation_range=0.25)
    return _with_colour_camera(name, scene, None, 5)


def displace(ba, seed):
    """tests/test_cpu_oracle_vs_reference.py::_perturbed_oracle's state: surfels up to 4 mm off the surface and 3 units off their
    descriptors, keyframe 3 inactive, keyframe 1 co-visible."""
    n = ba.surfels_size
    rng = np.random.Generator(np.random.PCG64(seed))
    ba.surfel_data[2, :n] += rng.uniform(0, 0.004, n).astype(np.float32)
    ba.surfel_data[6:8, :n] += rng.uniform(-3, 3, (2, n)).astype(np.float32)
    ba.keyframes[3].activation = ob.KF_INACTIVE
    ba.keyframes[1].activation = ob.KF_COVIS_ACTIVE
    return ba


def perturb(tc, ba):
    """Brings a freshly built oracle (surfels created at the ground-truth poses) into the scene's perturbed state, the way the suite
    does for its single-camera scenes: `crop` as _perturbed_oracle (surfels up to 4 mm and 3 descriptor units off, keyframe 3
    inactive, keyframe 1 co-visible), the others with poses 5 mm / 1 mrad off (synthetic.perturb_pose) and a cfactor image of U(+-2e-3), as vga_scene has."""
    if tc.name == "crop":
        return displace(ba, tc.seed)
    rng = np.random.Generator(np.random.PCG64(tc.seed))
    tc.poses = [synthetic.perturb_pose(rng, T) for T in tc.scene.poses_gt]
    for k, T in enumerate(tc.poses):
        ba.set_pose(k, T)
    ba.cfactor[:] = rng.uniform(-2e-3, 2e-3, ba.cfactor.shape).astype(np.float32)
    return ba


def build_oracle(tc, use_depth=True, use_desc=True, create_from=None, perturbed=True, min_observation_count=2):
    """common.build_oracle with the scene's own colour camera and image size."""
    scene = tc.scene
    color = ob.make_camera(tc.color_camera, tc.color_width, tc.color_height)
    depth = ob.make_camera(scene.camera, scene.width, scene.height)
    ba = ob.OracleBA(tc.max_surfels, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, color, depth,
                     use_depth_residuals=use_depth, use_descriptor_residuals=use_desc, min_observation_count=min_observation_count)
    for k in range(len(scene.depth)):
        ba.add_keyframe(scene.depth[k], scene.rgb[k], scene.poses_gt[k])
    for k in (range(len(scene.depth)) if create_from is None else create_from):
        ba.create_surfels_for_keyframe(k)
    return perturb(tc, ba) if perturbed else ba


def build_gpu(tc, ba=None, ctx=None):
    """common.build_gpu with the scene's own colour camera and image size, no surfels created; with `ba` the oracle's state -- surfels,
    flags, poses, activations, cameras, a, cfactor image -- is copied over and the keyframes are bound."""
    from badslam_amd import capi, lowlevel as ll
    scene = tc.scene
    ctx = ctx or ll.Context()
    color = ll.make_camera(tc.color_camera, tc.color_width, tc.color_height)
    depth = ll.make_camera(scene.camera, scene.width, scene.height)
    g = ll.Scene(ctx, tc.max_surfels, scene.raw_to_float_depth, scene.baseline_fx, scene.cell, color, depth)
    for k in range(len(scene.depth)):
        g.add_keyframe(scene.depth[k], scene.rgb[k], scene.poses_gt[k])
    if ba is not None:
        sync_gpu(g, ba)
    return g


def sync_gpu(g, ba, active=None):
    """Copies the oracle's state into the GPU scene and binds the keyframes."""
    from badslam_amd import lowlevel as ll
    n = ba.surfels_size
    g.upload_surfels(ba.surfel_data[:, :n].copy(), ba.active[:n].copy() if active is None else active)
    for k, kf in enumerate(ba.keyframes):
        g.keyframes[k]["pose"] = kf.global_T_frame.to_array().astype(np.float32)
        g.keyframes[k]["activation"] = int(kf.activation)
    for name, src in (("color_cam", ba.color_cam), ("depth_cam", ba.depth_cam)):
        setattr(g, name, ll.make_camera([src.fx, src.fy, src.cx, src.cy], src.width, src.height))
    g.dp.a = float(ba.dp.a)
    g.cfactor.upload(ba.cfactor)
    g.set_intrinsics()
    g.bind_keyframes()
    return g


# ---- float64 restatements -----------------------------------------------------------------------------------------------------------
def _camera(cam):
    return np.array([cam.fx, cam.fy, cam.cx, cam.cy], np.float64), int(cam.width), int(cam.height)


def _unpack_normal10(bits):
    def ten(v):
        return (((v & 0x3ff).astype(np.int64) ^ 0x200) - 0x200) / 511.0
    n = np.stack([ten(bits), ten(bits >> 10), ten(bits >> 20)])
    return n / np.linalg.norm(n, axis=0)


def _unpack_normal8(code):
    x = (code & 0xff).astype(np.uint8).view(np.int8) / 127.0
    y = (code >> 8).astype(np.uint8).view(np.int8) / 127.0
    return np.stack([x, y, -np.sqrt(np.maximum(0.0, 1 - x * x - y * y))])


def colour_geometry(surfels, pose, depth_cam, color_cam):
    """For every surfel column of `surfels` (>= 5 rows: position, packed normal, squared radius) seen from the keyframe at
    global_T_frame `pose`, all in float64: dict(local (3, N), depth pixel (2, N), in_image, colour pixel c (2, N) = d2c(depth pixel),
    colour_valid (0 <= c < size), margin (distance of c to the nearest bound of that test, px), the tangent points' colour pixels
    t1, t2 (2, N), interior (all three samples satisfy 0 <= x - 0.5 < w, 0 <= y - 0.5 < h))."""
    (fx, fy, cx, cy), W, H = _camera(depth_cam)
    (cfx, cfy, ccx, ccy), cw, ch = _camera(color_cam)
    inv = se3.inverse(np.asarray(pose, np.float64))
    R, t = se3.quat_to_rot(inv[:4]), inv[4:]
    gp = np.asarray(surfels[:3], np.float64)
    gn = _unpack_normal10(np.ascontiguousarray(surfels[3]).view(np.uint32))
    radius_sq = np.asarray(surfels[4], np.float64)
    local = R @ gp + t[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        px = np.stack([fx * local[0] / local[2] + cx, fy * local[1] / local[2] + cy])
        in_image = (local[2] > 0) & (px[0] >= 0) & (px[1] >= 0) & (px[0] < W) & (px[1] < H)
        # TransformDepthToColorPixelCorner: the colour camera's projection of the depth pixel's ray
        c = np.stack([cfx * (px[0] - cx) / fx + ccx, cfy * (px[1] - cy) / fy + ccy])
        colour_valid = (c[0] >= 0) & (c[1] >= 0) & (c[0] < cw) & (c[1] < ch)
        margin = np.minimum.reduce([np.abs(c[0]), np.abs(c[1]), np.abs(c[0] - cw), np.abs(c[1] - ch)])
        # ComputeTangentProjections: gp + t1, gp + t2 with |t| = 2 radius in the surfel's plane, through the colour camera
        axis = np.where(np.abs(gn[0]) > 0.9, 1, 0)
        e = np.zeros_like(gn)
        e[0], e[1] = axis == 0, axis == 1
        t1 = np.cross(gn, e, axis=0)
        t1 *= 2.0 * np.sqrt(radius_sq / np.maximum(1e-12, (t1 * t1).sum(0)))
        t2 = np.cross(gn, t1, axis=0)
        t2 *= 2.0 * np.sqrt(radius_sq / np.maximum(1e-12, (t2 * t2).sum(0)))
        tangents = []
        for tv in (t1, t2):
            q = R @ (gp + tv) + t[:, None]
            tangents.append(np.stack([cfx * q[0] / q[2] + ccx, cfy * q[1] / q[2] + ccy]))

        def inside(p):
            return (p[0] - 0.5 >= 0) & (p[0] - 0.5 < cw) & (p[1] - 0.5 >= 0) & (p[1] - 0.5 < ch)
        interior = inside(c) & inside(tangents[0]) & inside(tangents[1])
    return dict(local=local, normal=gn, R=R, pixel=px, in_image=in_image, c=c, colour_valid=colour_valid, margin=margin,
                t1=tangents[0], t2=tangents[1], interior=interior, color_size=(cw, ch))


def census(ba, surfels=None, poses=None):
    """Counts, in numpy float64 from the surfel rows and the poses (and the keyframes' depth / normal images, the cfactor image and
    the cameras the oracle object `ba` holds): dict(surfels, associated pairs, colour_invalid pairs among them, non_interior pairs
    among the colour-valid ones, near_border: colour-valid pairs whose centre is within 2 px of the colour image's border).  The
    association test is B/surfel_projection_nvcc_only.cuh's, restated (a pair on a last-bit edge may fall either way: a census)."""
    n = ba.surfels_size
    surfels = ba.surfel_data[:8, :n] if surfels is None else surfels
    (fx, fy, cx, cy), W, H = _camera(ba.depth_cam)
    cell, a, scale, baseline_fx = int(ba.dp.cell), float(ba.dp.a), float(ba.dp.raw_to_float_depth), float(ba.dp.baseline_fx)
    out = dict(surfels=int(surfels.shape[1]), associated=0, colour_invalid=0, non_interior=0, near_border=0)
    for k in range(len(ba.keyframes)):
        pose = ba.pose(k) if poses is None else poses[k]
        g = colour_geometry(surfels, pose, ba.depth_cam, ba.color_cam)
        ok = g["in_image"] & ~np.isnan(g["local"][0])
        ix = np.where(ok, g["pixel"][0], 0).astype(np.int64)
        iy = np.where(ok, g["pixel"][1], 0).astype(np.int64)
        arrs = ba.kf_arrays(k)
        raw = arrs["depth"][iy, ix]
        ok &= (raw & 0x8000) == 0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            inv_depth = 1.0 / (scale * raw.astype(np.float64))
            depth = 1.0 / (ba.cfactor[iy // cell, ix // cell].astype(np.float64) * np.exp(-a * inv_depth) + inv_depth)
            nl = g["R"] @ g["normal"]
            nx, ny = (ix - (cx - 0.5)) / fx, (iy - (cy - 0.5)) / fy
            stddev = 0.1 * np.abs(nl[0] * nx + nl[1] * ny + nl[2]) * depth * depth / baseline_fx
            ok &= np.abs(g["local"][2] - depth) <= 10.0 * stddev
            ok &= (g["local"] * nl).sum(0) <= 0
            ok &= (nl * _unpack_normal8(arrs["normals"][iy, ix])).sum(0) >= 0.76604
        cw, ch = g["color_size"]
        valid = ok & g["colour_valid"]
        near = (g["c"][0] <= 2) | (g["c"][1] <= 2) | (g["c"][0] >= cw - 2) | (g["c"][1] >= ch - 2)
        out["associated"] += int(ok.sum())
        out["colour_invalid"] += int((ok & ~g["colour_valid"]).sum())
        out["non_interior"] += int((valid & ~g["interior"]).sum())
        out["near_border"] += int((valid & near).sum())
    return out


def assert_scene_has_the_work(tc, ba):
    """What every test asserts first: the scene holds the colour-invalid pairs and the border samples it claims to exercise."""
    c = census(ba)
    assert c["associated"] > 1000, c
    assert c["colour_invalid"] >= MIN_INVALID_SHARE[tc.name] * c["associated"], (tc.name, c)
    assert c["non_interior"] >= MIN_NON_INTERIOR[tc.name], (tc.name, c)
    if MIN_INVALID_SHARE[tc.name] > 0:
        assert c["colour_invalid"] < c["associated"] - 1000, (tc.name, c)      # ... and pairs with a descriptor as well
    return c


def bilinear(image, x, y):
    """CUDA's documented linear filter on unnormalised coordinates with clamp addressing (CUDA C Programming Guide, "Texture
    Fetching"): texel centres at +0.5, i = floor(x - 0.5), alpha = x - 0.5 - i, indices clamped to [0, size - 1]; float64."""
    h, w = image.shape
    xb, yb = np.asarray(x, np.float64) - 0.5, np.asarray(y, np.float64) - 0.5
    i, j = np.floor(xb), np.floor(yb)
    alpha, beta = xb - i, yb - j
    i0, i1 = np.clip(i, 0, w - 1).astype(np.int64), np.clip(i + 1, 0, w - 1).astype(np.int64)
    j0, j1 = np.clip(j, 0, h - 1).astype(np.int64), np.clip(j + 1, 0, h - 1).astype(np.int64)
    top = (1 - alpha) * image[j0, i0] + alpha * image[j0, i1]
    bottom = (1 - alpha) * image[j1, i0] + alpha * image[j1, i1]
    return (1 - beta) * top + beta * bottom


def model_pairs(ba, k, surfels=None, pose=None):
    """The float64 model of the colour chain for every surfel against keyframe k: dict(colour_valid, margin, residual (2, N)) with
    residual = 180 (I(t) - I(c)) - d, I the bilinear luma (the image's fourth channel / 255) -- meaningful wherever a pair is
    associated (the model takes the association from whoever it is compared with: it restates the colour chain only)."""
    n = ba.surfels_size
    surfels = ba.surfel_data[:8, :n] if surfels is None else surfels
    g = colour_geometry(surfels, ba.pose(k) if pose is None else pose, ba.depth_cam, ba.color_cam)
    luma = ba.kf_arrays(k)["color"][:, :, 3].astype(np.float64) / 255.0

    def sample(p):
        finite = np.isfinite(p[0]) & np.isfinite(p[1])
        x = np.clip(np.where(finite, p[0], 0.0), -10.0, luma.shape[1] + 10.0)     # clamp addressing: far outside == at the edge
        y = np.clip(np.where(finite, p[1], 0.0), -10.0, luma.shape[0] + 10.0)
        return bilinear(luma, x, y)
    centre = sample(g["c"])
    residual = np.stack([180.0 * (sample(g["t1"]) - centre) - np.asarray(surfels[6], np.float64),
                         180.0 * (sample(g["t2"]) - centre) - np.asarray(surfels[7], np.float64)])
    return dict(colour_valid=g["colour_valid"], margin=g["margin"], residual=residual, interior=g["interior"])


def against_the_model(ba, k, associated, valid, residual):
    """One implementation's pairs of keyframe k -- masks `associated` and `valid` (colour pixel valid), `residual` (2, N) -- against
    model_pairs: (pairs, pairs left out by the margin rule, colour-valid mismatches outside it, pairs compared, largest residual
    deviation on the pairs that both call colour-valid)."""
    model = model_pairs(ba, k)
    decided = model["margin"] > MODEL_MARGIN_PX
    both = associated & valid & model["colour_valid"]
    worst = float(np.abs(np.asarray(residual, np.float64) - model["residual"])[:, both].max()) if both.any() else 0.0
    return (int(associated.sum()), int((associated & ~decided).sum()), int((associated & decided & (valid != model["colour_valid"])).sum()),
            int(both.sum()), worst)


# The descriptor-residual bound of the float64 model: 4 x the largest deviation the reference's own functions show from the model on
# the associated, colour-valid pairs of crop_small and tiny (tests/test_cpu_two_cameras.py measures it and asserts that the bound
# is that multiple): a one-ulp difference in a binary32 pixel coordinate times 180 x the local luma gradient.
MODEL_MARGIN_PX = 1e-3            # colour-valid decisions are compared where the float64 colour pixel is further than this from a bound
MODEL_MAX_LEFT_OUT = 1e-3         # ... which may leave out at most this share of the pairs
REFERENCE_VS_MODEL = 1.52e-3
MODEL_RESIDUAL_BOUND = 4 * REFERENCE_VS_MODEL
