"""Thin Python conveniences over the C ABI (badslam_amd.capi): pitched device buffers, keyframe
image sets and a context object.  Used by the kernel-level parity tests and by tooling; the
DirectBA-level API lives in the C++ host library (badslam_amd/host) and its binding
(badslam_amd.directba).  No arithmetic happens here and nothing falls back to the CPU.
"""
import contextlib
import ctypes as C

import numpy as np

from . import capi


def cost_dict(c):
    """A bahip_cost as a dict (depth, descriptor_1, descriptor_2: float; depth_residuals, descriptor_pairs: int)."""
    return dict(depth=c.depth, descriptor_1=c.descriptor_1, descriptor_2=c.descriptor_2, depth_residuals=int(c.depth_residuals),
                descriptor_pairs=int(c.descriptor_pairs))


def live_allocations(lib=None):
    """(blocks, bytes) of device and page-locked memory the library holds for itself at the moment: bahip_debug_live_allocations."""
    count, nbytes = C.c_longlong(), C.c_longlong()
    capi.check((lib or capi.load()).bahip_debug_live_allocations(C.byref(count), C.byref(nbytes)))
    return int(count.value), int(nbytes.value)


def set_observed_structure_route(route, lib=None):
    """Which kernels the observed co-visibility, the keyframe redundancy and the observation lists run (process-wide test hook,
    bahip_debug_set_observed_structure_route): 0 = their own wherever those are allowed (the default), 1 = the tile mask table on an
    unsharded or surfel-sharded context too.  A keyframe-sharded context always takes the table."""
    capi.check((lib or capi.load()).bahip_debug_set_observed_structure_route(int(route)))


def set_tile_mask_shape(waves=0, workgroups=0, tile_order=-1, entry_slice=0, payload_slice=0, lib=None):
    """Launch shape and exchange slices of the tile mask table (process-wide test hook, bahip_debug_set_tile_mask_shape); no argument:
    the defaults."""
    capi.check((lib or capi.load()).bahip_debug_set_tile_mask_shape(int(waves), int(workgroups), int(tile_order), int(entry_slice),
                                                                    int(payload_slice)))


def split_render_key(key):
    """A key plane of bahip_render_surfels (uint64: bits(depth) << 32 | index, all ones where empty) as (depth float32, index uint32) with
    the empty pixels as the call's own depth and index planes have them: +0.0 and 0xFFFFFFFF.  The elementwise minimum of the key planes
    of several renders (shards, clouds with their own index_base) is the key plane of their union."""
    key = np.ascontiguousarray(key, np.uint64)
    empty = key == np.uint64(0xFFFFFFFFFFFFFFFF)
    depth = np.where(empty, np.uint32(0), (key >> np.uint64(32)).astype(np.uint32)).astype(np.uint32).view(np.float32)
    index = (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return depth, index


def split_residual_key(key, select=capi.RESIDUAL_BEST):
    """A key plane of bahip_frame_residual_image (uint64: magnitude word << 32 | index, all ones where empty) as (|raw| float32, index
    uint32): the magnitude word is bits(|raw|) under RESIDUAL_BEST and 0x7fffffff - bits(|raw|) under RESIDUAL_WORST; empty pixels
    give +0.0 and 0xFFFFFFFF, as the call's own planes have them.  The sign of raw is in the depth_residual plane only.  The
    elementwise minimum of the key planes of several shards (each with its own index_base) is the key plane of their union."""
    key = np.ascontiguousarray(key, np.uint64)
    empty = key == np.uint64(0xFFFFFFFFFFFFFFFF)
    high = (key >> np.uint64(32)).astype(np.uint32)
    if int(select) == capi.RESIDUAL_WORST:
        high = np.uint32(0x7FFFFFFF) - np.where(empty, np.uint32(0x7FFFFFFF), high)
    magnitude = np.where(empty, np.uint32(0), high).astype(np.uint32).view(np.float32)
    index = (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return magnitude, index


RESIDUAL_IMAGE_PLANES = (("key", np.uint64, 1), ("pairs", np.uint32, 1), ("index", np.uint32, 1), ("depth_residual", np.float32, 1),
                         ("inv_stddev", np.float32, 1), ("desc_residual", np.float32, 2), ("color_valid", np.uint8, 1))


def frame_residual_image(ctx, frame, frame_T_global, surfels, width, height, select=capi.RESIDUAL_BEST, index_base=0, planes=None,
                         prefill=None):
    """bahip_frame_residual_image for one frame (capi.Frame, or None) at frame_T_global (12 floats) over `surfels` (capi.Surfels): a
    dict of numpy arrays of height x width pixels of the depth camera -- key (uint64), pairs, index (uint32), depth_residual,
    inv_stddev (float32), desc_residual (x 2, float32), color_valid (uint8).  planes: the names to ask for (the others are passed as
    NULL and left out of the dict); prefill: a byte value the device planes are filled with before the call (tests: an entry the call
    did not write shows; after a refused call the planes come back as filled).  Raises capi.BackendError when the call is refused --
    the dict of the untouched planes is then the exception's `planes` attribute when prefill was given."""
    w, h = int(width), int(height)
    n = max(1, w * h)
    wanted = [name for name, _, _ in RESIDUAL_IMAGE_PLANES] if planes is None else list(planes)
    bufs = {name: DeviceBuffer2D(ctx, 1, n, dtype, channels) for name, dtype, channels in RESIDUAL_IMAGE_PLANES if name in wanted}
    shapes = {name: (h, w) if channels == 1 else (h, w, channels) for name, _, channels in RESIDUAL_IMAGE_PLANES}
    download = lambda: {name: b.download()[0, :w * h].reshape(shapes[name]).copy() for name, b in bufs.items()}   # noqa: E731
    try:
        if prefill is not None:
            for b in bufs.values():
                b.clear(prefill)
        F = (C.c_float * 12)(*[float(v) for v in frame_T_global])
        opt = capi.ResidualImageOptions(select, index_base)
        out = capi.ResidualImageOut(*[bufs[name].ptr if name in bufs else None for name, _, _ in RESIDUAL_IMAGE_PLANES])
        try:
            capi.check(ctx.lib.bahip_frame_residual_image(ctx.handle, C.byref(frame) if frame is not None else None, F, C.byref(surfels),
                                                          C.byref(opt), C.byref(out)))
        except capi.BackendError as e:
            if prefill is not None:
                ctx.synchronize()
                e.planes = download()
            raise
        return download()
    finally:
        for b in bufs.values():
            b.free()


class DeviceBuffer2D:
    """libvis CUDABuffer<T> semantics: (height, width) pitched device allocation."""

    def __init__(self, ctx, height, width, dtype, channels=1):
        self.ctx, self.height, self.width = ctx, int(height), int(width)
        self.dtype, self.channels = np.dtype(dtype), int(channels)
        self.elem_bytes = self.dtype.itemsize * self.channels
        ptr, pitch = C.c_void_p(), C.c_size_t()
        capi.check(ctx.lib.bahip_malloc_pitch(C.byref(ptr), C.byref(pitch), self.width * self.elem_bytes, self.height))
        self.ptr, self.pitch = ptr.value, pitch.value

    def upload(self, array):
        a = np.ascontiguousarray(array, dtype=self.dtype).reshape(self.height, self.width * self.channels)
        capi.check(self.ctx.lib.bahip_memcpy_2d(self.ctx.handle, self.ptr, self.pitch, a.ctypes.data, a.strides[0],
                                                self.width * self.elem_bytes, self.height, 1))
        return self

    def download(self):
        shape = (self.height, self.width) if self.channels == 1 else (self.height, self.width, self.channels)
        out = np.empty(shape, dtype=self.dtype)
        capi.check(self.ctx.lib.bahip_memcpy_2d(self.ctx.handle, out.ctypes.data, self.width * self.elem_bytes, self.ptr,
                                                self.pitch, self.width * self.elem_bytes, self.height, 2))
        return out

    def clear(self, byte_value=0):
        capi.check(self.ctx.lib.bahip_memset_2d(self.ctx.handle, self.ptr, self.pitch, byte_value,
                                                self.width * self.elem_bytes, self.height))
        return self

    def free(self):
        if self.ptr:
            self.ctx.lib.bahip_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    def __init__(self, stream=None):
        self.lib = capi.load()
        h = C.c_void_p()
        capi.check(self.lib.bahip_context_create(C.byref(h), stream))
        self.handle = h

    def synchronize(self):
        capi.check(self.lib.bahip_context_synchronize(self.handle))

    def set_arithmetic(self, arithmetic):
        """"exact" (default: the oracle's bits) or "fast" (hardware reciprocal / square root / exp, contraction): bahip_context_set_arithmetic."""
        mode = {"exact": capi.ARITHMETIC_EXACT, "fast": capi.ARITHMETIC_FAST}.get(arithmetic, arithmetic)
        capi.check(self.lib.bahip_context_set_arithmetic(self.handle, int(mode)))

    @property
    def arithmetic(self):
        return "fast" if self.lib.bahip_context_get_arithmetic(self.handle) == capi.ARITHMETIC_FAST else "exact"

    def close(self):
        if self.handle:
            self.lib.bahip_context_destroy(self.handle)
            self.handle = None


def bilateral_filtering_and_depth_cutoff(ctx, depth_u16, sigma_xy, sigma_value, radius_factor, max_depth, raw_to_float_depth):
    """BadSlam::PreprocessFrame's depth filter on a host image (upload, filter on the GPU, download)."""
    d = np.ascontiguousarray(depth_u16, np.uint16)
    src = DeviceBuffer2D(ctx, d.shape[0], d.shape[1], np.uint16)
    dst = DeviceBuffer2D(ctx, d.shape[0], d.shape[1], np.uint16)
    src.upload(d)
    capi.check(ctx.lib.bahip_bilateral_filtering_and_depth_cutoff(ctx.handle, sigma_xy, sigma_value, radius_factor, int(max_depth),
                                                                  raw_to_float_depth, src.ptr, src.pitch, dst.ptr, dst.pitch,
                                                                  d.shape[1], d.shape[0]))
    return dst.download()


def median_filter_and_densify(ctx, depth_u16, iterations=1):
    """`iterations` rounds of BadSlam::PreprocessFrame's median filter and densification (bahip_median_filter_and_densify) on a host
    image of raw depth (0 = no measurement): upload, ping-pong between two device images, download."""
    d = np.ascontiguousarray(depth_u16, np.uint16)
    src = DeviceBuffer2D(ctx, d.shape[0], d.shape[1], np.uint16).upload(d)
    dst = DeviceBuffer2D(ctx, d.shape[0], d.shape[1], np.uint16)
    for _ in range(int(iterations)):
        capi.check(ctx.lib.bahip_median_filter_and_densify(ctx.handle, src.ptr, src.pitch, dst.ptr, dst.pitch, d.shape[1], d.shape[0]))
        src, dst = dst, src
    return src.download()


def downscale_depth_median(ctx, depth_u16, out_width, out_height):
    """Image<u16>::DownscaleUsingMedianWhileExcluding(0, ...) on a host image (bahip_downscale_depth_median)."""
    d = np.ascontiguousarray(depth_u16, np.uint16)
    src = DeviceBuffer2D(ctx, d.shape[0], d.shape[1], np.uint16).upload(d)
    dst = DeviceBuffer2D(ctx, max(1, int(out_height)), max(1, int(out_width)), np.uint16)
    capi.check(ctx.lib.bahip_downscale_depth_median(ctx.handle, src.ptr, src.pitch, d.shape[1], d.shape[0], dst.ptr, dst.pitch,
                                                    int(out_width), int(out_height)))
    return dst.download()


def downscale_rgb_half(ctx, rgb_u8, levels):
    """Image<Vec3u8>::DownscaleToHalfSize applied `levels` times to a host (H, W, 3) image (bahip_downscale_rgb_half)."""
    c = np.ascontiguousarray(rgb_u8, np.uint8)
    h, w = c.shape[:2]
    src = DeviceBuffer2D(ctx, h, w, np.uint8, 3).upload(c)
    dst = DeviceBuffer2D(ctx, max(1, h >> max(0, int(levels))), max(1, w >> max(0, int(levels))), np.uint8, 3)
    capi.check(ctx.lib.bahip_downscale_rgb_half(ctx.handle, src.ptr, src.pitch, w, h, int(levels), dst.ptr, dst.pitch))
    return dst.download()


def make_camera(params, width, height):
    p = np.asarray(params, dtype=np.float32)
    return capi.Camera(float(p[0]), float(p[1]), float(p[2]), float(p[3]), int(width), int(height))


def scaled_camera(cam, level):
    """PinholeCamera4f::Scaled(1 / 2^level): the four parameters (pixel-corner convention) times the factor in binary32, width and
    height int(factor * size + 0.5) -- the camera the BA runs with at a pyramid level."""
    if not 0 <= int(level) <= 3:
        raise ValueError("pyramid levels are 0 .. 3")
    factor = np.float32(1.0) / np.float32(1 << int(level))
    p = [float(np.float32(v) * factor) for v in (cam.fx, cam.fy, cam.cx, cam.cy)]
    return capi.Camera(p[0], p[1], p[2], p[3], int(float(factor) * cam.width + 0.5), int(float(factor) * cam.height + 0.5))


class Scene:
    """Intrinsics + cfactor image + surfel buffer + keyframes bound to one context."""

    def __init__(self, ctx, max_surfel_count, raw_to_float_depth, baseline_fx, cell, color_cam, depth_cam):
        self.ctx, self.lib = ctx, ctx.lib
        self.color_cam, self.depth_cam = color_cam, depth_cam
        W, H = depth_cam.width, depth_cam.height
        self.cf_w, self.cf_h = (W - 1) // cell + 1, (H - 1) // cell + 1
        self.cfactor = DeviceBuffer2D(ctx, self.cf_h, self.cf_w, np.float32).clear(0)
        self.dp = capi.DepthParams(0.0, raw_to_float_depth, baseline_fx, cell, self.cfactor.ptr, self.cfactor.pitch,
                                   self.cf_w, self.cf_h)
        self.surfel_buf = DeviceBuffer2D(ctx, capi.SURFEL_ATTRIBUTE_COUNT, max_surfel_count, np.float32).clear(0)
        self.active_buf = DeviceBuffer2D(ctx, 1, max_surfel_count, np.uint8).clear(0)
        self.supporting = [DeviceBuffer2D(ctx, H, W, np.uint32) for _ in range(capi.MERGE_BUFFER_COUNT)]
        self.capacity = int(max_surfel_count)
        self.surfels_size = 0
        self.surfel_count = 0
        self.keyframes = []   # dicts: depth, normals, radius, color (DeviceBuffer2D), pose (7,), activation, min/max depth
        self.set_intrinsics()

    def set_intrinsics(self):
        capi.check(self.lib.bahip_set_intrinsics(self.ctx.handle, C.byref(self.color_cam), C.byref(self.depth_cam), C.byref(self.dp)))

    def surfels_struct(self, size=None):
        return capi.Surfels(self.surfel_buf.ptr, self.surfel_buf.pitch, self.active_buf.ptr,
                            self.surfels_size if size is None else size, self.capacity)

    # Keyframe ctor #2 (B/keyframe.cc:81-158)
    def add_keyframe(self, depth_u16, rgb_u8, global_T_frame):
        ctx = self.ctx
        W, H = self.depth_cam.width, self.depth_cam.height
        cw, ch = self.color_cam.width, self.color_cam.height
        rgb = DeviceBuffer2D(ctx, ch, cw, np.uint8, 3).upload(rgb_u8)
        raw = DeviceBuffer2D(ctx, H, W, np.uint16).upload(depth_u16)
        return self._add_keyframe_from_device(raw, rgb, global_T_frame)

    def _add_keyframe_from_device(self, raw, rgb, global_T_frame):
        """The keyframe from device images of the cameras' sizes (both are freed)."""
        ctx, lib, h = self.ctx, self.lib, self.ctx.handle
        W, H = self.depth_cam.width, self.depth_cam.height
        cw, ch = self.color_cam.width, self.color_cam.height
        kf = dict(depth=DeviceBuffer2D(ctx, H, W, np.uint16), normals=DeviceBuffer2D(ctx, H, W, np.uint16),
                  radius=DeviceBuffer2D(ctx, H, W, np.uint16).clear(0), color=DeviceBuffer2D(ctx, ch, cw, np.uint8, 4),
                  pose=np.asarray(global_T_frame, dtype=np.float32).copy(), activation=capi.KF_ACTIVE)
        capi.check(lib.bahip_compute_brightness(h, rgb.ptr, rgb.pitch, kf["color"].ptr, kf["color"].pitch, cw, ch))
        tmp = DeviceBuffer2D(ctx, H, W, np.uint16)
        capi.check(lib.bahip_compute_normals(h, C.byref(self.depth_cam), C.byref(self.dp), raw.ptr, raw.pitch, tmp.ptr, tmp.pitch,
                                             kf["normals"].ptr, kf["normals"].pitch))
        capi.check(lib.bahip_compute_point_radii_and_remove_isolated_pixels(
            h, C.byref(self.depth_cam), self.dp.raw_to_float_depth, tmp.ptr, tmp.pitch, kf["radius"].ptr, kf["radius"].pitch,
            kf["depth"].ptr, kf["depth"].pitch))
        mn, mx = C.c_float(), C.c_float()
        capi.check(lib.bahip_compute_min_max_depth(h, tmp.ptr, tmp.pitch, W, H, self.dp.raw_to_float_depth, C.byref(mn), C.byref(mx)))
        kf["min_depth"], kf["max_depth"] = mn.value, mx.value
        ctx.synchronize()
        for b in (rgb, raw, tmp):
            b.free()
        self.keyframes.append(kf)
        return len(self.keyframes) - 1

    def add_frame(self, depth_full, rgb_full, global_T_frame, pyramid_level_for_depth=0, pyramid_level_for_color=0, median_iterations=0,
                  bilateral=None):
        """BadSlam::PreprocessFrame (B/bad_slam.cc:657-706) + the keyframe constructor on a full-resolution frame: raw depth (0 = no
        measurement) through `median_iterations` rounds of the median filter and densification or, at a depth level > 0, the median
        downscale to the depth camera's size; colour halved `pyramid_level_for_color` times to the colour camera's size; then, with
        bilateral = (sigma_xy, sigma_inv_depth, radius_factor, max_depth_raw), the bilateral filter and depth cut-off; then what
        add_keyframe does.  All on the device.  The scene's cameras are the scaled ones (scaled_camera)."""
        ctx, lib, h = self.ctx, self.lib, self.ctx.handle
        ld, lc, iterations = int(pyramid_level_for_depth), int(pyramid_level_for_color), int(median_iterations)
        if not (0 <= ld <= 3 and 0 <= lc <= 3):
            raise ValueError("pyramid levels are 0 .. 3")
        if ld > 0 and iterations > 0:
            raise ValueError("Simultaneous downscaling and median filtering of depth maps is not implemented.")
        d = np.ascontiguousarray(depth_full, np.uint16)
        c = np.ascontiguousarray(rgb_full, np.uint8)
        W, H = self.depth_cam.width, self.depth_cam.height
        cw, ch = self.color_cam.width, self.color_cam.height
        scale = lambda size, level: int(float(np.float32(1.0) / np.float32(1 << level)) * size + 0.5)
        if (scale(d.shape[1], ld), scale(d.shape[0], ld)) != (W, H):
            raise ValueError(f"a {d.shape[1]} x {d.shape[0]} depth image at level {ld} is not the depth camera's {W} x {H}")
        if (scale(c.shape[1], lc), scale(c.shape[0], lc)) != (cw, ch):
            raise ValueError(f"a {c.shape[1]} x {c.shape[0]} colour image at level {lc} is not the colour camera's {cw} x {ch}")
        raw = DeviceBuffer2D(ctx, d.shape[0], d.shape[1], np.uint16).upload(d)
        if iterations > 0:
            other = DeviceBuffer2D(ctx, H, W, np.uint16)
            for _ in range(iterations):
                capi.check(lib.bahip_median_filter_and_densify(h, raw.ptr, raw.pitch, other.ptr, other.pitch, W, H))
                raw, other = other, raw
            ctx.synchronize()
            other.free()
        if ld > 0:
            small = DeviceBuffer2D(ctx, H, W, np.uint16)
            capi.check(lib.bahip_downscale_depth_median(h, raw.ptr, raw.pitch, d.shape[1], d.shape[0], small.ptr, small.pitch, W, H))
            ctx.synchronize()
            raw.free()
            raw = small
        rgb = DeviceBuffer2D(ctx, c.shape[0], c.shape[1], np.uint8, 3).upload(c)
        if lc > 0:
            small = DeviceBuffer2D(ctx, ch, cw, np.uint8, 3)
            capi.check(lib.bahip_downscale_rgb_half(h, rgb.ptr, rgb.pitch, c.shape[1], c.shape[0], lc, small.ptr, small.pitch))
            ctx.synchronize()
            rgb.free()
            rgb = small
        if bilateral is not None:
            sigma_xy, sigma_value, radius_factor, max_depth = bilateral
            filtered = DeviceBuffer2D(ctx, H, W, np.uint16)
            capi.check(lib.bahip_bilateral_filtering_and_depth_cutoff(h, sigma_xy, sigma_value, radius_factor, int(max_depth),
                                                                      self.dp.raw_to_float_depth, raw.ptr, raw.pitch, filtered.ptr,
                                                                      filtered.pitch, W, H))
            ctx.synchronize()
            raw.free()
            raw = filtered
        return self._add_keyframe_from_device(raw, rgb, global_T_frame)

    def frame_struct(self, i):
        kf = self.keyframes[i]
        return capi.Frame(kf["depth"].ptr, kf["depth"].pitch, kf["normals"].ptr, kf["normals"].pitch,
                          kf["radius"].ptr, kf["radius"].pitch, kf["color"].ptr, kf["color"].pitch)

    def set_sum_classes(self, classes):
        """4 (default) or 8 interleaved keyframe classes in the per-surfel sums (bahip_context_set_sum_classes)."""
        capi.check(self.lib.bahip_context_set_sum_classes(self.ctx.handle, int(classes)))

    def set_intrinsics_sum_classes(self, classes):
        """1 (default), 2, 4 or 8 keyframe classes in the global sums of the intrinsics step (bahip_context_set_intrinsics_sum_classes)."""
        capi.check(self.lib.bahip_context_set_intrinsics_sum_classes(self.ctx.handle, int(classes)))

    def set_pcg_sum_classes(self, classes):
        """1 (default), 2, 4 or 8 keyframe classes in the surfel block of the PCG scheme's r, M and g (bahip_context_set_pcg_sum_classes)."""
        capi.check(self.lib.bahip_context_set_pcg_sum_classes(self.ctx.handle, int(classes)))

    def read_intrinsics_sums(self, with_cells=True):
        """The last intrinsics step's sums rounded to binary32 (bahip_debug_read_intrinsics_sums): (glob[34], cells[S, 8] or None)."""
        glob = np.zeros(34, np.float32)
        cells = np.zeros((self.cf_w * self.cf_h, 8), np.float32) if with_cells else None
        capi.check(self.lib.bahip_debug_read_intrinsics_sums(self.ctx.handle, glob.ctypes.data_as(C.POINTER(C.c_float)),
                                                              cells.ctypes.data_as(C.POINTER(C.c_float)) if with_cells else None))
        return glob, cells

    def set_lifecycle_dealing(self, enabled):
        """Deal the lifecycle calls of a whole-cloud phase (between bahip_gather_surfel_shards over world >= 2 ranks and the extract)
        over that surfel partition (bahip_context_set_lifecycle_dealing)."""
        capi.check(self.lib.bahip_context_set_lifecycle_dealing(self.ctx.handle, int(bool(enabled))))

    def lifecycle_deal_stats(self, reset=True):
        """[creation keyframes swept, sum of their index + 1, merge keyframes swept, sum of their index + 1, deletion surfels swept,
        dealt calls, creation candidates exchanged, merge pairs exchanged] of this rank since the last reset
        (bahip_debug_lifecycle_deal_stats)."""
        out = (C.c_longlong * 8)()
        capi.check(self.lib.bahip_debug_lifecycle_deal_stats(self.ctx.handle, out, int(bool(reset))))
        return [int(v) for v in out]

    def set_keyframe_sharding(self, rank, world):
        """Keyframe k lives on rank k % world (bahip_context_set_keyframe_sharding); bind_keyframes then hands over the
        images of this rank's keyframes only (null pointers for the others: the backend must not look at them)."""
        capi.check(self.lib.bahip_context_set_keyframe_sharding(self.ctx.handle, int(rank), int(world)))
        self.kf_shard = (int(rank), int(world))

    def bind_keyframes(self):
        arr = (capi.Keyframe * max(1, len(self.keyframes)))()
        rank, world = getattr(self, "kf_shard", (0, 1))
        for i, kf in enumerate(self.keyframes):
            arr[i].frame = self.frame_struct(i) if i % world == rank else capi.Frame()
            for c in range(7):
                arr[i].global_T_frame[c] = float(kf["pose"][c])
            arr[i].activation = int(kf["activation"])
        capi.check(self.lib.bahip_set_keyframes(self.ctx.handle, arr, len(self.keyframes)))

    def read_keyframe_activations(self):
        """The activation (capi.KF_*) of every bound keyframe as the DEVICE table holds it now, after waiting for the stream
        (bahip_debug_read_keyframe_activations): what the window, the co-visible propagation and the pose phase left there."""
        K = len(self.keyframes)
        out = (C.c_int * max(1, K))()
        capi.check(self.lib.bahip_debug_read_keyframe_activations(self.ctx.handle, out, K))
        return [int(v) for v in out[:K]]

    def _supporting_ptrs(self):
        return (C.c_void_p * capi.MERGE_BUFFER_COUNT)(*[b.ptr for b in self.supporting])

    def create_surfels_for_keyframe(self, i, filter_new_surfels=False, min_observation_count=2, covis=None):
        self.bind_keyframes()
        if covis is None:
            covis = [j for j in range(len(self.keyframes)) if j != i]
        cv = (C.c_int * max(1, len(covis)))(*covis)
        n = C.c_uint32()
        s = self.surfels_struct()
        capi.check(self.lib.bahip_create_surfels_for_keyframe(self.ctx.handle, i, int(filter_new_surfels), int(min_observation_count),
                                                              cv, len(covis), C.byref(s), self._supporting_ptrs(),
                                                              self.supporting[0].pitch, C.byref(n)))
        self.surfels_size += n.value
        self.surfel_count += n.value
        return n.value

    def create_surfels_for_keyframes(self, plan, filter_new_surfels=False, min_observation_count=2):
        """bahip_create_surfels_for_keyframes; plan = [(keyframe index, co-visible keyframe indices or None for all others), ...]."""
        self.bind_keyframes()
        ids, offsets, covis = [], [0], []
        for i, cv in plan:
            ids.append(i)
            covis += [j for j in range(len(self.keyframes)) if j != i] if cv is None else list(cv)
            offsets.append(len(covis))
        n = C.c_uint32()
        s = self.surfels_struct()
        capi.check(self.lib.bahip_create_surfels_for_keyframes(self.ctx.handle, (C.c_int * len(ids))(*ids), len(ids), int(filter_new_surfels),
                                                               int(min_observation_count), (C.c_int * len(offsets))(*offsets),
                                                               (C.c_int * max(1, len(covis)))(*covis), C.byref(s), self._supporting_ptrs(),
                                                               self.supporting[0].pitch, C.byref(n)))
        self.surfels_size += n.value
        self.surfel_count += n.value
        return n.value

    @contextlib.contextmanager
    def lifecycle_batch(self, keyframes=None, frames=None):
        """bahip_lifecycle_batch_begin / _end around the creations or merges of a batch of keyframes; keyframes (bound indices) or
        frames (frame_T_global 3x4 each): the batch knows its frames and keeps a list of visible tiles for each."""
        s = self.surfels_struct()
        capi.check(self.lib.bahip_lifecycle_batch_begin(self.ctx.handle, C.byref(s)))
        if keyframes is not None:
            self.bind_keyframes()
            capi.check(self.lib.bahip_lifecycle_batch_set_keyframes(self.ctx.handle, (C.c_int * max(1, len(keyframes)))(*keyframes), len(keyframes)))
        if frames is not None:
            flat = [float(v) for F in frames for v in F]
            capi.check(self.lib.bahip_lifecycle_batch_set_frames(self.ctx.handle, (C.c_float * max(1, len(flat)))(*flat), len(frames)))
        try:
            yield
        finally:
            capi.check(self.lib.bahip_lifecycle_batch_end(self.ctx.handle))

    def determine_supporting_surfels(self, i, frame_T_global, merge=False, merge_dist_factor=0.8):
        """DetermineSupportingSurfels[AndMergeSurfels]CUDA for keyframe i; returns (the three supporting planes restricted to
        the sparse-cell grid, number of surfels deleted by merging)."""
        F = (C.c_float * 12)(*[float(v) for v in frame_T_global])
        merged = C.c_uint32()
        fr, s = self.frame_struct(i), self.surfels_struct()
        capi.check(self.lib.bahip_determine_supporting_surfels(self.ctx.handle, int(merge), float(merge_dist_factor), C.byref(fr), F,
                                                               C.byref(s), self._supporting_ptrs(), self.supporting[0].pitch,
                                                               C.byref(merged)))
        self.ctx.synchronize()
        self.surfel_count -= merged.value
        planes = np.stack([b.download()[:self.cf_h, :self.cf_w] for b in self.supporting])
        return planes, merged.value

    def merge_surfels_for_keyframes(self, keyframes, frames_T_global, merge_dist_factor=0.8):
        """bahip_merge_surfels_for_keyframes: the merges of a batch of keyframes, pipelined (two dependent launches per keyframe);
        returns (the three supporting planes afterwards -- left empty --, surfels merged away)."""
        n = len(keyframes)
        structs = (capi.Frame * n)(*[self.frame_struct(k) for k in keyframes])
        F = (C.c_float * (12 * n))(*[float(v) for T in frames_T_global for v in T])
        merged = C.c_uint32()
        s = self.surfels_struct()
        capi.check(self.lib.bahip_merge_surfels_for_keyframes(self.ctx.handle, float(merge_dist_factor), structs, F, n, C.byref(s),
                                                              self._supporting_ptrs(), self.supporting[0].pitch, C.byref(merged)))
        self.ctx.synchronize()
        self.surfel_count -= merged.value
        planes = np.stack([b.download()[:self.cf_h, :self.cf_w] for b in self.supporting])
        return planes, merged.value

    def merge_surfels_for_bound_keyframes(self, keyframes, merge_dist_factor=0.8):
        """bahip_merge_surfels_for_bound_keyframes: the merges of a batch of bound keyframes, named by index (the keyframes as last bound);
        returns (the three supporting planes afterwards -- left empty --, surfels merged away)."""
        n = len(keyframes)
        merged = C.c_uint32()
        s = self.surfels_struct()
        capi.check(self.lib.bahip_merge_surfels_for_bound_keyframes(self.ctx.handle, float(merge_dist_factor), (C.c_int * max(1, n))(*keyframes), n,
                                                                    C.byref(s), self._supporting_ptrs(), self.supporting[0].pitch, C.byref(merged)))
        self.ctx.synchronize()
        self.surfel_count -= merged.value
        planes = np.stack([b.download()[:self.cf_h, :self.cf_w] for b in self.supporting])
        return planes, merged.value

    def delete_surfels_and_update_radii(self, min_observation_count):
        deleted = C.c_uint32()
        s = self.surfels_struct()
        capi.check(self.lib.bahip_delete_surfels_and_update_radii(self.ctx.handle, int(min_observation_count), C.byref(s), C.byref(deleted)))
        self.surfel_count -= deleted.value
        return deleted.value

    def compact_surfels(self, with_active=True):
        s = self.surfels_struct()
        if not with_active:
            s.active = None
        capi.check(self.lib.bahip_compact_surfels(self.ctx.handle, self.surfel_count, C.byref(s)))
        self.surfels_size = self.surfel_count

    def download_surfels(self):
        self.ctx.synchronize()
        return self.surfel_buf.download()[:, :self.surfels_size]

    def upload_surfels(self, data, active=None):
        full = np.zeros((capi.SURFEL_ATTRIBUTE_COUNT, self.capacity), np.float32)
        n = data.shape[1]
        full[:data.shape[0], :n] = data
        self.surfel_buf.upload(full)
        self.surfels_size = self.surfel_count = n
        if active is not None:
            a = np.zeros((1, self.capacity), np.uint8)
            a[0, :n] = active
            self.active_buf.upload(a)

    def accumulate_pose_coeffs(self, i, use_depth, use_desc, frame_T_global):
        F = (C.c_float * 12)(*[float(v) for v in frame_T_global])
        H, b = (C.c_float * 21)(), (C.c_float * 6)()
        fr, s = self.frame_struct(i), self.surfels_struct()
        capi.check(self.lib.bahip_accumulate_pose_estimation_coeffs(self.ctx.handle, int(use_depth), int(use_desc), C.byref(fr), F,
                                                                    C.byref(s), H, b))
        return np.array(list(H)), np.array(list(b))

    def estimate_frame_pose(self, i, use_depth, use_desc, init_pose):
        init = (C.c_float * 7)(*[float(v) for v in init_pose])
        out = (C.c_float * 7)()
        its, conv = C.c_int(), C.c_int()
        fr, s = self.frame_struct(i), self.surfels_struct()
        capi.check(self.lib.bahip_estimate_frame_pose(self.ctx.handle, int(use_depth), int(use_desc), C.byref(fr), init, C.byref(s),
                                                      out, C.byref(its), C.byref(conv)))
        return np.array(list(out), dtype=np.float64), its.value, bool(conv.value)

    def update_surfel_activation(self):
        s = self.surfels_struct()
        capi.check(self.lib.bahip_update_surfel_activation(self.ctx.handle, C.byref(s), self.surfels_size))

    def assign_colors(self):
        s = self.surfels_struct()
        capi.check(self.lib.bahip_assign_colors(self.ctx.handle, C.byref(s)))

    def optimize_geometry_iteration(self, use_depth, use_desc):
        s = self.surfels_struct()
        capi.check(self.lib.bahip_optimize_geometry_iteration(self.ctx.handle, int(use_depth), int(use_desc), C.byref(s)))

    def update_activation_and_optimize_geometry(self, use_depth, use_desc, activation_surfels_size=None):
        s = self.surfels_struct()
        n = self.surfels_size if activation_surfels_size is None else int(activation_surfels_size)
        capi.check(self.lib.bahip_update_activation_and_optimize_geometry(self.ctx.handle, int(use_depth), int(use_desc), C.byref(s), n))

    GEOMETRY_STEP_CONTROL = dict(lambda_initial=0.0, lambda_up=4.0, lambda_min=1.0, lambda_max=1e4, max_trials=4, guard_pairs=1)

    def optimize_geometry_controlled(self, use_depth=True, use_desc=True, control=None, activation_surfels_size=None, want_outcome=True,
                                     want_stats=True, prefill=0xEE):
        """One geometry step of the alternating scheme under step control (bahip_optimize_geometry_iteration_controlled).  control: a
        dict overriding fields of GEOMETRY_STEP_CONTROL (the defaults of DirectBA::GeometryStepControl); activation_surfels_size: None
        = the flags are kept (-1), else the range the normals pass decides.  Returns (outcome, stats): outcome a uint8 array of
        surfels_size entries (its device buffer filled with the byte `prefill` first: an entry the call did not write shows) or None,
        stats a dict of the fields of bahip_geometry_step_stats or None."""
        fields = dict(self.GEOMETRY_STEP_CONTROL)
        fields.update(control or {})
        ctl = capi.GeometryStepControl(float(fields["lambda_initial"]), float(fields["lambda_up"]), float(fields["lambda_min"]),
                                       float(fields["lambda_max"]), int(fields["max_trials"]), int(fields["guard_pairs"]))
        n = self.surfels_size
        buf = DeviceBuffer2D(self.ctx, 1, max(1, n), np.uint8) if want_outcome else None
        stats = capi.GeometryStepStats() if want_stats else None
        try:
            if buf is not None:
                buf.clear(prefill)
            s = self.surfels_struct()
            capi.check(self.lib.bahip_optimize_geometry_iteration_controlled(
                self.ctx.handle, int(use_depth), int(use_desc), C.byref(ctl), C.byref(s),
                -1 if activation_surfels_size is None else int(activation_surfels_size), buf.ptr if buf is not None else None,
                C.byref(stats) if stats is not None else None))
            self.ctx.synchronize()
            outcome = buf.download()[0, :n].copy() if buf is not None else None
        finally:
            if buf is not None:
                buf.free()
        return outcome, ({name: int(getattr(stats, name)) for name, _ in capi.GeometryStepStats._fields_} if stats is not None else None)

    def read_geometry_sums(self, count):
        """The per-surfel totals the last controlled geometry step consumed (bahip_debug_read_geometry_sums): (count, surfels_size)
        binary32, count = 2 depth-only (H, b) or 8 (a0 a1 a2 a3 a5 a6 a7 a8)."""
        out = np.zeros((8, self.surfels_size), np.float32)   # (room for either count: the call writes what the step consumed)
        capi.check(self.lib.bahip_debug_read_geometry_sums(self.ctx.handle, out.ctypes.data_as(C.POINTER(C.c_float))))
        return out[:int(count)].copy()

    def estimate_keyframe_poses(self, use_depth, use_desc):
        K = len(self.keyframes)
        poses = (C.c_float * (7 * K))()
        its, conv = (C.c_int * K)(), (C.c_int * K)()
        rounds = C.c_int()
        s = self.surfels_struct()
        capi.check(self.lib.bahip_estimate_keyframe_poses(self.ctx.handle, int(use_depth), int(use_desc), C.byref(s), poses, its, conv,
                                                          C.byref(rounds)))
        return (np.array(list(poses), dtype=np.float64).reshape(K, 7), np.array(list(its)), np.array(list(conv)), rounds.value)

    def estimate_keyframe_poses_controlled(self, lambdas, control, use_depth=True, use_desc=True, update_activation=False):
        """The pose phase under step control (bahip_estimate_keyframe_poses_controlled): `lambdas` = the damping factor per bound keyframe,
        `control` = (lambda_up, lambda_down, lambda_min, lambda_max, max_trials).  Adopts the poses the call leaves.  Returns a dict of
        arrays in bound order -- poses (binary32, K x 7), lambdas, iterations, converged, moved, trials, rejected -- the lists
        cost_before / cost_after (dicts like evaluate_cost's), and rounds, num_converged."""
        K = len(self.keyframes)
        up, down, lo, hi, trials = control
        ctl = capi.PoseStepControl(float(up), float(down), float(lo), float(hi), int(trials))
        lam = (C.c_float * max(1, K))(*[float(v) for v in lambdas])
        poses = (C.c_float * (7 * max(1, K)))()
        its, conv, moved, ran, rejected = ((C.c_int * max(1, K))() for _ in range(5))
        before, after = (capi.Cost * max(1, K))(), (capi.Cost * max(1, K))()
        rounds, num_converged = C.c_int(), C.c_int()
        s = self.surfels_struct()
        capi.check(self.lib.bahip_estimate_keyframe_poses_controlled(self.ctx.handle, int(use_depth), int(use_desc), C.byref(ctl), C.byref(s),
                                                                     int(update_activation), lam, poses, its, conv, moved, ran, rejected,
                                                                     before, after, C.byref(rounds), C.byref(num_converged)))
        arr = np.array(list(poses), dtype=np.float32).reshape(-1, 7)[:K]
        for k, kf in enumerate(self.keyframes):
            kf["pose"] = arr[k].copy()
        ints = lambda a: np.array(list(a), dtype=np.int64)[:K]
        return {"poses": arr, "lambdas": np.array(list(lam), dtype=np.float32)[:K], "iterations": ints(its), "converged": ints(conv),
                "moved": ints(moved), "trials": ints(ran), "rejected": ints(rejected), "cost_before": [cost_dict(c) for c in before[:K]],
                "cost_after": [cost_dict(c) for c in after[:K]], "rounds": rounds.value, "num_converged": num_converged.value}

    def update_surfel_normals(self):
        s = self.surfels_struct()
        capi.check(self.lib.bahip_update_surfel_normals(self.ctx.handle, C.byref(s)))

    def sort_surfels_spatially(self, grid_cell_size=0.02):
        s = self.surfels_struct()
        capi.check(self.lib.bahip_sort_surfels_spatially(self.ctx.handle, C.byref(s), float(grid_cell_size)))

    def optimize_intrinsics(self, optimize_depth, optimize_color, apply=True):
        """OptimizeIntrinsicsCUDA; with apply=True the new cameras / a are adopted like
        B/direct_ba_alternating.cc:609-619 does."""
        cc, dc, a = capi.Camera(), capi.Camera(), C.c_float()
        s = self.surfels_struct()
        capi.check(self.lib.bahip_optimize_intrinsics(self.ctx.handle, int(optimize_depth), int(optimize_color), C.byref(s),
                                                      C.byref(cc), C.byref(dc), C.byref(a)))
        if apply and self.surfels_size > 0:
            if optimize_color:
                self.color_cam = cc
            if optimize_depth:
                self.depth_cam = dc
                self.dp.a = a.value
            self.set_intrinsics()
        return cc, dc, a.value

    INTRINSICS_STEP_CONTROL = dict(lambda_first=1.0, lambda_up=4.0, lambda_max=1e4, max_trials=4)

    def optimize_intrinsics_controlled(self, lam, optimize_depth=True, optimize_color=True, use_depth=True, use_desc=True, control=None,
                                       cost_before=None):
        """One intrinsics step of the alternating scheme under step control (bahip_optimize_intrinsics_controlled) starting at the
        damping factor `lam`; control: a dict overriding fields of INTRINSICS_STEP_CONTROL (the defaults of
        DirectBA::IntrinsicsStepControl); cost_before: a capi.Cost of the current state, or None to have it evaluated.  Adopts the
        cameras and a the call leaves (the context keeps them itself).  Returns a dict: lam (the next call's), accepted, trials,
        lambda_accepted, color_camera / depth_camera (fx, fy, cx, cy as binary32), a (binary32), cost_before, cost_after (dicts like
        evaluate_cost's) and cost_after_struct (to pass on as the next call's cost_before)."""
        fields = dict(self.INTRINSICS_STEP_CONTROL)
        fields.update(control or {})
        ctl = capi.IntrinsicsStepControl(float(fields["lambda_first"]), float(fields["lambda_up"]), float(fields["lambda_max"]),
                                         int(fields["max_trials"]))
        cc, dc, a = capi.Camera(), capi.Camera(), C.c_float()
        ran, accepted = C.c_int(), C.c_int()
        lam_io, lam_accepted = C.c_float(float(lam)), C.c_float()
        before = capi.Cost() if cost_before is None else cost_before
        after = capi.Cost()
        s = self.surfels_struct()
        capi.check(self.lib.bahip_optimize_intrinsics_controlled(
            self.ctx.handle, int(optimize_depth), int(optimize_color), int(use_depth), int(use_desc), C.byref(ctl), C.byref(s),
            C.byref(lam_io), C.byref(cc), C.byref(dc), C.byref(a), int(cost_before is not None), C.byref(before), C.byref(after),
            C.byref(ran), C.byref(accepted), C.byref(lam_accepted)))
        if accepted.value:
            if optimize_color:
                self.color_cam = cc
            if optimize_depth:
                self.depth_cam = dc
                self.dp.a = a.value
        cam = lambda c: np.array([c.fx, c.fy, c.cx, c.cy], np.float32)
        return {"lam": float(lam_io.value), "accepted": bool(accepted.value), "trials": ran.value,
                "lambda_accepted": float(lam_accepted.value), "color_camera": cam(cc), "depth_camera": cam(dc),
                "a": np.float32(a.value), "cost_before": cost_dict(before), "cost_after": cost_dict(after), "cost_after_struct": after}

    def intrinsics_solve_damped(self, lam, optimize_depth=True, optimize_color=True, with_cells=True):
        """The damped solves from the sums of the last intrinsics step (bahip_debug_intrinsics_solve_damped); nothing is applied.
        Returns (x1[5], xc[4], cells[S, 8] or None) in binary32."""
        x1, xc = np.zeros(5, np.float32), np.zeros(4, np.float32)
        cells = np.zeros((self.cf_w * self.cf_h, 8), np.float32) if with_cells and optimize_depth else None
        fp = lambda arr: arr.ctypes.data_as(C.POINTER(C.c_float))
        capi.check(self.lib.bahip_debug_intrinsics_solve_damped(self.ctx.handle, int(optimize_depth), int(optimize_color), float(lam),
                                                                 fp(x1), fp(xc), fp(cells) if cells is not None else None))
        return x1, xc, cells

    def intrinsics_trial_timing(self, enable):
        """Switches the host wall-clock split of the controlled intrinsics step on or off and returns the last call's (milliseconds:
        sweep, cost sweeps, solves + back-substitution + restore, waits for the read-backs; bahip_debug_intrinsics_trial_timing)."""
        out = (C.c_double * 4)()
        capi.check(self.lib.bahip_debug_intrinsics_trial_timing(self.ctx.handle, int(bool(enable)), out))
        return [float(v) for v in out]

    def pcg_iteration(self, optimize_poses=True, optimize_geometry=True, optimize_depth_intrinsics=False,
                      optimize_color_intrinsics=False, use_depth=True, use_desc=True, max_inner_iterations=30, gauge_keyframe=0,
                      windowed=False):
        """One outer iteration of the PCG scheme on the bound keyframes; adopts new poses / intrinsics.  windowed: over the active
        keyframe window of the device table and the active surfels (bahip_pcg_iteration_windowed)."""
        opt = capi.PCGOptions(int(optimize_poses), int(optimize_geometry), int(optimize_depth_intrinsics),
                              int(optimize_color_intrinsics), int(use_depth), int(use_desc), int(max_inner_iterations),
                              int(gauge_keyframe))
        cc, dc, a = capi.Camera(), capi.Camera(), C.c_float()
        steps, conv = C.c_int(), C.c_int()
        s = self.surfels_struct()
        fn = self.lib.bahip_pcg_iteration_windowed if windowed else self.lib.bahip_pcg_iteration
        capi.check(fn(self.ctx.handle, C.byref(opt), C.byref(s), C.byref(cc), C.byref(dc), C.byref(a), C.byref(steps), C.byref(conv)))
        K = len(self.keyframes)
        if optimize_poses and K:
            poses = (C.c_float * (7 * K))()
            capi.check(self.lib.bahip_get_keyframe_poses(self.ctx.handle, poses, K))
            arr = np.array(list(poses), dtype=np.float32).reshape(K, 7)
            for k, kf in enumerate(self.keyframes):
                kf["pose"] = arr[k].copy()
        if optimize_color_intrinsics:
            self.color_cam = cc
        if optimize_depth_intrinsics:
            self.depth_cam = dc
            self.dp.a = a.value
        if optimize_color_intrinsics or optimize_depth_intrinsics:
            self.set_intrinsics()
        return steps.value, conv.value

    def set_pcg_damping(self, lam):
        """The damping factor of the PCG system (bahip_context_set_pcg_damping); 0 = off."""
        capi.check(self.lib.bahip_context_set_pcg_damping(self.ctx.handle, float(lam)))

    def pcg_iteration_controlled(self, lam, control, optimize_poses=True, optimize_geometry=True, optimize_depth_intrinsics=False,
                                 optimize_color_intrinsics=False, use_depth=True, use_desc=True, max_inner_iterations=30,
                                 gauge_keyframe=0, windowed=False, update_normals=False, cost_before=None):
        """One controlled outer iteration (bahip_pcg_iteration_controlled) with damping `lam`; `control` = (lambda_up, lambda_down,
        lambda_min, lambda_max, max_trials); cost_before: a capi.Cost of the current state, or None to have it evaluated.  Adopts the
        poses / intrinsics the call leaves.  Returns a dict: lam, accepted, trials, steps, converged, cost_before, cost_after (dicts
        like evaluate_cost's) and cost_after_struct (to pass on as the next call's cost_before)."""
        opt = capi.PCGOptions(int(optimize_poses), int(optimize_geometry), int(optimize_depth_intrinsics),
                              int(optimize_color_intrinsics), int(use_depth), int(use_desc), int(max_inner_iterations),
                              int(gauge_keyframe))
        up, down, lo, hi, trials = control
        ctl = capi.PCGStepControl(float(lam), float(up), float(down), float(lo), float(hi), int(trials))
        cc, dc, a = capi.Camera(), capi.Camera(), C.c_float()
        steps, conv, ran, accepted = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        lam_io = C.c_float(float(lam))
        before = capi.Cost() if cost_before is None else cost_before
        after = capi.Cost()
        s = self.surfels_struct()
        capi.check(self.lib.bahip_pcg_iteration_controlled(self.ctx.handle, C.byref(opt), C.byref(ctl), int(windowed), int(update_normals),
                                                           C.byref(s), C.byref(lam_io), C.byref(cc), C.byref(dc), C.byref(a),
                                                           C.byref(steps), C.byref(conv), int(cost_before is not None),
                                                           C.byref(before), C.byref(after), C.byref(ran), C.byref(accepted)))
        K = len(self.keyframes)
        if optimize_poses and K:
            poses = (C.c_float * (7 * K))()
            capi.check(self.lib.bahip_get_keyframe_poses(self.ctx.handle, poses, K))
            arr = np.array(list(poses), dtype=np.float32).reshape(K, 7)
            for k, kf in enumerate(self.keyframes):
                kf["pose"] = arr[k].copy()
        if optimize_color_intrinsics:
            self.color_cam = cc
        if optimize_depth_intrinsics:
            self.depth_cam = dc
            self.dp.a = a.value
        return {"lam": float(lam_io.value), "accepted": bool(accepted.value), "trials": ran.value, "steps": steps.value,
                "converged": conv.value, "cost_before": cost_dict(before), "cost_after": cost_dict(after), "cost_after_struct": after}

    def read_pcg_vector(self, which, count, offset=0):
        out = np.zeros(count, np.float32)
        capi.check(self.lib.bahip_debug_read_pcg_vector(self.ctx.handle, int(which), int(offset), int(count),
                                                        out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def evaluate_cost(self, use_depth=True, use_desc=True, per_keyframe=True):
        """The value of the BA objective over the bound keyframes (bahip_evaluate_cost): (total, per-keyframe list or None), each a
        dict of the three exactly summed costs (binary64) and the two counts.  Call bind_keyframes first."""
        s = self.surfels_struct()
        total = capi.Cost()
        per = (capi.Cost * max(1, len(self.keyframes)))() if per_keyframe else None
        capi.check(self.lib.bahip_evaluate_cost(self.ctx.handle, int(use_depth), int(use_desc), C.byref(s), C.byref(total), per))
        return cost_dict(total), ([cost_dict(c) for c in per[:len(self.keyframes)]] if per_keyframe else None)

    def evaluate_frame_cost(self, i, frame_T_global, use_depth=True, use_desc=True):
        """The same for keyframe i's images at an arbitrary frame_T_global (12 floats; bahip_evaluate_frame_cost)."""
        F = (C.c_float * 12)(*[float(v) for v in frame_T_global])
        fr, s = self.frame_struct(i), self.surfels_struct()
        out = capi.Cost()
        capi.check(self.lib.bahip_evaluate_frame_cost(self.ctx.handle, int(use_depth), int(use_desc), C.byref(fr), F, C.byref(s), C.byref(out)))
        return cost_dict(out)

    SURFEL_COST_PLANES = (("depth", np.float64), ("descriptor_1", np.float64), ("descriptor_2", np.float64),
                          ("depth_residuals", np.uint32), ("descriptor_pairs", np.uint32))

    def evaluate_surfel_costs(self, use_depth=True, use_desc=True, planes=None, prefill=None):
        """The value of the BA objective per surfel over the bound keyframes (bahip_evaluate_surfel_costs): a dict of five numpy arrays
        of surfels_size entries in buffer order -- depth, descriptor_1, descriptor_2 (float64, exact sums) and depth_residuals,
        descriptor_pairs (uint32).  planes: the names to ask for (the others are passed as NULL and left out of the dict); prefill: a
        byte value the device planes are filled with before the call (tests: an entry the call did not write shows).  Call
        bind_keyframes first."""
        n = self.surfels_size
        wanted = [name for name, _ in self.SURFEL_COST_PLANES] if planes is None else list(planes)
        bufs = {name: DeviceBuffer2D(self.ctx, 1, max(1, n), dtype) for name, dtype in self.SURFEL_COST_PLANES if name in wanted}
        try:
            if prefill is not None:
                for b in bufs.values():
                    b.clear(prefill)
            s = self.surfels_struct()
            out = capi.SurfelCosts(*[bufs[name].ptr if name in bufs else None for name, _ in self.SURFEL_COST_PLANES])
            capi.check(self.lib.bahip_evaluate_surfel_costs(self.ctx.handle, int(use_depth), int(use_desc), C.byref(s), C.byref(out)))
            return {name: b.download()[0, :n].copy() for name, b in bufs.items()}
        finally:
            for b in bufs.values():
                b.free()

    RENDER_PLANES = (("key", np.uint64, 1), ("depth", np.float32, 1), ("index", np.uint32, 1), ("normal", np.float32, 3), ("color", np.uint8, 4))

    def render_surfels(self, view_cam, frame_T_global, options=None, planes=None, prefill=None):
        """The surfel buffer seen from the camera `view_cam` (capi.Camera) at frame_T_global (12 floats): bahip_render_surfels.  A dict
        of numpy arrays of the view's height x width pixels -- key (uint64), depth (float32), index (uint32), normal (x 3, float32),
        color (x 4, uint8).  options: a capi.RenderOptions (default: its defaults); planes: the names to ask for (the others are passed
        as NULL and left out of the dict); prefill: a byte value the device planes are filled with before the call (tests: an entry the
        call did not write shows).  Needs no bound keyframes."""
        w, h = int(view_cam.width), int(view_cam.height)
        n = max(1, w * h)
        wanted = [name for name, _, _ in self.RENDER_PLANES] if planes is None else list(planes)
        bufs = {name: DeviceBuffer2D(self.ctx, 1, n, dtype, channels) for name, dtype, channels in self.RENDER_PLANES if name in wanted}
        try:
            if prefill is not None:
                for b in bufs.values():
                    b.clear(prefill)
            F = (C.c_float * 12)(*[float(v) for v in frame_T_global])
            s = self.surfels_struct()
            opt = options if options is not None else capi.RenderOptions()
            out = capi.RenderOut(*[bufs[name].ptr if name in bufs else None for name, _, _ in self.RENDER_PLANES])
            capi.check(self.lib.bahip_render_surfels(self.ctx.handle, C.byref(s), C.byref(view_cam), F, C.byref(opt), C.byref(out)))
            shapes = {name: (h, w) if channels == 1 else (h, w, channels) for name, _, channels in self.RENDER_PLANES}
            return {name: b.download()[0, :w * h].reshape(shapes[name]).copy() for name, b in bufs.items()}
        finally:
            for b in bufs.values():
                b.free()

    def residual_image(self, k, frame_T_global, select=capi.RESIDUAL_BEST, index_base=0, planes=None, prefill=None, size=None):
        """Keyframe k's images against the surfel buffer at frame_T_global (12 floats), per pixel of the depth image the associated
        surfel with the smallest (select = capi.RESIDUAL_BEST) or largest (RESIDUAL_WORST) |depth residual| and its residuals:
        frame_residual_image on this scene's context, cameras and surfels (size: the first `size` surfels only)."""
        return frame_residual_image(self.ctx, self.frame_struct(k), frame_T_global, self.surfels_struct(size), self.depth_cam.width,
                                    self.depth_cam.height, select=select, index_base=index_base, planes=planes, prefill=prefill)

    def observed_covisibility(self, size=None, pitch=None, prefill=None):
        """The surfels every pair of bound keyframes shares (bahip_observed_covisibility) over the first `size` surfels (default: all):
        a (K, K) uint32 array in bound order, both triangles, the diagonal a keyframe's own pair count.  pitch: words per row of the
        device buffer (default K; the call refuses less) -- the result is then the whole (K, pitch) buffer; prefill: a byte value the
        buffer is filled with before the call (tests: a word the call did not write shows; after a refused call the buffer is the
        exception's `arrays` attribute).  Call bind_keyframes first."""
        K = len(self.keyframes)
        p = K if pitch is None else int(pitch)
        buf = DeviceBuffer2D(self.ctx, 1, max(1, K * max(p, 1)), np.uint32)
        try:
            buf.clear(0 if prefill is None else prefill)
            s = self.surfels_struct(size)
            try:
                capi.check(self.lib.bahip_observed_covisibility(self.ctx.handle, C.byref(s), buf.ptr, p))
            except capi.BackendError as e:
                self.ctx.synchronize()
                e.arrays = buf.download()[0].copy()
                raise
            self.ctx.synchronize()
            return buf.download()[0, :K * p].reshape(K, p).copy()
        finally:
            buf.free()

    RCS_STATS = ("list_entries", "pairs_visited", "atomics_issued", "degenerate_surfels", "overflow_tiles", "invalid")

    def reduced_camera_system(self, use_depth=True, use_desc=True, marginalise=True, size=None, pitch=None, prefill=None, planes=True):
        """The reduced camera system of the bound keyframes (bahip_reduced_camera_system) over the first `size` surfels (default: all):
        a dict with S (6K, 6K) and g (6K,) in binary64 -- the Gauss-Newton system over the poses with every surfel eliminated
        (marginalise=False: the block-diagonal pose equations) --, A (K, 6, 6) and b (K, 6) (planes=False: not asked for, None) and
        stats (RCS_STATS).  pitch: doubles per row of the device buffer of S (default 6K; the call refuses less) -- S is then the whole
        (6K, pitch) buffer; prefill: a byte value every buffer is filled with before the call (after a refused call the buffers are
        the exception's `arrays` attribute: S, g, A, b).  Call bind_keyframes first."""
        K = len(self.keyframes)
        n = 6 * K
        p = n if pitch is None else int(pitch)
        bufs = [DeviceBuffer2D(self.ctx, 1, max(1, n * max(p, 1)), np.float64), DeviceBuffer2D(self.ctx, 1, max(1, n), np.float64)]
        if planes:
            bufs += [DeviceBuffer2D(self.ctx, 1, max(1, 36 * K), np.float64), DeviceBuffer2D(self.ctx, 1, max(1, n), np.float64)]
        try:
            for buf in bufs:
                buf.clear(0 if prefill is None else prefill)
            s = self.surfels_struct(size)
            stats = (C.c_uint64 * 6)()
            try:
                capi.check(self.lib.bahip_reduced_camera_system(self.ctx.handle, int(bool(use_depth)), int(bool(use_desc)), int(bool(marginalise)),
                                                                C.byref(s), bufs[0].ptr, p, bufs[1].ptr, bufs[2].ptr if planes else None,
                                                                bufs[3].ptr if planes else None, stats))
            except capi.BackendError as e:
                self.ctx.synchronize()
                e.arrays = [buf.download()[0].copy() for buf in bufs]
                raise
            self.ctx.synchronize()
            return dict(S=bufs[0].download()[0, :n * p].reshape(n, p).copy(), g=bufs[1].download()[0, :n].copy(),
                        A=bufs[2].download()[0, :36 * K].reshape(K, 6, 6).copy() if planes else None,
                        b=bufs[3].download()[0, :n].reshape(K, 6).copy() if planes else None,
                        stats=dict(zip(self.RCS_STATS, (int(v) for v in stats))))
        finally:
            for buf in bufs:
                buf.free()

    def covisibility_census(self):
        """Of the last observed_covisibility: [(tile, keyframe) entries with a non-zero mask, atomic adds issued, tiles that took the
        overflow path] (bahip_debug_covisibility_census)."""
        out = (C.c_uint64 * 3)()
        capi.check(self.lib.bahip_debug_covisibility_census(self.ctx.handle, out))
        return [int(v) for v in out]

    def keyframe_observer_histogram(self, bins, prefill=None, size=None, pitch=None):
        """Per bound keyframe its surfels by the number of other keyframes that observe them (bahip_keyframe_observer_histogram) over
        the first `size` surfels (default: all): a (K, bins) uint32 array in bound order, column j the surfels with min(o, bins - 1) = j
        other observers.  pitch: words per row of the device buffer (default bins; the call refuses less) -- the result is then the
        whole (K, pitch) buffer; prefill: a byte value the buffer is filled with before the call (tests: a word the call did not write
        shows; after a refused call the buffer is the exception's `arrays` attribute).  Call bind_keyframes first."""
        K = len(self.keyframes)
        p = int(bins) if pitch is None else int(pitch)
        buf = DeviceBuffer2D(self.ctx, 1, max(1, K * max(p, 1)), np.uint32)
        try:
            buf.clear(0 if prefill is None else prefill)
            s = self.surfels_struct(size)
            try:
                capi.check(self.lib.bahip_keyframe_observer_histogram(self.ctx.handle, C.byref(s), int(bins), buf.ptr, p))
            except capi.BackendError as e:
                self.ctx.synchronize()
                e.arrays = buf.download()[0].copy()
                raise
            self.ctx.synchronize()
            return buf.download()[0, :K * p].reshape(K, p).copy()
        finally:
            buf.free()

    def redundancy_census(self):
        """Of the last keyframe_observer_histogram: [(tile, keyframe) entries with a non-zero mask, atomic adds issued, tiles that took
        a second traversal] (bahip_debug_redundancy_census)."""
        out = (C.c_uint64 * 3)()
        capi.check(self.lib.bahip_debug_redundancy_census(self.ctx.handle, out))
        return [int(v) for v in out]

    def tile_masks(self, size=None):
        """The tile mask table the last observed_covisibility, keyframe_observer_histogram or surfel_observations of this scene built
        (bahip_debug_read_tile_masks; under keyframe sharding, or on route 1 of set_observed_structure_route) over `size` surfels
        (default: all; the size that call was given): (tile_first, keyframes, masks) -- tiles + 1 uint32, and per entry a uint32
        keyframe index and a uint64 ballot, a tile's entries contiguous and ascending by keyframe."""
        entries = C.c_uint64(0)
        capi.check(self.lib.bahip_debug_read_tile_masks(self.ctx.handle, None, None, None, 0, C.byref(entries)))
        E = int(entries.value)
        first = np.zeros(((self.surfels_size if size is None else int(size)) + 63) // 64 + 1, np.uint32)
        keyframes, masks = np.zeros(max(1, E), np.uint32), np.zeros(max(1, E), np.uint64)
        capi.check(self.lib.bahip_debug_read_tile_masks(self.ctx.handle, first.ctypes.data, keyframes.ctypes.data, masks.ctypes.data, E,
                                                        C.byref(entries)))
        assert int(entries.value) == E and int(first[-1]) == E
        return first, keyframes[:E], masks[:E]

    def tile_mask_stats(self):
        """Of the last call on the table route (bahip_debug_tile_mask_stats): [entries this rank listed, entries of the merged table,
        exchanges, tiles whose reduction this rank ran, atomic adds, payload words written]."""
        out = (C.c_uint64 * 6)()
        capi.check(self.lib.bahip_debug_tile_mask_stats(self.ctx.handle, out))
        return [int(v) for v in out]

    OBSERVATION_PLANES = (("keyframes", np.uint16, 1), ("depth_raw", np.float32, 1), ("descriptor_raw", np.float32, 2))

    def surfel_observations(self, size=None, capacity=None, prefill=None, residuals=("depth_raw", "descriptor_raw"), keyframes=True):
        """The observation lists of the first `size` surfels (default: all) over the bound keyframes (bahip_surfel_observations): a
        dict with `pairs` (P), `surfel_first` (size + 1 uint32) and the device planes asked for, WHOLE -- `keyframes` (capacity uint16),
        `depth_raw` (capacity float32), `descriptor_raw` (capacity x 2 float32) -- of which the call fills the first P entries when
        P <= capacity.  capacity None: a count-only call sizes the planes (capacity = P).  keyframes False: the keyframes plane is
        passed as NULL (with residuals (): the count-only call).  residuals: the payload planes to ask for.  prefill: a byte value
        every device plane, surfel_first included, is filled with before the call (tests: a word the call did not write shows; after a
        refused call the planes are the exception's `arrays` attribute).  Call bind_keyframes first."""
        s = self.surfels_struct(size)
        n = int(s.surfels_size)
        pairs = C.c_uint64(0)
        first = DeviceBuffer2D(self.ctx, 1, n + 1, np.uint32)
        bufs = {}
        try:
            if capacity is None:
                out = capi.Observations(first.ptr, None, None, None, 0)
                capi.check(self.lib.bahip_surfel_observations(self.ctx.handle, C.byref(s), C.byref(out), C.byref(pairs)))
                capacity = int(pairs.value)
            cap = int(capacity)
            wanted = (["keyframes"] if keyframes else []) + list(residuals)
            for name, dtype, channels in self.OBSERVATION_PLANES:
                if name in wanted:
                    bufs[name] = DeviceBuffer2D(self.ctx, 1, max(1, cap) * channels, dtype)
            if prefill is not None:
                first.clear(prefill)
                for b in bufs.values():
                    b.clear(prefill)

            def planes():
                self.ctx.synchronize()
                res = {"surfel_first": first.download()[0].copy()}
                for name, dtype, channels in self.OBSERVATION_PLANES:
                    if name in bufs:
                        a = bufs[name].download()[0, :cap * channels]
                        res[name] = (a.reshape(cap, channels) if channels > 1 else a).copy()
                return res

            out = capi.Observations(first.ptr, *[bufs[name].ptr if name in bufs else None for name, _, _ in self.OBSERVATION_PLANES], cap)
            try:
                capi.check(self.lib.bahip_surfel_observations(self.ctx.handle, C.byref(s), C.byref(out), C.byref(pairs)))
            except capi.BackendError as e:
                e.arrays = planes()
                raise
            res = planes()
            res["pairs"] = int(pairs.value)
            return res
        finally:
            first.free()
            for b in bufs.values():
                b.free()

    def exact_sum(self, values, mode=0):
        """Exactly rounded binary64 sum of binary32 values through the device's exact accumulators (test hook)."""
        v = np.ascontiguousarray(values, np.float32)
        out = C.c_double()
        capi.check(self.lib.bahip_debug_exact_sum(self.ctx.handle, v.ctypes.data_as(C.POINTER(C.c_float)), v.size, int(mode), C.byref(out)))
        return float(out.value)

    def count_pairs(self):
        """(wave-keyframe candidates, wave-keyframe hits, associated pairs, in-image pairs) of one sweep."""
        out = (C.c_uint64 * 4)()
        s = self.surfels_struct()
        capi.check(self.lib.bahip_debug_count_pairs(self.ctx.handle, C.byref(s), out))
        return [int(v) for v in out]

    def tile_cull(self, size=None, want_bounds=True, prefill=None):
        """The tile cull of the sweeps as the device compiles it in the context's flavour (bahip_debug_tile_cull) over the first `size`
        surfels (default: all) and the bound keyframes: (bounds, masks) -- bounds (tiles, 4) float32 (centre, inflated radius; None
        without want_bounds), masks (tiles, ceil(K / 64)) uint64, bit k % 64 of word k / 64 = the tile's sphere may project into
        keyframe k.  prefill: a byte value both host arrays are filled with before the call (tests: a word the call did not write
        shows; after a refused call they are the exception's `arrays` attribute)."""
        n = self.surfels_size if size is None else int(size)
        tiles, words = (n + 63) // 64, (len(self.keyframes) + 63) // 64
        bounds = np.zeros((max(1, tiles), 4), np.float32) if want_bounds else None
        masks = np.zeros((max(1, tiles), max(1, words)), np.uint64)
        if prefill is not None:
            for a in (bounds, masks):
                if a is not None:
                    a.view(np.uint8)[...] = prefill
        s = self.surfels_struct(n)
        try:
            capi.check(self.lib.bahip_debug_tile_cull(self.ctx.handle, C.byref(s), bounds.ctypes.data_as(C.POINTER(C.c_float)) if want_bounds else None,
                                                      masks.ctypes.data_as(C.POINTER(C.c_uint64))))
        except capi.BackendError as e:
            e.arrays = (bounds, masks)
            raise
        return (bounds[:tiles] if want_bounds else None), masks[:tiles, :words]

    def evaluate_pairs(self, i, surfel_indices, frame_T_global):
        idx = np.ascontiguousarray(surfel_indices, dtype=np.uint32)
        out = np.zeros((len(idx), 40), np.float32)
        F = (C.c_float * 12)(*[float(v) for v in frame_T_global])
        fr, s = self.frame_struct(i), self.surfels_struct()
        capi.check(self.lib.bahip_debug_evaluate_pairs(self.ctx.handle, C.byref(fr), F, C.byref(s),
                                                       idx.ctypes.data_as(C.POINTER(C.c_uint32)), len(idx),
                                                       out.ctypes.data_as(C.POINTER(C.c_float))))
        return out
