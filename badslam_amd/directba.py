"""Python view of the C++ host classes vis::DirectBA / vis::Keyframe (badslam_amd/host), through the
flat C header include/badslam_directba.h.  Method names follow the reference's DirectBA
(applications/badslam/src/badslam/direct_ba.h:73-388).  Nothing here computes: every call ends in
the HIP backend; if the libraries are missing or no GPU is present, construction raises."""
import ctypes as C
import os

import numpy as np

from . import capi

_HERE = os.path.dirname(os.path.abspath(__file__))
# BADSLAM_LIB_DIR: load the backend from another build directory (A/B timing of two builds on one GPU box)
HOST_LIB_PATH = os.path.join(os.environ.get("BADSLAM_LIB_DIR") or os.path.join(_HERE, "lib"), "libbadslam_host.so")

_F7 = C.c_float * 7
_F4 = C.c_float * 4
_lib = None


_CALLBACK = C.CFUNCTYPE(None, C.c_void_p)


def _load():
    global _lib
    if _lib is None:
        capi.load()   # raises if the HIP library is missing
        if not os.path.exists(HOST_LIB_PATH):
            raise capi.BackendError(f"{HOST_LIB_PATH} not found: run __graft_entry__.build()")
        L = C.CDLL(HOST_LIB_PATH)
        L.dba_create.restype = C.c_void_p
        L.dba_create.argtypes = [C.c_int, C.c_float, C.c_float, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_int, C.c_int]
        L.dba_destroy.argtypes = [C.c_void_p]
        L.dba_add_keyframe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]
        L.dba_keyframe_count.argtypes = [C.c_void_p]
        L.dba_get_keyframe_pose.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
        L.dba_set_keyframe_pose.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
        L.dba_get_keyframe_activation.argtypes = [C.c_void_p, C.c_int]
        L.dba_get_keyframe_ba_iterations.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.dba_download_keyframe_image.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.dba_upload_keyframe_image.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.dba_delete_keyframe.argtypes = [C.c_void_p, C.c_int]
        L.dba_create_surfels_for_keyframe.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.dba_estimate_frame_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.dba_bundle_adjustment.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 11 + [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
        L.dba_compute_cost.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(capi.Cost), C.POINTER(capi.Cost)]
        L.dba_compute_surfel_costs.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 5
        L.dba_render_surfels.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_float),
                                         C.POINTER(capi.RenderOptions)] + [C.c_void_p] * 4 + [C.POINTER(C.c_float)]
        # (an older build under A/B timing, scripts/ab_bench.sh, may lack this newer entry point: as capi.load)
        if not os.environ.get("BADSLAM_LIB_DIR") or hasattr(L, "dba_keyframe_residual_image"):
            L.dba_keyframe_residual_image.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float),
                                                      C.POINTER(capi.ResidualImageOptions)] + [C.c_void_p] * 7 + [C.POINTER(C.c_float)]
        if not os.environ.get("BADSLAM_LIB_DIR") or hasattr(L, "dba_observed_covisibility"):
            L.dba_observed_covisibility.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        if not os.environ.get("BADSLAM_LIB_DIR") or hasattr(L, "dba_reduced_camera_system"):
            L.dba_reduced_camera_system.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4 + \
                [C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
            L.dba_pose_covariances.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                               C.POINTER(C.c_int), C.c_void_p, C.c_char_p, C.c_int]
        if not os.environ.get("BADSLAM_LIB_DIR") or hasattr(L, "dba_surfel_observations"):
            L.dba_surfel_observations.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int] + [C.c_void_p] * 4 + \
                [C.POINTER(C.c_int), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        if not os.environ.get("BADSLAM_LIB_DIR") or hasattr(L, "dba_keyframe_redundancy"):
            L.dba_keyframe_redundancy.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
            L.dba_find_redundant_keyframes.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.POINTER(C.c_int),
                                                       C.POINTER(C.c_int)]
            L.dba_cull_redundant_keyframes.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                                                       C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.dba_surfel_count.restype = C.c_uint32
        L.dba_surfel_count.argtypes = [C.c_void_p]
        L.dba_surfels_size.restype = C.c_uint32
        L.dba_surfels_size.argtypes = [C.c_void_p]
        L.dba_set_surfel_count.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.dba_download_surfels.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]
        L.dba_upload_surfels.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]
        L.dba_get_cameras.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.dba_set_cameras.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float]
        L.dba_cfactor_size.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.dba_download_cfactor.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.dba_clear_cfactor.argtypes = [C.c_void_p, C.c_void_p]
        L.dba_set_surfel_sharding.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32]
        L.dba_set_keyframe_sharding.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.dba_set_pcg_gauge_keyframe.argtypes = [C.c_void_p, C.c_int]
        L.dba_set_windowed_pcg.argtypes = [C.c_void_p, C.c_int]
        L.dba_set_pcg_step_control.argtypes = [C.c_void_p, C.c_int] + [C.c_float] * 5 + [C.c_int]
        L.dba_pcg_step_stats.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.dba_set_pose_step_control.argtypes = [C.c_void_p, C.c_int] + [C.c_float] * 5 + [C.c_int]
        L.dba_get_pose_step_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_float)]
        L.dba_set_geometry_step_control.argtypes = [C.c_void_p, C.c_int] + [C.c_float] * 4 + [C.c_int, C.c_int]
        L.dba_get_geometry_step_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_longlong)] * 3 + [C.POINTER(C.c_int)]
        # (an older build under A/B timing, scripts/ab_bench.sh, may lack these newer entry points: as capi.load)
        if not os.environ.get("BADSLAM_LIB_DIR") or hasattr(L, "dba_set_intrinsics_step_control"):
            L.dba_set_intrinsics_step_control.argtypes = [C.c_void_p, C.c_int] + [C.c_float] * 3 + [C.c_int]
            L.dba_set_intrinsics_updated_callback.argtypes = [C.c_void_p, _CALLBACK, C.c_void_p]
            L.dba_get_intrinsics_step_drops.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
            L.dba_get_intrinsics_step_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float),
                                                        C.POINTER(C.c_float)]
        L.dba_set_distributed_lifecycle.argtypes = [C.c_void_p, C.c_int]
        L.dba_set_ba_iteration_counts.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.dba_last_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.dba_backend_context.restype = C.c_void_p
        L.dba_backend_context.argtypes = [C.c_void_p]
        L.dba_keyframe_frame.argtypes = [C.c_void_p, C.c_int, C.POINTER(capi.Frame)]
        L.dba_surfels_struct.argtypes = [C.c_void_p, C.POINTER(capi.Surfels)]
        L.dba_bind_scene.argtypes = [C.c_void_p, C.c_void_p]
        L.dba_keyframe_covisibility.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int]
        _lib = L
    return _lib


class _BackendContext:
    """Duck-types lowlevel.Context for helpers that need (lib, handle)."""

    def __init__(self, handle):
        self.lib = capi.load()
        self.handle = C.c_void_p(handle)

    def synchronize(self):
        capi.check(self.lib.bahip_context_synchronize(self.handle))


class DirectBA:
    def __init__(self, max_surfel_count, raw_to_float_depth, baseline_fx, sparse_surfel_cell_size, width, height, color_camera,
                 depth_camera, use_depth_residuals=True, use_descriptor_residuals=True, surfel_merge_dist_factor=0.8,
                 min_observation_count_while_bootstrapping_1=2, min_observation_count_while_bootstrapping_2=2,
                 min_observation_count=2, stream=None):
        self.L = _load()
        cc = _F4(*[float(v) for v in color_camera])
        dc = _F4(*[float(v) for v in depth_camera])
        self.h = self.L.dba_create(int(max_surfel_count), float(raw_to_float_depth), float(baseline_fx), int(sparse_surfel_cell_size),
                                   float(surfel_merge_dist_factor), int(min_observation_count_while_bootstrapping_1),
                                   int(min_observation_count_while_bootstrapping_2), int(min_observation_count), int(width),
                                   int(height), cc, dc, int(use_depth_residuals), int(use_descriptor_residuals))
        if not self.h:
            raise capi.BackendError("DirectBA needs a HIP device (no CPU fallback)")
        self.width, self.height, self.stream = int(width), int(height), stream
        self.capacity = int(max_surfel_count)

    def close(self):
        if self.h:
            self.L.dba_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def backend_context(self):
        return _BackendContext(self.L.dba_backend_context(self.h))

    # borrowed views for driving single bahip_* stages on this scene (stage-level parity tests)
    def keyframe_frame(self, k):
        f = capi.Frame()
        assert self.L.dba_keyframe_frame(self.h, int(k), C.byref(f)) == 0
        return f

    def surfels_struct(self):
        s = capi.Surfels()
        assert self.L.dba_surfels_struct(self.h, C.byref(s)) == 0
        return s

    def keyframe_covisibility(self, k):
        cap = max(1, self.keyframe_count())
        out = (C.c_int * cap)()
        n = self.L.dba_keyframe_covisibility(self.h, int(k), out, cap)
        assert 0 <= n <= cap
        return [int(out[i]) for i in range(n)]

    def BindScene(self):
        assert self.L.dba_bind_scene(self.h, self.stream) == 0

    # -- keyframes --
    def AddKeyframe(self, depth_u16, rgb_u8, global_T_frame):
        d = np.ascontiguousarray(depth_u16, np.uint16)
        c = np.ascontiguousarray(rgb_u8, np.uint8)
        return self.L.dba_add_keyframe(self.h, self.stream, d.ctypes.data, c.ctypes.data, _F7(*[float(v) for v in global_T_frame]))

    def keyframe_count(self):
        return self.L.dba_keyframe_count(self.h)

    def keyframe_pose(self, k):
        out = _F7()
        assert self.L.dba_get_keyframe_pose(self.h, k, out) == 0
        return np.array(list(out), np.float64)

    def set_keyframe_pose(self, k, pose):
        assert self.L.dba_set_keyframe_pose(self.h, k, _F7(*[float(v) for v in pose])) == 0

    def keyframe_activation(self, k):
        return self.L.dba_get_keyframe_activation(self.h, k)

    def keyframe_ba_iterations(self, k):
        """(last_active_in_ba_iteration, last_covis_in_ba_iteration) of keyframe k: the BA iteration counts of the last creation loops
        that met it kActive / kCovisibleActive (-1: none)."""
        a, c = C.c_int(), C.c_int()
        assert self.L.dba_get_keyframe_ba_iterations(self.h, int(k), C.byref(a), C.byref(c)) == 0
        return a.value, c.value

    def keyframe_image(self, k, which):
        names = {"depth": (0, np.uint16, 1), "normals": (1, np.uint16, 1), "radius": (2, np.uint16, 1), "color": (3, np.uint8, 4)}
        idx, dt, ch = names[which]
        out = np.empty((self.height, self.width) if ch == 1 else (self.height, self.width, ch), dt)
        assert self.L.dba_download_keyframe_image(self.h, self.stream, k, idx, out.ctypes.data) == 0
        return out

    def upload_keyframe_image(self, k, which, array):
        names = {"depth": (0, np.uint16), "normals": (1, np.uint16), "radius": (2, np.uint16), "color": (3, np.uint8)}
        idx, dt = names[which]
        a = np.ascontiguousarray(array, dt)
        assert self.L.dba_upload_keyframe_image(self.h, self.stream, k, idx, a.ctypes.data) == 0

    # -- surfels --
    def CreateSurfelsForKeyframe(self, k, filter_new_surfels=False):
        assert self.L.dba_create_surfels_for_keyframe(self.h, self.stream, int(filter_new_surfels), int(k)) == 0

    def surfel_count(self):
        return int(self.L.dba_surfel_count(self.h))

    def surfels_size(self):
        return int(self.L.dba_surfels_size(self.h))

    def SortSurfelsSpatially(self, grid_cell_size=0.02):
        self.L.dba_sort_surfels_spatially.argtypes = [C.c_void_p, C.c_void_p, C.c_float]
        assert self.L.dba_sort_surfels_spatially(self.h, self.stream, float(grid_cell_size)) == 0

    def SetBatchedCreation(self, enabled):
        self.L.dba_set_batched_creation.argtypes = [C.c_void_p, C.c_int]
        assert self.L.dba_set_batched_creation(self.h, int(bool(enabled))) == 0

    def SetSpatialSortCellSize(self, grid_cell_size):
        self.L.dba_set_spatial_sort_cell_size.argtypes = [C.c_void_p, C.c_float]
        assert self.L.dba_set_spatial_sort_cell_size(self.h, float(grid_cell_size)) == 0

    def unsorted_surfels(self):
        self.L.dba_unsorted_surfels.restype = C.c_uint32
        self.L.dba_unsorted_surfels.argtypes = [C.c_void_p]
        return int(self.L.dba_unsorted_surfels(self.h))

    def SetSurfelCount(self, surfel_count, surfels_size):
        self.L.dba_set_surfel_count(self.h, int(surfel_count), int(surfels_size))

    def download_surfels(self, rows=8, count=None):
        n = self.surfels_size() if count is None else int(count)
        out = np.zeros((rows, n), np.float32)
        if n:
            assert self.L.dba_download_surfels(self.h, self.stream, rows, n, out.ctypes.data) == 0
        return out

    def upload_surfels(self, data):
        a = np.ascontiguousarray(data, np.float32)
        assert self.L.dba_upload_surfels(self.h, self.stream, a.shape[0], a.shape[1], a.ctypes.data) == 0
        self.SetSurfelCount(a.shape[1], a.shape[1])

    # -- optimisation --
    def EstimateFramePose(self, k, init_pose):
        out = _F7()
        assert self.L.dba_estimate_frame_pose(self.h, self.stream, int(k), _F7(*[float(v) for v in init_pose]), out) == 0
        return np.array(list(out), np.float64)

    def compute_cost(self, per_keyframe=True):
        """DirectBA::ComputeCost: the value of the BA objective with this object's residual switches (exact sums; the same bits under
        either sharding).  Returns (total, list indexed by keyframe id or None), dicts as lowlevel.cost_dict."""
        from badslam_amd.lowlevel import cost_dict
        total = capi.Cost()
        n = self.keyframe_count()
        per = (capi.Cost * max(1, n))() if per_keyframe else None
        assert self.L.dba_compute_cost(self.h, self.stream, C.byref(total), per) == 0
        return cost_dict(total), ([cost_dict(c) for c in per[:n]] if per_keyframe else None)

    def compute_surfel_costs(self):
        """DirectBA::ComputeSurfelCosts: the objective per surfel with this object's residual switches, in buffer order.  Returns a
        dict of five numpy arrays of surfels_size() entries: depth, descriptor_1, descriptor_2 (float64: exact sums over all keyframes)
        and depth_residuals, descriptor_pairs (uint32).  Under keyframe sharding every rank gets the unsharded values, under surfel
        sharding those of its own shard."""
        n = self.surfels_size()
        out = {name: np.zeros(n, np.float64) for name in ("depth", "descriptor_1", "descriptor_2")}
        out.update({name: np.zeros(n, np.uint32) for name in ("depth_residuals", "descriptor_pairs")})
        assert self.L.dba_compute_surfel_costs(self.h, self.stream, n, *[a.ctypes.data for a in out.values()]) == 0
        return out

    def observed_covisibility(self):
        """DirectBA::ComputeObservedCovisibility: (ids, counts) -- the ids of the existing keyframes in order and the (K, K) uint32
        matrix of the surfels the association rule pairs with both keyframes of a pair (both triangles; the diagonal a keyframe's own
        pair count).  Under surfel sharding with an all-reduce installed, and under keyframe sharding, every rank gets the
        unsharded matrix."""
        cap = max(1, self.keyframe_count())
        counts = np.zeros(cap * cap, np.uint32)
        ids = (C.c_int * cap)()
        rows = C.c_int()
        assert self.L.dba_observed_covisibility(self.h, self.stream, cap, counts.ctypes.data, ids, C.byref(rows)) == 0
        K = rows.value
        return [int(v) for v in ids[:K]], counts[:K * K].reshape(K, K).copy()

    RCS_STATS = ("list_entries", "pairs_visited", "atomics_issued", "degenerate_surfels", "overflow_tiles", "invalid")

    def reduced_camera_system(self, marginalise=True):
        """DirectBA::ComputeReducedCameraSystem: a dict -- keyframe_ids (the id of each block), S (6K, 6K) and g (6K,) in float64: the
        Gauss-Newton system over the poses of the existing keyframes with every surfel eliminated (marginalise=False: the block
        diagonal of the pose equations), A (K, 6, 6) and b (K, 6) the keyframes' own pose equations, stats (RCS_STATS).  No gauge is
        removed.  Not available under keyframe sharding."""
        cap = max(1, self.keyframe_count())
        n = 6 * cap
        S, g, A, b = np.zeros(n * n), np.zeros(n), np.zeros(36 * cap), np.zeros(n)
        ids, rows, stats = (C.c_int * cap)(), C.c_int(), (C.c_uint64 * 6)()
        assert self.L.dba_reduced_camera_system(self.h, self.stream, int(bool(marginalise)), cap, S.ctypes.data, g.ctypes.data, A.ctypes.data,
                                                b.ctypes.data, ids, stats, C.byref(rows)) == 0
        K = rows.value
        return dict(keyframe_ids=[int(v) for v in ids[:K]], S=S[:36 * K * K].reshape(6 * K, 6 * K).copy(), g=g[:6 * K].copy(),
                    A=A[:36 * K].reshape(K, 6, 6).copy(), b=b[:6 * K].reshape(K, 6).copy(), stats=dict(zip(self.RCS_STATS, (int(v) for v in stats))))

    def pose_covariances(self, gauge_keyframe, pairs=()):
        """DirectBA::ComputePoseCovariances: the gauge keyframe's rows and columns deleted from the reduced camera system, the rest
        factored and inverted in float64.  Returns (ids, marginal, cross): the remaining keyframe ids, their (R, 6, 6) marginal pose
        covariances, and the (len(pairs), 6, 6) covariance blocks between the keyframes of each pair of ids.  Raises ValueError with
        the reason when the gauge keyframe does not exist, a pair names it or an unknown id, or a pivot is not positive."""
        cap = max(1, self.keyframe_count())
        pairs = [(int(i), int(j)) for i, j in pairs]
        marginal, cross = np.zeros(36 * cap), np.zeros(36 * max(1, len(pairs)))
        ids, rows = (C.c_int * cap)(), C.c_int()
        flat = (C.c_int * max(1, 2 * len(pairs)))(*[v for p in pairs for v in p])
        error = C.create_string_buffer(512)
        rc = self.L.dba_pose_covariances(self.h, self.stream, int(gauge_keyframe), cap, marginal.ctypes.data, ids, C.byref(rows), len(pairs), flat,
                                         cross.ctypes.data, error, len(error))
        if rc == 2:
            raise ValueError(error.value.decode())
        assert rc == 0
        R = rows.value
        return [int(v) for v in ids[:R]], marginal[:36 * R].reshape(R, 6, 6).copy(), cross[:36 * len(pairs)].reshape(len(pairs), 6, 6).copy()

    def surfel_observations(self, residuals=False):
        """DirectBA::ComputeSurfelObservations: a dict -- keyframe_ids (the id of each bound index), first (surfels_size + 1 uint32
        offsets, the last one the number of pairs P), keyframes (P uint16 indices into keyframe_ids, ascending within a surfel's list)
        and, with residuals, depth_raw (P float32) and descriptor_raw ((P, 2) float32, NaN where the pair's colour pixel is not
        valid).  Under surfel sharding this rank's shard; under keyframe sharding the unsharded lists on every rank."""
        n, cap = self.surfels_size(), max(1, self.keyframe_count())
        pairs, K = C.c_uint64(), C.c_int()
        self.L.dba_surfel_observations(self.h, self.stream, 0, 0, 0, None, None, None, None, None, C.byref(pairs), C.byref(K))   # sizes the arrays
        P = int(pairs.value)
        first, ks = np.zeros(n + 1, np.uint32), np.zeros(P, np.uint16)
        depth, desc = (np.zeros(P, np.float32), np.zeros((P, 2), np.float32)) if residuals else (None, None)
        ids = (C.c_int * cap)()
        assert self.L.dba_surfel_observations(self.h, self.stream, n, P, cap, first.ctypes.data, ks.ctypes.data,
                                              depth.ctypes.data if residuals else None, desc.ctypes.data if residuals else None, ids,
                                              C.byref(pairs), C.byref(K)) == 0
        assert pairs.value == P
        out = dict(keyframe_ids=[int(v) for v in ids[:K.value]], first=first, keyframes=ks)
        if residuals:
            out.update(depth_raw=depth, descriptor_raw=desc)
        return out

    def keyframe_redundancy(self, bins=16):
        """DirectBA::ComputeKeyframeRedundancy: (ids, hist) -- the ids of the existing keyframes in order and the (K, bins) uint32
        table: hist[i, j] = the surfels paired with keyframe ids[i] that min(o, bins - 1) = j other keyframes are paired with too.
        Under surfel sharding with an all-reduce installed, and under keyframe sharding, every rank gets the unsharded table."""
        cap = max(1, self.keyframe_count())
        hist = np.zeros(cap * bins, np.uint32)
        ids = (C.c_int * cap)()
        rows = C.c_int()
        assert self.L.dba_keyframe_redundancy(self.h, self.stream, int(bins), cap, hist.ctypes.data, ids, C.byref(rows)) == 0
        K = rows.value
        return [int(v) for v in ids[:K]], hist[:K * bins].reshape(K, bins).copy()

    def find_redundant_keyframes(self, min_other_observers, min_fraction, bins=16):
        """DirectBA::FindRedundantKeyframes: the ids of the keyframes of whose surfels at least min_fraction have min_other_observers
        other observers or more, most redundant first, ties to the lower id.  Deletes nothing."""
        cap = max(1, self.keyframe_count())
        ids = (C.c_int * cap)()
        n = C.c_int()
        assert self.L.dba_find_redundant_keyframes(self.h, self.stream, int(min_other_observers), float(min_fraction), int(bins), cap, ids,
                                                   C.byref(n)) == 0
        return [int(v) for v in ids[:n.value]]

    def cull_redundant_keyframes(self, min_other_observers, min_fraction, max_deletions, protect_newest=0):
        """DirectBA::CullRedundantKeyframes: deletes, one by one and with the table computed again after each deletion, the most
        redundant qualifying keyframe that is neither the first existing one nor among the protect_newest last ones; returns the
        deleted ids in order.  Nothing calls it unless asked."""
        cap = max(1, self.keyframe_count())
        ids = (C.c_int * cap)()
        n = C.c_int()
        assert self.L.dba_cull_redundant_keyframes(self.h, self.stream, int(min_other_observers), float(min_fraction), int(max_deletions),
                                                   int(protect_newest), cap, ids, C.byref(n)) == 0
        return [int(v) for v in ids[:n.value]]

    def render_surfels(self, keyframe=None, view_camera=None, width=None, height=None, global_T_frame=None, options=None):
        """DirectBA::RenderKeyframeView (keyframe: an id -- the depth camera at that keyframe's pose) or DirectBA::RenderSurfels (the
        camera fx, fy, cx, cy of width x height pixels at the pose global_T_frame, 7 floats): the surfel map seen from that camera.
        options: a capi.RenderOptions (default: discs of at most 4 px, back faces culled).  Returns a dict of numpy arrays of height x
        width pixels -- depth (float32, 0 where empty), index (uint32, 0xFFFFFFFF where empty), normal (x 3, float32), color (x 4,
        uint8) -- and frame_T_global, the 12 floats the render used."""
        if keyframe is not None:
            width, height, cam, pose, keyframe = self.width, self.height, None, None, int(keyframe)
        else:
            cam = _F4(*[float(v) for v in view_camera])
            pose = (C.c_float * 7)(*[float(v) for v in global_T_frame])
            width, height, keyframe = int(width), int(height), -1
        out = dict(depth=np.zeros((height, width), np.float32), index=np.zeros((height, width), np.uint32),
                   normal=np.zeros((height, width, 3), np.float32), color=np.zeros((height, width, 4), np.uint8))
        F = (C.c_float * 12)()
        opt = options if options is not None else capi.RenderOptions()
        assert self.L.dba_render_surfels(self.h, self.stream, keyframe, cam, width, height, pose, C.byref(opt),
                                         *[a.ctypes.data for a in out.values()], F) == 0
        out["frame_T_global"] = np.array(list(F), np.float32)
        return out

    def keyframe_residual_image(self, keyframe, global_T_frame=None, select=capi.RESIDUAL_BEST, index_base=0):
        """DirectBA::KeyframeResidualImage (keyframe: an id, at its own pose) or, with global_T_frame (7 floats), DirectBA::
        FrameResidualImage on that keyframe's images at the pose given: per pixel of the depth image the associated surfel with the
        smallest (capi.RESIDUAL_BEST) or largest (RESIDUAL_WORST) |depth residual| and its residuals.  Returns a dict of numpy arrays
        of height x width pixels -- key (uint64), pairs, index (uint32), depth_residual, inv_stddev (float32), desc_residual (x 2,
        float32), color_valid (uint8) -- and frame_T_global, the 12 floats the call used."""
        h, w = self.height, self.width
        out = dict(key=np.zeros((h, w), np.uint64), pairs=np.zeros((h, w), np.uint32), index=np.zeros((h, w), np.uint32),
                   depth_residual=np.zeros((h, w), np.float32), inv_stddev=np.zeros((h, w), np.float32),
                   desc_residual=np.zeros((h, w, 2), np.float32), color_valid=np.zeros((h, w), np.uint8))
        pose = None if global_T_frame is None else (C.c_float * 7)(*[float(v) for v in global_T_frame])
        F = (C.c_float * 12)()
        opt = capi.ResidualImageOptions(select, index_base)
        assert self.L.dba_keyframe_residual_image(self.h, self.stream, int(keyframe), pose, C.byref(opt),
                                                  *[a.ctypes.data for a in out.values()], F) == 0
        out["frame_T_global"] = np.array(list(F), np.float32)
        return out

    def BundleAdjustment(self, optimize_depth_intrinsics=False, optimize_color_intrinsics=False, do_surfel_updates=False,
                         optimize_poses=True, optimize_geometry=True, min_iterations=1, max_iterations=1, use_pcg=False,
                         active_keyframe_window_start=0, active_keyframe_window_end=None, increase_ba_iteration_count=True,
                         pcg_max_inner_iterations=30):
        if active_keyframe_window_end is None:
            active_keyframe_window_end = self.keyframe_count() - 1
        done, conv = C.c_int(), C.c_int()
        assert self.L.dba_bundle_adjustment(self.h, self.stream, int(optimize_depth_intrinsics), int(optimize_color_intrinsics),
                                            int(do_surfel_updates), int(optimize_poses), int(optimize_geometry), int(min_iterations),
                                            int(max_iterations), int(use_pcg), int(active_keyframe_window_start),
                                            int(active_keyframe_window_end), int(increase_ba_iteration_count), C.byref(done),
                                            C.byref(conv), int(pcg_max_inner_iterations)) == 0
        return done.value, bool(conv.value)

    def last_stats(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self.L.dba_last_stats(self.h, C.byref(a), C.byref(b), C.byref(c))
        return dict(pose_rounds=a.value, pose_steps=b.value, pcg_inner_steps=c.value)

    # -- intrinsics --
    def cameras(self):
        cc, dc, a = _F4(), _F4(), C.c_float()
        self.L.dba_get_cameras(self.h, cc, dc, C.byref(a))
        return np.array(list(cc)), np.array(list(dc)), a.value

    def set_cameras(self, color_camera, depth_camera, a=0.0):
        self.L.dba_set_cameras(self.h, _F4(*[float(v) for v in color_camera]), _F4(*[float(v) for v in depth_camera]), float(a))

    def cfactor(self):
        w, h = C.c_int(), C.c_int()
        self.L.dba_cfactor_size(self.h, C.byref(w), C.byref(h))
        out = np.zeros((h.value, w.value), np.float32)
        self.L.dba_download_cfactor(self.h, self.stream, out.ctypes.data)
        return out

    def set_ba_iteration_counts(self, ba_iteration_count, last_ba_iteration_count):
        self.L.dba_set_ba_iteration_counts(self.h, int(ba_iteration_count), int(last_ba_iteration_count))

    def SetSurfelSharding(self, rank, world, chunk=1024):
        """This object holds rank `rank`'s chunk-cyclic shard of one cloud; lifecycle phases run on the gathered cloud."""
        assert self.L.dba_set_surfel_sharding(self.h, int(rank), int(world), int(chunk)) == 0

    def MergeKeyframes(self, approx_merge_count=10):
        self.L.dba_merge_keyframes.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        assert self.L.dba_merge_keyframes(self.h, self.stream, int(approx_merge_count)) == 0

    def keyframe_exists(self, k):
        self.L.dba_keyframe_exists.argtypes = [C.c_void_p, C.c_int]
        return bool(self.L.dba_keyframe_exists(self.h, int(k)))

    def ExportToPointCloud_count(self):
        n = C.c_uint()
        self.L.dba_export_point_count.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint)]
        assert self.L.dba_export_point_count(self.h, self.stream, C.byref(n)) == 0
        return int(n.value)

    def SetRowMajorCreation(self, enabled):
        self.L.dba_set_row_major_creation.argtypes = [C.c_void_p, C.c_int]
        assert self.L.dba_set_row_major_creation(self.h, int(bool(enabled))) == 0

    def SetFastArithmetic(self, enabled):
        self.L.dba_set_fast_arithmetic.argtypes = [C.c_void_p, C.c_int]
        assert self.L.dba_set_fast_arithmetic(self.h, int(bool(enabled))) == 0

    def SetSumClasses(self, classes):
        self.L.dba_set_sum_classes.argtypes = [C.c_void_p, C.c_int]
        assert self.L.dba_set_sum_classes(self.h, int(classes)) == 0

    def SetIntrinsicsSumClasses(self, classes):
        """1 (default), 2, 4 or 8 keyframe classes in the global sums of the intrinsics step (keyframe sharding of it over world ranks needs >= world)."""
        self.L.dba_set_intrinsics_sum_classes.argtypes = [C.c_void_p, C.c_int]
        assert self.L.dba_set_intrinsics_sum_classes(self.h, int(classes)) == 0

    def SetPCGSumClasses(self, classes):
        """1 (default), 2, 4 or 8 keyframe classes in the surfel block of the PCG scheme's r, M and g (keyframe sharding of it over world ranks needs >= world)."""
        self.L.dba_set_pcg_sum_classes.argtypes = [C.c_void_p, C.c_int]
        assert self.L.dba_set_pcg_sum_classes(self.h, int(classes)) == 0

    def SetKeyframeSharding(self, rank, world):
        """This object holds all surfels and sweeps the keyframes k with k % world == rank (world = 2, 4 or 8: whole keyframe classes of the per-surfel sums; the intrinsics after SetIntrinsicsSumClasses(>= world), the PCG scheme after SetPCGSumClasses(>= world), without surfel updates)."""
        assert self.L.dba_set_keyframe_sharding(self.h, int(rank), int(world)) == 0

    def set_pcg_gauge_keyframe(self, k):
        self.L.dba_set_pcg_gauge_keyframe(self.h, int(k))

    def SetDistributedLifecycle(self, enabled):
        """Under surfel sharding (default off): the surfel lifecycle's sweeps are dealt over the ranks -- creation and merging by keyframe
        owner, deletion by surfel chunk -- with the bits of the replicated run.  Raises under keyframe sharding."""
        if self.L.dba_set_distributed_lifecycle(self.h, int(bool(enabled))) != 0:
            raise RuntimeError("SetDistributedLifecycle: refused under keyframe sharding, which deals its lifecycle by keyframe already")

    def SetPCGStepControl(self, control=None, **fields):
        """Step control of the PCG scheme (default off): BundleAdjustment(use_pcg=True) takes Marquardt-damped steps and keeps one only
        if ComputeCost's scalar falls strictly; a rejected step is undone bit for bit.  control: None / False = off, True = the defaults,
        or a dict; fields: lambda_initial, lambda_up, lambda_down, lambda_min, lambda_max, max_trials.  Raises under keyframe sharding
        and for values out of range."""
        if control is None or control is False:
            if self.L.dba_set_pcg_step_control(self.h, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0) != 0:
                raise RuntimeError("SetPCGStepControl: could not be switched off")
            return
        v = dict(lambda_initial=1e-3, lambda_up=10.0, lambda_down=0.33, lambda_min=0.0, lambda_max=1e6, max_trials=6)
        v.update(control if isinstance(control, dict) else {})
        v.update(fields)
        if self.L.dba_set_pcg_step_control(self.h, 1, v["lambda_initial"], v["lambda_up"], v["lambda_down"], v["lambda_min"],
                                           v["lambda_max"], int(v["max_trials"])) != 0:
            raise RuntimeError("SetPCGStepControl: refused under keyframe sharding, or a value is out of range")

    def SetPoseStepControl(self, control=None, **fields):
        """Step control of the pose phase of the alternating scheme (default off): per keyframe, a Marquardt-damped Gauss-Newton step is
        kept only if that keyframe's cost falls strictly.  control: None / False = off, True = the defaults, or a dict; fields:
        lambda_initial, lambda_up, lambda_down, lambda_min, lambda_max, max_trials.  Raises under keyframe sharding and for values out of
        range."""
        if control is None or control is False:
            if self.L.dba_set_pose_step_control(self.h, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0) != 0:
                raise RuntimeError("SetPoseStepControl: could not be switched off")
            return
        v = dict(lambda_initial=1e-3, lambda_up=10.0, lambda_down=0.33, lambda_min=0.0, lambda_max=1e6, max_trials=4)
        v.update(control if isinstance(control, dict) else {})
        v.update(fields)
        if self.L.dba_set_pose_step_control(self.h, 1, v["lambda_initial"], v["lambda_up"], v["lambda_down"], v["lambda_min"],
                                            v["lambda_max"], int(v["max_trials"])) != 0:
            raise RuntimeError("SetPoseStepControl: refused under keyframe sharding, or a value is out of range")

    def SetGeometryStepControl(self, control=None, **fields):
        """Step control of the geometry phase of the alternating scheme (default off): per surfel, a damped step is kept only if that
        surfel's cost falls strictly (and, with guard_pairs, it loses no associated pair); otherwise its words come back bit for bit.
        control: None / False = off, True = the defaults, or a dict; fields: lambda_initial, lambda_up, lambda_min, lambda_max,
        max_trials, guard_pairs.  Allowed under either sharding; raises for values out of range."""
        if control is None or control is False:
            if self.L.dba_set_geometry_step_control(self.h, 0, 0.0, 0.0, 0.0, 0.0, 0, 0) != 0:
                raise RuntimeError("SetGeometryStepControl: could not be switched off")
            return
        v = dict(lambda_initial=0.0, lambda_up=4.0, lambda_min=1.0, lambda_max=1e4, max_trials=4, guard_pairs=True)
        v.update(control if isinstance(control, dict) else {})
        v.update(fields)
        if self.L.dba_set_geometry_step_control(self.h, 1, v["lambda_initial"], v["lambda_up"], v["lambda_min"], v["lambda_max"],
                                                int(v["max_trials"]), int(bool(v["guard_pairs"]))) != 0:
            raise RuntimeError("SetGeometryStepControl: a value is out of range")

    def SetIntrinsicsStepControl(self, control=None, **fields):
        """Step control of the intrinsics step of the alternating scheme (default off): damped trials up the ladder 0, lambda_first,
        lambda_first * lambda_up, ... lambda_max; the first that lowers the objective strictly is kept, otherwise cameras, a and the
        cfactor image come back bit for bit.  The damping factor persists across iterations and calls; the intrinsics-updated callback
        fires only after an accepted step.  control: None / False = off, True = the defaults, or a dict; fields: lambda_first,
        lambda_up, lambda_max, max_trials.  Allowed under either sharding; raises for values out of range."""
        if control is None or control is False:
            if self.L.dba_set_intrinsics_step_control(self.h, 0, 0.0, 0.0, 0.0, 0) != 0:
                raise RuntimeError("SetIntrinsicsStepControl: could not be switched off")
            return
        v = dict(lambda_first=1.0, lambda_up=4.0, lambda_max=1e4, max_trials=4)
        v.update(control if isinstance(control, dict) else {})
        v.update(fields)
        if self.L.dba_set_intrinsics_step_control(self.h, 1, v["lambda_first"], v["lambda_up"], v["lambda_max"], int(v["max_trials"])) != 0:
            raise RuntimeError("SetIntrinsicsStepControl: a value is out of range")

    def SetIntrinsicsUpdatedCallback(self, callback):
        """DirectBA::SetIntrinsicsUpdatedCallback: `callback()` is called from BundleAdjustment after an intrinsics step has changed
        the cameras or the depth parameters (with the step control on: after an accepted step only); None removes it."""
        self._intrinsics_callback = _CALLBACK(lambda _user: callback()) if callback is not None else C.cast(None, _CALLBACK)
        self.L.dba_set_intrinsics_updated_callback(self.h, self._intrinsics_callback, None)

    def intrinsics_step_stats(self):
        """(last_intrinsics_trials, last_intrinsics_accepted, last_intrinsics_lambda, intrinsics_lambda): trials run and steps accepted
        by the intrinsics steps of the last BundleAdjustment call, the factor of its last accepted step (-1: none), and the factor
        the next step starts with."""
        trials, accepted, lam, nxt = C.c_int(), C.c_int(), C.c_float(), C.c_float()
        self.L.dba_get_intrinsics_step_stats(self.h, C.byref(trials), C.byref(accepted), C.byref(lam), C.byref(nxt))
        return trials.value, accepted.value, lam.value, nxt.value

    def intrinsics_step_drops(self):
        """(total, smallest): by how much the accepted intrinsics steps of the last BundleAdjustment call lowered the objective."""
        total, smallest = C.c_double(), C.c_double()
        self.L.dba_get_intrinsics_step_drops(self.h, C.byref(total), C.byref(smallest))
        return total.value, smallest.value

    def geometry_step_stats(self):
        """(last_geometry_candidates, last_geometry_accepted, last_geometry_restored, last_geometry_trials): the totals over the geometry
        calls of the last BundleAdjustment call; candidates = accepted + restored."""
        candidates, accepted, restored, trials = C.c_longlong(), C.c_longlong(), C.c_longlong(), C.c_int()
        self.L.dba_get_geometry_step_stats(self.h, C.byref(candidates), C.byref(accepted), C.byref(restored), C.byref(trials))
        return candidates.value, accepted.value, restored.value, trials.value

    def pose_step_stats(self, keyframe_id=0):
        """(last_pose_trials, last_pose_rejected_steps, lambda of keyframe_id): candidates evaluated / rejected by the pose phases of the
        last BundleAdjustment call, and the damping factor that keyframe's next pose phase starts with."""
        trials, rejected, lam = C.c_int(), C.c_int(), C.c_float()
        self.L.dba_get_pose_step_stats(self.h, C.byref(trials), C.byref(rejected), int(keyframe_id), C.byref(lam))
        return trials.value, rejected.value, lam.value

    def pcg_step_stats(self):
        """(last_pcg_lambda, last_pcg_trials, last_pcg_rejected_steps): the damping factor the next outer iteration starts with, and the
        trial steps / undone trial steps of the last BundleAdjustment call."""
        lam, trials, rejected = C.c_float(), C.c_int(), C.c_int()
        self.L.dba_pcg_step_stats(self.h, C.byref(lam), C.byref(trials), C.byref(rejected))
        return lam.value, trials.value, rejected.value

    def SetWindowedPCG(self, enabled):
        """Windowed PCG scheme (default off): BundleAdjustment(use_pcg=True) honours a fixed active keyframe window and skips deleted
        keyframes.  Raises under keyframe sharding and after SetPCGSumClasses(c > 1)."""
        if self.L.dba_set_windowed_pcg(self.h, int(bool(enabled))) != 0:
            raise RuntimeError("SetWindowedPCG: the windowed PCG scheme is not available under keyframe sharding or with more than one "
                               "PCG sum class")
