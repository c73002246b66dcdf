"""Loader of the HIP library (csrc/libmpmvs_hip.so) behind include/mpmvs.h.

There is no CPU fallback: if the library is missing or no HIP device is
visible, creating a context raises.
"""
import ctypes as C
import os

import numpy as np

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libmpmvs_hip.so")

# entry points of include/mpmvs.h beyond the set shared with the test oracle
_P = C.c_void_p
_EXTRA = {
    "run_get": (C.c_int, [_P, C.POINTER(_abi.PatchMatchParams), C.c_uint64, _P, _P, _P]),
    "run_get_async": (C.c_int, [_P, C.POINTER(_abi.PatchMatchParams), C.c_uint64, _P, _P, _P]),
    "wait": (C.c_int, [_P]),
    "verify_rcp": (C.c_int, [C.POINTER(C.c_ulonglong)]),
    "device_count": (C.c_int, []),
    "texture_filter_bits": (C.c_int, []),
    "set_src_depths_device": (C.c_int, [_P, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "export_depth_device": (C.c_int, [_P, _P]),
    "set_src_depths_mixed": (C.c_int, [_P, C.c_int, C.POINTER(C.POINTER(C.c_float)), C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "device_alloc": (C.c_void_p, [C.c_int, C.c_size_t]),
    "device_free": (None, [C.c_int, C.c_void_p]),
    "set_profiling": (C.c_int, [_P, C.c_int]),
    "set_texture_format": (C.c_int, [_P, C.c_int]),
    "texture_format": (C.c_int, [_P]),
    "get_kernel_times": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "set_geom_costs": (C.c_int, [_P, _P]),
    "prior_vertices": (C.c_int, [_P, C.c_int, _P, C.c_int, C.POINTER(C.c_int)]),
    "prior_from_triangles": (C.c_int, [_P, C.POINTER(_abi.PatchMatchParams), _P, C.c_int]),
    "get_prior": (C.c_int, [_P, _P, _P]),
    "prior_rows": (C.c_int, [_P, C.c_int, _P]),
    "alloc_pinned": (C.c_void_p, [C.c_size_t]),
    "free_pinned": (None, [C.c_void_p]),
    "peer_info": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "chain_status": (C.c_int, [_P]),
    "view_select": (C.c_int, [C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, C.c_int, _P, _P, _P, _P]),
    "view_select_kernel_ms": (C.c_float, []),
    "dbg_chain_stall": (C.c_int, [_P, C.c_int, C.c_int]),
    "dbg_own_costs": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int)]),
    "set_views_u8": (C.c_int, [_P, C.c_int, C.POINTER(_abi.Camera), C.POINTER(C.POINTER(C.c_ubyte)), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]),
    "resize_u8": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int, _P]),
    "skyseg_inspect": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_longlong)]),
    "skyseg_load": (C.c_int, [C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_void_p)]),
    "skyseg_run": (C.c_int, [_P, _P, _P]),
    "skyseg_run_u8": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_size_t, _P]),
    "skyseg_preprocess_u8": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_size_t, _P]),
    "skyseg_set_keep": (C.c_int, [_P, C.c_int]),
    "skyseg_blob": (C.c_int, [_P, C.c_char_p, _P, C.POINTER(C.c_int)]),
    "skyseg_dims": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "skyseg_ms": (C.c_float, [_P, C.POINTER(C.c_float)]),
    "skyseg_destroy": (None, [_P]),
    "undistort_camera": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, _P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "undistort_u8": (C.c_int, [C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, _P, C.c_int, _P, C.c_int, C.c_int, _P, _P]),
    "undistort_kernel_ms": (C.c_float, []),
    "eval_ncc_multi": (C.c_int, [_P, C.POINTER(_abi.PatchMatchParams), _P, C.c_int, C.c_int, C.c_int, _P, C.POINTER(C.c_float)]),
    # point clouds (cloud.py)
    "cloud_create": (C.c_int, [C.c_int, C.c_longlong, _P, C.POINTER(C.c_void_p)]),
    "cloud_nearest": (C.c_int, [_P, C.c_float, C.c_longlong, _P, _P, _P]),
    "cloud_stats": (C.c_int, [_P, C.POINTER(C.c_longlong)]),
    "cloud_kernel_ms": (C.c_float, [_P, C.POINTER(C.c_float)]),
    "cloud_destroy": (None, [_P]),
    "cloud_render_depth": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_float, _P, _P]),
    "cloud_render_ms": (C.c_float, [_P]),
    "cloud_render_pass_ms": (C.c_int, [_P, C.POINTER(C.c_float)]),
    # the space a scan's scanners observed (cloud.py: Observer)
    "observer_create": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "observer_classify": (C.c_int, [_P, C.c_longlong, _P, C.c_float, C.c_float, _P, _P]),
    "observer_maps": (C.c_int, [_P, C.c_int, _P]),
    "observer_stats": (C.c_int, [_P, C.POINTER(C.c_longlong)]),
    "observer_ms": (C.c_float, [_P, C.POINTER(C.c_float)]),
    "observer_destroy": (None, [_P]),
    # voxel-grid downsampling (cloud.py: voxel_downsample)
    "cloud_voxel_downsample": (C.c_longlong, [C.c_int, C.c_longlong, _P, _P, _P, C.c_float, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                              C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _P]),
    "cloud_voxel_ms": (C.c_float, []),
    "cloud_voxel_pass_ms": (None, [C.POINTER(C.c_float)]),
    # k nearest neighbours and outlier removal (cloud.py: Cloud.knn, remove_outliers)
    "cloud_knn": (C.c_int, [_P, C.c_float, C.c_int, C.c_longlong, _P, _P, _P, _P]),
    "cloud_knn_ms": (C.c_float, [_P, C.POINTER(C.c_float)]),
    "cloud_outliers": (C.c_longlong, [C.c_int, C.c_longlong, _P, C.c_float, C.c_int, C.c_double, C.c_int, _P, _P, _P, C.POINTER(C.c_longlong),
                                      C.POINTER(C.c_double)]),
    "cloud_outliers_ms": (C.c_float, []),
    # normals from the k nearest neighbours (cloud.py: Cloud.normals, estimate_normals)
    "cloud_normals": (C.c_int, [_P, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_double), _P, _P, _P, _P]),
    "cloud_normals_ms": (C.c_float, [_P, C.POINTER(C.c_float)]),
    # connected components within a radius (cloud.py: Cloud.components, remove_small_clusters)
    "cloud_components": (C.c_int, [_P, C.c_float, _P, _P, C.POINTER(C.c_longlong)]),
    "cloud_components_ms": (C.c_float, [_P, C.POINTER(C.c_float)]),
    "cloud_components_pass_ms": (C.c_int, [_P, C.POINTER(C.c_float)]),
    # registration (cloud.py: Aligner, solve, align)
    "align_create": (C.c_int, [_P, C.c_longlong, _P, C.POINTER(C.c_void_p)]),
    "align_sums": (C.c_int, [_P, C.c_float, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_double)]),
    "align_solve": (C.c_int, [C.POINTER(C.c_longlong), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "align_icp": (C.c_int, [_P, C.c_float, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_double)]),
    "align_ms": (C.c_float, [_P]),
    "align_destroy": (None, [_P]),
    # point-to-plane registration (cloud.py: Aligner.set_normals / plane_sums / plane_icp, plane_solve)
    "align_set_normals": (C.c_int, [_P, _P]),
    "align_plane_sums": (C.c_int, [_P, C.c_float, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_double)]),
    "align_plane_solve": (C.c_int, [C.POINTER(C.c_longlong), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                    C.POINTER(C.c_double)]),
    "align_plane_icp": (C.c_int, [_P, C.c_float, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                  C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    # TSDF volume and marching tetrahedra (mesh.py: Volume)
    "tsdf_create": (C.c_int, [C.c_int, C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_int), C.c_float, C.c_int, C.POINTER(C.c_void_p)]),
    "tsdf_integrate": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int]),
    "tsdf_get": (C.c_int, [_P, _P, _P, _P]),
    "tsdf_set": (C.c_int, [_P, _P, _P, _P]),
    "tsdf_mesh": (C.c_longlong, [_P, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)]),
    "tsdf_pass_ms": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "tsdf_destroy": (None, [_P]),
    # the brick-sparse volume (mesh.py: SparseVolume)
    "tsdf_create_sparse": (C.c_int, [C.c_int, C.POINTER(C.c_float), C.c_float, C.POINTER(C.c_int), C.c_float, C.c_int, C.c_float, C.c_longlong,
                                     C.POINTER(C.c_void_p)]),
    "tsdf_allocate": (C.c_int, [_P, C.c_int, _P, _P]),
    "tsdf_bricks": (C.c_longlong, [_P, C.POINTER(C.c_void_p)]),
    "tsdf_get_bricks": (C.c_int, [_P, _P, _P, _P]),
    "tsdf_set_bricks": (C.c_int, [_P, C.c_longlong, _P, _P, _P, _P]),
    "tsdf_sparse_stats": (C.c_int, [_P, C.POINTER(C.c_longlong), C.POINTER(C.c_float)]),
    # an indexed triangle mesh: components, vertex normals, select (mesh.py: Mesh)
    "mesh_create": (C.c_int, [C.c_int, C.c_longlong, _P, _P, C.c_longlong, _P, C.POINTER(C.c_void_p)]),
    "mesh_components": (C.c_int, [_P, _P, _P, _P, C.POINTER(C.c_longlong)]),
    "mesh_normals": (C.c_int, [_P, _P, C.POINTER(C.c_longlong)]),
    "mesh_select": (C.c_longlong, [_P, _P, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                   C.POINTER(C.c_longlong)]),
    "mesh_pass_ms": (C.c_int, [_P, C.POINTER(C.c_float)]),
    "mesh_destroy": (None, [_P]),
    # simplification by vertex clustering with quadrics (mesh.py: Mesh.simplify)
    "simplify_mesh": (C.c_longlong, [_P, C.c_float, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong), _P,
                                     C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_longlong)]),
    "simplify_mesh_ms": (C.c_int, [_P, C.POINTER(C.c_float)]),
    # a mesh as a surface: point-to-triangle distance and sampling (mesh.py: Mesh.distance, Mesh.sample)
    "surface_distance": (C.c_int, [_P, _P, C.c_float, _P, _P, C.POINTER(C.c_longlong)]),
    "surface_distance_ms": (C.c_float, [_P, C.POINTER(C.c_float)]),
    "surface_sample": (C.c_longlong, [_P, C.c_float, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "surface_sample_ms": (C.c_float, [_P, C.POINTER(C.c_float)]),
    # a mesh rendered into cameras: depth and triangle-id maps (mesh.py: Mesh.render_depth)
    "surface_render_depth": (C.c_int, [_P, C.c_int, _P, _P, _P, C.POINTER(C.c_longlong)]),
    "surface_render_ms": (C.c_float, [_P, C.POINTER(C.c_float)]),
    "surface_render_work": (C.c_int, [_P, C.POINTER(C.c_longlong)]),
}
ALL_SYMBOLS = ["mpmvs_" + n for n in list(_abi.SIGNATURES) + list(_EXTRA)] + ["mpmvs_fuse", "mpmvs_fuse_kernel_ms", "mpmvs_fuse_passes", "mpmvs_sky_bilateral", "mpmvs_sky_kernel_ms", "mpmvs_fuse_ply", "mpmvs_free", "mpmvs_fuse_ctx", "mpmvs_fuse_ply_ctx", "mpmvs_fuse_ply_tracks"]

_cache = {}


def load():
    """dlopen the HIP library and bind every entry point; raises if it is not built."""
    if "lib" in _cache:
        return _cache["lib"], _cache["fns"]
    # torch bundles its own libamdhip64; if our library pulled in /opt/rocm's copy
    # first, torch.cuda could no longer initialise in this process.  Importing
    # torch first makes both share one HIP runtime (same soname).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = os.environ.get("MPMVS_HIP_LIB", LIB_PATH)  # override: A/B-ing kernel builds
    if not os.path.exists(path):
        raise RuntimeError(f"HIP library not built: {path} (run __graft_entry__.build() or make -C mp-mvs_amd/csrc)")
    lib = C.CDLL(path)
    fns = _abi.bind(lib, "mpmvs_")
    for name, (res, args) in _EXTRA.items():
        fn = getattr(lib, "mpmvs_" + name)
        fn.restype = res
        fn.argtypes = args
        fns[name] = fn
    _cache["lib"], _cache["fns"] = lib, fns
    return lib, fns


LIB_Q8_PATH = os.path.join(_HERE, "csrc", "libmpmvs_hip_q8.so")


def load_variant(path):
    """a second build of the library next to the default one (the opt-in 8-bit-fraction twin, measurement builds): its own
    dlopen handle and function table; contexts are made with create(device, fns=...)"""
    if path in _cache:
        return _cache[path]
    load()   # torch's HIP runtime first (see load)
    if not os.path.exists(path):
        raise RuntimeError(f"HIP library not built: {path}")
    lib = C.CDLL(path)
    fns = _abi.bind(lib, "mpmvs_")
    for name, (res, args) in _EXTRA.items():
        fn = getattr(lib, "mpmvs_" + name)
        fn.restype = res
        fn.argtypes = args
        fns[name] = fn
    _cache[path] = (lib, fns)
    return lib, fns


class HipPatchMatch(_abi.PatchMatchHandle):
    """One PatchMatch context on one MI355X (the device-side half of the
    reference's PatchMatchCUDA object, reference include/PatchMatch.h:87-154)."""

    def __init__(self, device=0, fns=None):
        if fns is None:
            _, fns = load()
        ctx = fns["create"](int(device))
        if not ctx:
            msg = fns["last_error"](None)
            raise RuntimeError("mpmvs_create failed: " + (msg.decode() if msg else "unknown"))
        super().__init__(fns, ctx)
        self.device = int(device)

    def run_into(self, params, seed, planes, costs, geom=None):
        """Run() with the device-to-host copies that end it in the reference (mpmvs_run_get): the cost maps travel while the
        median filter still runs; arrays as for get_into (pinned memory keeps the copies asynchronous)"""
        assert planes.shape == (self.H, self.W, 4) and costs.shape == (self.H, self.W) and planes.dtype == np.float32 and costs.dtype == np.float32
        self._chk(self._f["run_get"](self._ctx, C.byref(params), int(seed), planes.ctypes.data, costs.ctypes.data,
                                     geom.ctypes.data if geom is not None else None), "run_get")

    def run_into_async(self, params, seed, planes, costs, geom=None):
        """pipelined Run() (mpmvs_run_get_async): returns at once; the maps reach the (pinned) arrays while the next such call
        of this context already runs -- give consecutive calls different arrays and collect with wait()"""
        assert planes.shape == (self.H, self.W, 4) and costs.shape == (self.H, self.W) and planes.dtype == np.float32 and costs.dtype == np.float32
        for a in (planes, costs, geom):
            # the copy engine writes into these arrays after this call has returned: they must be plain memory in C order ...
            assert a is None or (a.flags.c_contiguous and a.flags.writeable), "run_into_async needs writeable C-contiguous arrays"
        # ... and must stay alive until wait(): the handle keeps them (a caller that drops its last reference would otherwise
        # let the DMA write into freed memory).  Pageable arrays work but make the copies synchronous: use alloc_pinned / pin_memory.
        if not hasattr(self, "_async_bufs"):
            self._async_bufs = []
        self._async_bufs.append((planes, costs, geom))
        self._chk(self._f["run_get_async"](self._ctx, C.byref(params), int(seed), planes.ctypes.data, costs.ctypes.data,
                                           geom.ctypes.data if geom is not None else None), "run_get_async")

    def wait(self):
        """every pipelined Run() of this context has delivered its maps when this returns"""
        try:
            self._chk(self._f["wait"](self._ctx), "wait")
        finally:
            self._async_bufs = []

    def set_texture_format(self, force_fp32):
        """call before set_views; True keeps the fp32 texture format even for 8-bit exact images"""
        self._chk(self._f["set_texture_format"](self._ctx, 1 if force_fp32 else 0), "set_texture_format")

    def texture_format(self):
        return "u8" if self._f["texture_format"](self._ctx) == 1 else "f32"

    def chain_status(self):
        """1: Run() chains the passes of a scale into one launch; 0: one launch per pass by request (MPMVS_CHAIN=0); -1: per pass
        because the self-check of the chained launch failed on this device"""
        return int(self._f["chain_status"](self._ctx))

    def dbg_chain_stall(self, block_pos, spin_limit=0):
        """fault injection (tests): the update block at `block_pos` never signals its first pass; block_pos < 0 switches it off"""
        self._chk(self._f["dbg_chain_stall"](self._ctx, int(block_pos), int(spin_limit)), "dbg_chain_stall")

    def dbg_own_costs(self, enable=None):
        """the per-view costs kept from InitializeScore (mpmvs_dbg_own_costs): enable False makes every update pass recompute
        them, True is the default, None leaves the setting; returns the number of update passes enqueued so far that read them"""
        n = C.c_int(0)
        self._chk(self._f["dbg_own_costs"](self._ctx, -1 if enable is None else (1 if enable else 0), C.byref(n)), "dbg_own_costs")
        return int(n.value)

    def set_profiling(self, on=True):
        self._chk(self._f["set_profiling"](self._ctx, 1 if on else 0), "set_profiling")

    def kernel_times(self):
        ms = (C.c_float * 6)()
        cnt = (C.c_int * 6)()
        self._chk(self._f["get_kernel_times"](self._ctx, ms, cnt), "get_kernel_times")
        return list(ms), list(cnt)

    def set_geom_costs(self, geom):
        import numpy as np
        g = np.ascontiguousarray(geom, np.float32)
        assert g.shape == (self.H, self.W)
        self._chk(self._f["set_geom_costs"](self._ctx, g.ctypes.data), "set_geom_costs")

    def prior_vertices(self, geom_rule):
        """GetTriangulateVertices on the device -> [n, 2] int32 (x, y) in cell raster order"""
        import numpy as np
        cap = 3 * ((self.H + 4) // 5) * ((self.W + 4) // 5)
        out = np.empty((cap, 2), np.int32)
        n = C.c_int(0)
        self._chk(self._f["prior_vertices"](self._ctx, 1 if geom_rule else 0, out.ctypes.data, cap, C.byref(n)), "prior_vertices")
        return out[:n.value].copy()

    def prior_from_triangles(self, params, tri_pts):
        """raster + plane fit + depth-range test on the device for triangles [n][3][2] (all vertices inside the image);
        installs the prior like set_prior"""
        import numpy as np
        t = np.ascontiguousarray(tri_pts, np.int32).reshape(-1, 6)
        self._chk(self._f["prior_from_triangles"](self._ctx, C.byref(params), t.ctypes.data, len(t)), "prior_from_triangles")

    def get_prior(self):
        import numpy as np
        prior = np.empty((self.H, self.W, 4), np.float32)
        mask = np.empty((self.H, self.W), np.uint32)
        self._chk(self._f["get_prior"](self._ctx, prior.ctypes.data, mask.ctypes.data), "get_prior")
        return prior, mask

    def eval_ncc_multi(self, params, planes_cam, scale, mapping=0):
        """ComputeBilateralNCC of nh planes per pixel ([nh][H][W][4]) against every view -> ([nh][V][H][W], kernel ms);
        mapping 0 = one thread per pixel (the only one, include/mpmvs.h)"""
        import numpy as np
        p = np.ascontiguousarray(planes_cam, np.float32)
        nh = p.shape[0]
        assert p.shape == (nh, self.H, self.W, 4)
        out = np.empty((nh, params.num_images - 1, self.H, self.W), np.float32)
        ms = C.c_float(0.0)
        self._chk(self._f["eval_ncc_multi"](self._ctx, C.byref(params), p.ctypes.data, nh, int(scale), int(mapping), out.ctypes.data, C.byref(ms)), "eval_ncc_multi")
        return out, float(ms.value)

    def set_src_depths_device(self, ptrs, widths, heights):
        n = len(ptrs)
        arr = (C.c_void_p * n)(*[int(p) for p in ptrs])
        ws = (C.c_int * n)(*widths)
        hs = (C.c_int * n)(*heights)
        self._chk(self._f["set_src_depths_device"](self._ctx, n, arr, ws, hs), "set_src_depths_device")

    def export_depth_device(self, ptr):
        self._chk(self._f["export_depth_device"](self._ctx, int(ptr)), "export_depth_device")


def prior_rows(edge_sq):
    """the p-rows prior_from_triangles dispatches per squared longest edge (mpmvs_prior_rows; host arithmetic, no device): int32 array"""
    import numpy as np
    _, fns = load()
    e = np.ascontiguousarray(edge_sq, np.int64).reshape(-1)
    rows = np.empty(len(e), np.int32)
    if fns["prior_rows"](e.ctypes.data, len(e), rows.ctypes.data) != 0:
        raise RuntimeError("mpmvs_prior_rows refused its arguments")
    return rows


def peer_info(device, peer):
    """(can_access, link_type, hops) of mpmvs_peer_info: how `device` reaches `peer` in this process (link type 4 = xGMI, 2 = PCIe)"""
    _, fns = load()
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    if fns["peer_info"](int(device), int(peer), C.byref(a), C.byref(b), C.byref(c)) != 0:
        raise RuntimeError(f"mpmvs_peer_info({device}, {peer}) failed")
    return a.value, b.value, c.value


def resize_u8(img, new_w, new_h, device=0):
    """the resampling of set_views_u8 on its own (mpmvs_resize_u8): uint8 [h, w] -> float32 [new_h, new_w], equal bit for bit to
    hostlib.resize_linear of the widened image"""
    _, fns = load()
    im = np.asarray(img)
    assert im.dtype == np.uint8 and im.ndim == 2, (im.dtype, im.shape)
    if im.strides[1] != 1 or im.strides[0] < im.shape[1]:
        im = np.ascontiguousarray(im)
    out = np.empty((int(new_h), int(new_w)), np.float32)
    rc = fns["resize_u8"](int(device), im.ctypes.data, im.shape[1], im.shape[0], im.strides[0], int(new_w), int(new_h), out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"mpmvs_resize_u8 failed ({rc})")
    return out


def _camera_args(model, params):
    """(model id, float64 parameter array) from a model id or a COLMAP model name"""
    from .colmap import CAMERA_MODELS
    mid = CAMERA_MODELS.index(model) if isinstance(model, str) else int(model)
    return mid, np.ascontiguousarray(params, np.float64).reshape(-1)


def undistort_camera(model, params, width, height, blank_pixels=0.0, min_scale=0.2, max_scale=2.0):
    """the PINHOLE camera an image of COLMAP camera (model, params) is undistorted to (mpmvs_undistort_camera; host only):
    ((fx, fy, cx', cy'), W', H').  model: id or name of colmap.CAMERA_MODELS, params in the order of a cameras file"""
    _, fns = load()
    mid, prm = _camera_args(model, params)
    k = np.zeros(4)
    w, h = C.c_int(0), C.c_int(0)
    rc = fns["undistort_camera"](mid, prm.ctypes.data, len(prm), int(width), int(height), float(blank_pixels), float(min_scale), float(max_scale),
                                 k.ctypes.data, C.byref(w), C.byref(h))
    if rc != 0:
        raise ValueError(f"mpmvs_undistort_camera refused the camera or the options ({rc})")
    return tuple(float(v) for v in k), w.value, h.value


def undistort_u8(img, model, params, dst, device=0, valid=False):
    """mpmvs_undistort_u8: uint8 [h, w] or [h, w, 3] taken by COLMAP camera (model, params) -> the image of the pinhole camera
    dst = ((fx, fy, cx, cy), W', H') as undistort_camera returns it, same channels; valid=True: also the uint8 [H', W'] mask of
    the pixels that have a source"""
    _, fns = load()
    mid, prm = _camera_args(model, params)
    im = np.asarray(img)
    if im.dtype != np.uint8 or im.ndim not in (2, 3) or (im.ndim == 3 and im.shape[2] not in (1, 3)):
        raise ValueError(f"need a uint8 [h, w], [h, w, 1] or [h, w, 3] image, got {im.dtype} {im.shape}")
    ch = 1 if im.ndim == 2 else im.shape[2]
    if im.strides[-1] != 1 or (im.ndim == 3 and im.strides[1] != ch) or im.strides[0] < im.shape[1] * ch:
        im = np.ascontiguousarray(im)
    k, dw, dh = dst
    k = np.ascontiguousarray(k, np.float64)
    out = np.empty((int(dh), int(dw)) + im.shape[2:], np.uint8)
    ok = np.empty((int(dh), int(dw)), np.uint8) if valid else None
    rc = fns["undistort_u8"](int(device), im.ctypes.data, ch, im.shape[1], im.shape[0], im.strides[0], mid, prm.ctypes.data, len(prm), k.ctypes.data,
                             int(dw), int(dh), out.ctypes.data, ok.ctypes.data if valid else None)
    if rc == -2:
        raise ValueError("mpmvs_undistort_u8 refused its arguments (-2)")
    if rc != 0:
        raise RuntimeError(f"mpmvs_undistort_u8 failed ({rc})")
    return (out, ok) if valid else out


class SkySegError(RuntimeError):
    """a refused model or call of the sky-segmentation engine; .code is the negative code of include/mpmvs.h"""

    def __init__(self, what, code, text):
        super().__init__(f"{what} failed ({code}): {text}")
        self.code = code
        self.text = text


def _skyseg_raise(fns, what, rc):
    msg = fns["last_error"](None)
    raise SkySegError(what, rc, msg.decode() if msg else "")


SKYSEG_COUNTS = ("layers", "blobs", "convolutions", "live_layers", "weight_bytes", "macs")


def skyseg_inspect(param_path, bin_path, in_h=384, in_w=384, output_blob=None):
    """what the loader makes of an ncnn .param / .bin pair (mpmvs_skyseg_inspect), as a dict; touches no device"""
    _, fns = load()
    counts = (C.c_longlong * 6)()
    rc = fns["skyseg_inspect"](str(param_path).encode(), str(bin_path).encode(), int(in_h), int(in_w),
                               output_blob.encode() if output_blob else None, counts)
    if rc != 0:
        _skyseg_raise(fns, "skyseg_inspect", rc)
    return dict(zip(SKYSEG_COUNTS, (int(v) for v in counts)))


class SkySeg:
    """The sky-segmentation network on one MI355X (mpmvs_skyseg_*): the reference's SkySegment object
    (reference SkySegment/src/SkyRegionDetect.cpp:541-561).  There is no CPU path."""

    def __init__(self, param_path, bin_path, in_h=384, in_w=384, output_blob=None, device=0):
        _, self._f = load()
        net = C.c_void_p(None)
        rc = self._f["skyseg_load"](int(device), str(param_path).encode(), str(bin_path).encode(), int(in_h), int(in_w),
                                    output_blob.encode() if output_blob else None, C.byref(net))
        self._net = None
        if rc != 0:
            _skyseg_raise(self._f, "skyseg_load", rc)
        self._net = net
        d = (C.c_int * 7)()
        self._f["skyseg_dims"](self._net, d)
        self.in_shape, self.out_shape, self.launches = tuple(d[0:3]), tuple(d[3:6]), int(d[6])

    def close(self):
        if self._net:
            self._f["skyseg_destroy"](self._net)
            self._net = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            _skyseg_raise(self._f, what, rc)

    def run(self, chw):
        """the bare network: float32 [c, h, w] -> the output blob [c', h', w']"""
        x = np.ascontiguousarray(chw, np.float32)
        if x.shape != self.in_shape:
            raise SkySegError("skyseg_run", -2, f"input of shape {x.shape}, the network takes {self.in_shape}")
        out = np.empty(self.out_shape, np.float32)
        self._chk(self._f["skyseg_run"](self._net, x.ctypes.data, out.ctypes.data), "skyseg_run")
        return out

    @staticmethod
    def _bgr(img):
        im = np.asarray(img)
        if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
            raise SkySegError("skyseg_run_u8", -2, f"need a uint8 [h, w, 3] B,G,R image, got {im.dtype} {im.shape}")
        if im.strides[2] != 1 or im.strides[1] != 3 or im.strides[0] < 3 * im.shape[1]:
            im = np.ascontiguousarray(im)
        return im

    def run_u8(self, bgr):
        """maskExtractor with the pyrDown loop in front: uint8 [h, w, 3] (B,G,R) -> the output blob"""
        im = self._bgr(bgr)
        out = np.empty(self.out_shape, np.float32)
        self._chk(self._f["skyseg_run_u8"](self._net, im.ctypes.data, im.shape[0], im.shape[1], im.strides[0], out.ctypes.data), "skyseg_run_u8")
        return out

    def preprocess_u8(self, bgr):
        """probe: what run_u8 feeds the network, float32 [3, in_h, in_w]"""
        im = self._bgr(bgr)
        out = np.empty(self.in_shape, np.float32)
        self._chk(self._f["skyseg_preprocess_u8"](self._net, im.ctypes.data, im.shape[0], im.shape[1], im.strides[0], out.ctypes.data), "skyseg_preprocess_u8")
        return out

    def set_keep(self, keep=True):
        """keep every blob of a run (no buffer reuse) so that blob() can fetch it"""
        self._chk(self._f["skyseg_set_keep"](self._net, 1 if keep else 0), "skyseg_set_keep")

    def blob(self, name):
        d = (C.c_int * 3)()
        self._chk(self._f["skyseg_blob"](self._net, name.encode(), None, d), "skyseg_blob")
        out = np.empty(tuple(d), np.float32)
        self._chk(self._f["skyseg_blob"](self._net, name.encode(), out.ctypes.data, d), "skyseg_blob")
        return out

    def ms(self):
        """(network ms, preprocessing ms) of the last run, device time"""
        pre = C.c_float(0.0)
        net = self._f["skyseg_ms"](self._net, C.byref(pre))
        return float(net), float(pre.value)


def device_count():
    return load()[1]["device_count"]()


def create(device=0, fns=None):
    return HipPatchMatch(device, fns)


def create_q8(device=0):
    """a context of the opt-in build with CUDA's 8-bit texture interpolation fractions (libmpmvs_hip_q8.so)"""
    return HipPatchMatch(device, load_variant(LIB_Q8_PATH)[1])
