"""Depth maps to a triangle mesh on the GPU: a TSDF volume, dense (Volume) or brick-sparse (SparseVolume), and marching tetrahedra
on the Kuhn split of its cells (mpmvs_tsdf_*, csrc/pm_tsdf.hpp, csrc/pm_tsdf_sparse.hpp, csrc/mpmvs_mesh.hip; contract:
include/mpmvs.h, DESIGN.md sections 22 and 23); an indexed triangle mesh on the device (Mesh: mpmvs_mesh_*, csrc/pm_mesh.hpp;
DESIGN.md section 24) with its connected components, area-weighted vertex normals and compaction, remove_small_components and
vertex_normals on top of it; the mesh as a surface (mpmvs_surface_*, csrc/pm_surface.hpp): the exact capped
distance from a cloud's points to it and its deterministic samples, with surface_distances, evaluate_mesh and compare on top of
them; and the PLY files of a mesh.  The device calls are bit for bit their plain-loop
statements (tests/tsdf_common.py and tests/tsdf_sparse_common.py have them in numpy).  The work runs on the GPU; there is no CPU
path."""
import ctypes as C

import numpy as np

from . import _abi, engine
from . import cloud as _cloud


def _raise(f, what, rc):
    msg = f["last_error"](None)
    text = f"mpmvs_{what} failed ({rc}): " + (msg.decode() if msg else "")
    raise (ValueError if rc in (-2, -3) else RuntimeError)(text)


class Volume:
    """mpmvs_tsdf: a lattice of dims = (nx, ny, nz) sample points, x fastest, voxel (i, j, k) at origin + (i, j, k) * voxel, with
    the truncation distance `trunc`; per voxel the sum of the truncated signed distances (float32), the number of observations
    (int32) and, with color=True, the B, G, R sums and their count (uint32 x 4).  Dense on purpose: every voxel of the box exists.
    The device is opened by the first call that needs it."""

    def __init__(self, origin, voxel, dims, trunc, color=False, device=0):
        _, self._f = engine.load()
        self._h = None
        o = np.ascontiguousarray(origin, np.float32)
        d = np.ascontiguousarray(dims, np.int32)
        if o.shape != (3,) or d.shape != (3,):
            raise ValueError(f"need an origin and dims of 3 numbers each, got {o.shape} and {d.shape}")
        h = C.c_void_p()
        rc = self._f["tsdf_create"](int(device), o.ctypes.data_as(C.POINTER(C.c_float)), float(voxel), d.ctypes.data_as(C.POINTER(C.c_int)), float(trunc),
                                    1 if color else 0, C.byref(h))
        if rc != 0:
            _raise(self._f, "tsdf_create", rc)
        self._h = h
        self.origin, self.voxel, self.trunc, self.color, self.device = o, float(np.float32(voxel)), float(np.float32(trunc)), bool(color), int(device)
        self.dims = tuple(int(v) for v in d)
        self.n_vox = self.dims[0] * self.dims[1] * self.dims[2]

    def close(self):
        if self._h is not None:
            self._f["tsdf_destroy"](self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def integrate(self, cams, depths, colors=None):
        """mpmvs_tsdf_integrate: the views in order; cams: _abi.Camera (width and height give the maps' sizes), depths: float32
        [H, W] each, colors (iff the volume has colour): uint8 [H, W] (grey) or [H, W, 3] (B, G, R), all of one kind.  Successive
        calls continue the same sums."""
        cams = list(cams)
        n = len(cams)
        if len(depths) != n or (colors is not None and len(colors) != n):
            raise ValueError("need one depth map (and one colour image) per camera")
        ds = [np.ascontiguousarray(d, np.float32) for d in depths]
        for c, d in zip(cams, ds):
            if d.shape != (int(c.height), int(c.width)):
                raise ValueError(f"a depth map of shape {d.shape} for a camera of {int(c.height)} x {int(c.width)}")
        cs, channels = None, 0
        if colors is not None:
            cs = [np.ascontiguousarray(c, np.uint8) for c in colors]
            channels = 3 if n and cs[0].ndim == 3 else 1
            for c, d in zip(cs, ds):
                if c.shape != (d.shape + (3,) if channels == 3 else d.shape):
                    raise ValueError(f"a colour image of shape {c.shape} for a depth map of shape {d.shape} ({channels} channel(s))")
        arr = (_abi.Camera * max(n, 1))(*cams)
        dp = (C.c_void_p * max(n, 1))(*[d.ctypes.data for d in ds])
        cp = (C.c_void_p * max(n, 1))(*[c.ctypes.data for c in cs]) if cs is not None else None
        rc = self._f["tsdf_integrate"](self._h, n, arr, dp, cp, channels)
        if rc != 0:
            _raise(self._f, "tsdf_integrate", rc)

    def get(self):
        """{"sum": float32 [nz, ny, nx], "weight": int32 [nz, ny, nx]} and, with colour, "color": uint32 [nz, ny, nx, 4]"""
        nx, ny, nz = self.dims
        out = {"sum": np.empty((nz, ny, nx), np.float32), "weight": np.empty((nz, ny, nx), np.int32)}
        if self.color:
            out["color"] = np.empty((nz, ny, nx, 4), np.uint32)
        rc = self._f["tsdf_get"](self._h, out["sum"].ctypes.data, out["weight"].ctypes.data, out["color"].ctypes.data if self.color else None)
        if rc != 0:
            _raise(self._f, "tsdf_get", rc)
        return out

    def set(self, sum, weight, color=None):
        """replaces the volume; with colour, color=None clears the colour sums"""
        nx, ny, nz = self.dims
        s, w = np.ascontiguousarray(sum, np.float32), np.ascontiguousarray(weight, np.int32)
        c = np.ascontiguousarray(color, np.uint32) if color is not None else None
        if s.size != self.n_vox or w.size != self.n_vox or (c is not None and c.size != 4 * self.n_vox):
            raise ValueError(f"need {self.n_vox} sums and weights (and four colour entries per voxel)")
        rc = self._f["tsdf_set"](self._h, s.ctypes.data, w.ctypes.data, c.ctypes.data if c is not None else None)
        if rc != 0:
            _raise(self._f, "tsdf_set", rc)

    def mesh(self, min_weight=1):
        """mpmvs_tsdf_mesh -> {"xyz": float32 [n, 3], "rgb": uint8 [n, 3] or None, "tri": int32 [m, 3]}: the zero level set of
        sum / weight over the voxels with weight >= min_weight, counter-clockwise seen from the positive side"""
        lib, _ = engine.load()
        lib.mpmvs_free.argtypes = [C.c_void_p]
        lib.mpmvs_free.restype = None
        px, pc, pt, nt = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_longlong(0)
        nv = self._f["tsdf_mesh"](self._h, int(min_weight), C.byref(px), C.byref(pc) if self.color else None, C.byref(pt), C.byref(nt))
        if nv < 0:
            _raise(self._f, "tsdf_mesh", nv)
        try:
            xyz = np.ctypeslib.as_array(C.cast(px, C.POINTER(C.c_float)), (nv, 3)).copy() if nv else np.zeros((0, 3), np.float32)
            tri = np.ctypeslib.as_array(C.cast(pt, C.POINTER(C.c_int32)), (nt.value, 3)).copy() if nt.value else np.zeros((0, 3), np.int32)
            rgb = None
            if self.color:
                rgb = np.ctypeslib.as_array(C.cast(pc, C.POINTER(C.c_uint8)), (nv, 3)).copy() if nv else np.zeros((0, 3), np.uint8)
        finally:
            for p in (px, pc, pt):
                if p.value:
                    lib.mpmvs_free(p)
        return {"xyz": xyz, "rgb": rgb, "tri": tri}

    def pass_ms(self):
        """device ms: {"integrate"} of the last integrate call, {"mark", "scan", "vertices", "triangles"} of the last mesh call"""
        ms = (C.c_float * 5)()
        rc = self._f["tsdf_pass_ms"](self._h, ms)
        if rc != 0:
            _raise(self._f, "tsdf_pass_ms", rc)
        return dict(zip(("integrate", "mark", "scan", "vertices", "triangles"), (float(v) for v in ms)))


class SparseVolume(Volume):
    """mpmvs_tsdf_create_sparse: the lattice of Volume with virtual dims, of which only bricks of 8 x 8 x 8 voxels exist
    (include/mpmvs.h, statements A and B).  allocate() marks the bricks within `pad` voxels of the samples
    along every depth pixel's ray through the truncation band; integrate() and mesh() are the dense calls on the existing voxels.
    Everything comes out in brick-major order: bricks ascending by (K*by + J)*bx + I, voxels within a brick by (lk*8 + lj)*8 + li.
    pad = 1.0 is an untuned starting value.  max_bricks (default: the whole brick grid, at most 2^21) caps the pool; memory is
    taken only for the bricks that exist."""

    def __init__(self, origin, voxel, dims, trunc, color=False, pad=1.0, max_bricks=None, device=0):
        _, self._f = engine.load()
        self._h = None
        o = np.ascontiguousarray(origin, np.float32)
        d = np.ascontiguousarray(dims, np.int32)
        if o.shape != (3,) or d.shape != (3,):
            raise ValueError(f"need an origin and dims of 3 numbers each, got {o.shape} and {d.shape}")
        grid = tuple((int(v) + 7) // 8 for v in d)
        if max_bricks is None:
            max_bricks = max(1, min(grid[0] * grid[1] * grid[2], 1 << 21))
        h = C.c_void_p()
        rc = self._f["tsdf_create_sparse"](int(device), o.ctypes.data_as(C.POINTER(C.c_float)), float(voxel), d.ctypes.data_as(C.POINTER(C.c_int)), float(trunc),
                                           1 if color else 0, float(pad), int(max_bricks), C.byref(h))
        if rc != 0:
            _raise(self._f, "tsdf_create_sparse", rc)
        self._h = h
        self.origin, self.voxel, self.trunc, self.color, self.device = o, float(np.float32(voxel)), float(np.float32(trunc)), bool(color), int(device)
        self.dims = tuple(int(v) for v in d)
        self.n_vox = self.dims[0] * self.dims[1] * self.dims[2]   # virtual
        self.grid, self.pad, self.max_bricks = grid, float(np.float32(pad)), int(max_bricks)

    def allocate(self, cams, depths):
        """mpmvs_tsdf_allocate: adds the bricks that the views' depth maps reach (statement A); existing bricks stay.  ValueError
        (-3) if that needs more than max_bricks; nothing is allocated then."""
        cams = list(cams)
        n = len(cams)
        if len(depths) != n:
            raise ValueError("need one depth map per camera")
        ds = [np.ascontiguousarray(d, np.float32) for d in depths]
        for c, d in zip(cams, ds):
            if d.shape != (int(c.height), int(c.width)):
                raise ValueError(f"a depth map of shape {d.shape} for a camera of {int(c.height)} x {int(c.width)}")
        arr = (_abi.Camera * max(n, 1))(*cams)
        dp = (C.c_void_p * max(n, 1))(*[d.ctypes.data for d in ds])
        rc = self._f["tsdf_allocate"](self._h, n, arr, dp)
        if rc != 0:
            _raise(self._f, "tsdf_allocate", rc)

    def bricks(self):
        """int32 [n, 3]: (I, J, K) of the allocated bricks in ascending linear index"""
        lib, _ = engine.load()
        lib.mpmvs_free.argtypes = [C.c_void_p]
        lib.mpmvs_free.restype = None
        p = C.c_void_p()
        n = self._f["tsdf_bricks"](self._h, C.byref(p))
        if n < 0:
            _raise(self._f, "tsdf_bricks", n)
        try:
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), (n, 3)).copy() if n else np.zeros((0, 3), np.int32)
        finally:
            if p.value:
                lib.mpmvs_free(p)

    def n_bricks(self):
        n = self._f["tsdf_bricks"](self._h, None)
        if n < 0:
            _raise(self._f, "tsdf_bricks", n)
        return int(n)

    def get_bricks(self):
        """{"coords": int32 [n, 3], "sum": float32 [n, 8, 8, 8] (indexed [brick, lk, lj, li]), "weight": int32 [n, 8, 8, 8]} and, with
        colour, "color": uint32 [n, 8, 8, 8, 4]; voxels cut off by dims read 0"""
        coords = self.bricks()
        n = len(coords)
        out = {"coords": coords, "sum": np.zeros((n, 8, 8, 8), np.float32), "weight": np.zeros((n, 8, 8, 8), np.int32)}
        if self.color:
            out["color"] = np.zeros((n, 8, 8, 8, 4), np.uint32)
        if n:
            rc = self._f["tsdf_get_bricks"](self._h, out["sum"].ctypes.data, out["weight"].ctypes.data, out["color"].ctypes.data if self.color else None)
            if rc != 0:
                _raise(self._f, "tsdf_get_bricks", rc)
        return out

    def set_bricks(self, coords, sum, weight, color=None):
        """replaces the whole volume: coords int32 [n, 3] strictly ascending by linear index, 512 entries per brick and array"""
        c = np.ascontiguousarray(coords, np.int32).reshape(-1, 3)
        n = len(c)
        s, w = np.ascontiguousarray(sum, np.float32), np.ascontiguousarray(weight, np.int32)
        col = np.ascontiguousarray(color, np.uint32) if color is not None else None
        if s.size != 512 * n or w.size != 512 * n or (col is not None and col.size != 2048 * n):
            raise ValueError(f"need 512 sums and weights (and four colour entries per voxel) for each of the {n} bricks")
        rc = self._f["tsdf_set_bricks"](self._h, n, c.ctypes.data if n else None, s.ctypes.data if n else None, w.ctypes.data if n else None,
                                        col.ctypes.data if col is not None and n else None)
        if rc != 0:
            _raise(self._f, "tsdf_set_bricks", rc)

    def get(self):
        raise ValueError("a brick-sparse volume is read with get_bricks() or to_dense()")

    def set(self, sum, weight, color=None):
        raise ValueError("a brick-sparse volume is written with set_bricks()")

    def to_dense(self):
        """the volume scattered into dense arrays on the host, as Volume.get() returns them, non-existing voxels zero; for small
        volumes (at most 2^27 voxels)"""
        if self.n_vox > 1 << 27:
            raise ValueError(f"to_dense: {self.n_vox} voxels, more than 2^27")
        nx, ny, nz = self.dims
        b = self.get_bricks()
        out = {"sum": np.zeros((nz, ny, nx), np.float32), "weight": np.zeros((nz, ny, nx), np.int32)}
        if self.color:
            out["color"] = np.zeros((nz, ny, nx, 4), np.uint32)
        for r, (I, J, K) in enumerate(b["coords"]):
            sx, sy, sz = min(8, nx - 8 * I), min(8, ny - 8 * J), min(8, nz - 8 * K)
            for key in out:
                out[key][8 * K:8 * K + sz, 8 * J:8 * J + sy, 8 * I:8 * I + sx] = b[key][r, :sz, :sy, :sx]
        return out

    def stats(self):
        """{"bricks", "max_bricks", "grid_cells", "device_bytes", "brick_share"} and the device ms of the last allocate:
        {"allocate_mark", "allocate_commit"}"""
        info, ms = (C.c_longlong * 4)(), (C.c_float * 2)()
        rc = self._f["tsdf_sparse_stats"](self._h, info, ms)
        if rc != 0:
            _raise(self._f, "tsdf_sparse_stats", rc)
        return {"bricks": int(info[0]), "max_bricks": int(info[1]), "grid_cells": int(info[2]), "device_bytes": int(info[3]),
                "brick_share": float(info[0]) / float(info[2]), "allocate_mark": float(ms[0]), "allocate_commit": float(ms[1])}


PLACEMENTS = {"mean": 0, "quadric": 1}
SIMPLIFY_PASSES = ("cluster", "position_accumulate", "quadric_accumulate", "place", "classify_insert", "flag_scan", "emit")


class Mesh:
    """mpmvs_mesh: an indexed triangle mesh resident on the device: xyz float32 [n, 3], tri int32 [m, 3] with indices in [0, n),
    rgb uint8 [n, 3] or None (include/mpmvs.h, statements 1 to 3).  Wherever the mesh came from: Volume.mesh()
    or read_ply_mesh().  The arrays are copied; the device is opened by the first call that needs it."""

    def __init__(self, xyz, tri, rgb=None, device=0):
        _, self._f = engine.load()
        self._h = None
        x = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
        c = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3) if rgb is not None else None
        if c is not None and len(c) != len(x):
            raise ValueError(f"{len(c)} colours for {len(x)} vertices")
        if c is not None and len(x) == 0:
            c = np.zeros((1, 3), np.uint8)   # a pointer that is not NULL: the mesh has colour
        h = C.c_void_p()
        rc = self._f["mesh_create"](int(device), len(x), x.ctypes.data if len(x) else None, c.ctypes.data if c is not None else None, len(t),
                                    t.ctypes.data if len(t) else None, C.byref(h))
        if rc != 0:
            _raise(self._f, "mesh_create", rc)
        self._h = h
        self.n, self.m, self.color, self.device = len(x), len(t), rgb is not None, int(device)

    def close(self):
        if self._h is not None:
            self._f["mesh_destroy"](self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def components(self, want_verts=True, want_tris=True):
        """mpmvs_mesh_components -> (label int32 [n], verts int32 [n] or None, tris int32 [n] or None, counts): the smallest vertex
        index of each vertex's component, its vertex and triangle counts, and counts = {"components", "unnamed",
        "largest_triangles", "largest_label"}.  Connectivity is by index: coincident vertices are not welded."""
        label = np.empty(self.n, np.int32)
        verts = np.empty(self.n, np.int32) if want_verts else None
        tris = np.empty(self.n, np.int32) if want_tris else None
        counts = (C.c_longlong * 4)()
        rc = self._f["mesh_components"](self._h, label.ctypes.data, verts.ctypes.data if want_verts else None, tris.ctypes.data if want_tris else None, counts)
        if rc != 0:
            _raise(self._f, "mesh_components", rc)
        return label, verts, tris, dict(zip(("components", "unnamed", "largest_triangles", "largest_label"), (int(v) for v in counts)))

    def normals(self):
        """mpmvs_mesh_normals -> (float32 [n, 3], n_defined): the area-weighted vertex normals, (0, 0, 0) where undefined"""
        out = np.empty((self.n, 3), np.float32)
        nd = C.c_longlong(0)
        rc = self._f["mesh_normals"](self._h, out.ctypes.data, C.byref(nd))
        if rc != 0:
            _raise(self._f, "mesh_normals", rc)
        return out, int(nd.value)

    def select(self, keep, drop_unreferenced=True):
        """mpmvs_mesh_select -> {"xyz", "rgb", "tri", "src"}: the vertices with keep[v] != 0 (and, with drop_unreferenced, a kept
        triangle), the triangles whose three vertices are kept, renumbered in order; src[new] = old.  The handle is unchanged."""
        k = np.ascontiguousarray(keep).reshape(-1)
        if len(k) != self.n:
            raise ValueError(f"a mask of {len(k)} entries for {self.n} vertices")
        k = np.ascontiguousarray(k != 0, np.uint8)
        lib, _ = engine.load()
        lib.mpmvs_free.argtypes = [C.c_void_p]
        lib.mpmvs_free.restype = None
        px, pc, pt, ps, mo = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_longlong(0)
        nv = self._f["mesh_select"](self._h, k.ctypes.data if self.n else None, 1 if drop_unreferenced else 0, C.byref(px), C.byref(pc) if self.color else None,
                                    C.byref(pt), C.byref(ps), C.byref(mo))
        if nv < 0:
            _raise(self._f, "mesh_select", nv)
        try:
            def take(p, ctype, rows, cols, dtype):
                if not rows:
                    return np.zeros((0, cols) if cols > 1 else (0,), dtype)
                return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), (rows, cols) if cols > 1 else (rows,)).copy()
            out = {"xyz": take(px, C.c_float, nv, 3, np.float32), "rgb": take(pc, C.c_uint8, nv, 3, np.uint8) if self.color else None,
                   "tri": take(pt, C.c_int32, mo.value, 3, np.int32), "src": take(ps, C.c_int32, nv, 1, np.int32)}
        finally:
            for p in (px, pc, pt, ps):
                if p.value:
                    lib.mpmvs_free(p)
        return out

    def simplify(self, cell, placement="quadric"):
        """mpmvs_simplify_mesh -> {"xyz", "rgb", "tri", "cluster_of", "count", "placed", "tri_src", "counts"}: vertex clustering on a
        grid of edge `cell`; one vertex per occupied cell, at the mean of its members (placement="mean") or where its plane quadric
        is smallest inside the cell ("quadric"; placed[k] = 1 where that was used, 2 where it fell back to the mean, 0 where the
        cluster has no plane).  Collapsed and duplicate triangles go; tri_src[new] = old; counts = {"non_finite", "collapsed",
        "duplicates"}.  Clusters no kept triangle names stay in the result.  The handle is unchanged."""
        if placement not in PLACEMENTS:
            raise ValueError(f"placement must be one of {sorted(PLACEMENTS)}, not {placement!r}")
        lib, _ = engine.load()
        lib.mpmvs_free.argtypes = [C.c_void_p]
        lib.mpmvs_free.restype = None
        px, pc, pt, pn, pp, ps = (C.c_void_p() for _ in range(6))
        mo, counts = C.c_longlong(0), (C.c_longlong * 3)()
        cluster_of = np.empty(self.n, np.int32)
        nc = self._f["simplify_mesh"](self._h, float(cell), PLACEMENTS[placement], C.byref(px), C.byref(pc) if self.color else None, C.byref(pt), C.byref(mo),
                                      cluster_of.ctypes.data if self.n else None, C.byref(pn), C.byref(pp), C.byref(ps), counts)
        if nc < 0:
            _raise(self._f, "simplify_mesh", nc)
        try:
            def take(p, ctype, rows, cols, dtype):
                if not rows:
                    return np.zeros((0, cols) if cols > 1 else (0,), dtype)
                return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), (rows, cols) if cols > 1 else (rows,)).copy()
            out = {"xyz": take(px, C.c_float, nc, 3, np.float32), "rgb": take(pc, C.c_uint8, nc, 3, np.uint8) if self.color else None,
                   "tri": take(pt, C.c_int32, mo.value, 3, np.int32), "cluster_of": cluster_of, "count": take(pn, C.c_int32, nc, 1, np.int32),
                   "placed": take(pp, C.c_uint8, nc, 1, np.uint8), "tri_src": take(ps, C.c_int32, mo.value, 1, np.int32),
                   "counts": dict(zip(("non_finite", "collapsed", "duplicates"), (int(v) for v in counts)))}
        finally:
            for p in (px, pc, pt, pn, pp, ps):
                if p.value:
                    lib.mpmvs_free(p)
        return out

    def distance(self, cloud, radius, want_tri=True):
        """mpmvs_surface_distance -> (d2 float32 [N], tri int32 [N]), or d2 alone with want_tri=False: per point of `cloud` (a
        cloud.Cloud on the same device) the squared distance to the nearest point of this mesh's surface within `radius` and the
        triangle that holds it; inf / -1 where there is none.  self.last_counts = {"with_candidate", "taking_part"} of the call."""
        d2 = np.empty(cloud.n, np.float32)
        tri = np.empty(cloud.n, np.int32) if want_tri else None
        counts = (C.c_longlong * 2)()
        rc = self._f["surface_distance"](self._h, cloud._h, float(radius), d2.ctypes.data if cloud.n else None, tri.ctypes.data if want_tri and cloud.n else None,
                                         counts)
        if rc != 0:
            _raise(self._f, "surface_distance", rc)
        self.last_counts = {"with_candidate": int(counts[0]), "taking_part": int(counts[1])}
        return (d2, tri) if want_tri else d2

    def distance_ms(self):
        """device ms of the last distance call: {"total", "init", "scatter", "finish"}; the grid build stays with Cloud.kernel_ms()"""
        ms = (C.c_float * 3)()
        total = self._f["surface_distance_ms"](self._h, ms)
        return {"total": float(total), "init": float(ms[0]), "scatter": float(ms[1]), "finish": float(ms[2])}

    def sample(self, spacing, want_normals=False):
        """mpmvs_surface_sample -> {"xyz" float32 [K, 3], "tri_of" int32 [K], "rgb" uint8 [K, 3] or None, "normals" float32 [K, 3] or
        None}: the centroids of the regular subdivision of every triangle whose longest sub-edge is at most `spacing`, so that every
        point of the surface lies within 2/3 * spacing of a sample; triangle by triangle, in a fixed order."""
        lib, _ = engine.load()
        lib.mpmvs_free.argtypes = [C.c_void_p]
        lib.mpmvs_free.restype = None
        px, po, pc, pn = (C.c_void_p() for _ in range(4))
        k = self._f["surface_sample"](self._h, float(spacing), C.byref(px), C.byref(po), C.byref(pc) if self.color else None, C.byref(pn) if want_normals else None)
        if k < 0:
            _raise(self._f, "surface_sample", k)
        try:
            def take(p, ctype, cols, dtype):
                if not k:
                    return np.zeros((0, cols) if cols > 1 else (0,), dtype)
                return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), (k, cols) if cols > 1 else (k,)).copy()
            out = {"xyz": take(px, C.c_float, 3, np.float32), "tri_of": take(po, C.c_int32, 1, np.int32),
                   "rgb": take(pc, C.c_uint8, 3, np.uint8) if self.color else None, "normals": take(pn, C.c_float, 3, np.float32) if want_normals else None}
        finally:
            for p in (px, po, pc, pn):
                if p.value:
                    lib.mpmvs_free(p)
        return out

    def sample_ms(self):
        """device ms of the last sample call: {"total", "count", "scan", "emit"}"""
        ms = (C.c_float * 3)()
        total = self._f["surface_sample_ms"](self._h, ms)
        return {"total": float(total), "count": float(ms[0]), "scan": float(ms[1]), "emit": float(ms[2])}

    def render_depth(self, cams, want_tri=False):
        """mpmvs_surface_render_depth: the mesh rasterised into every camera of `cams` (_abi.Camera; width and height give the map's
        size) -> a list of float32 [H, W] depth maps along the camera's z axis, 0 = no depth; with want_tri=True (depths, tris),
        tris a list of int32 [H, W] maps of the triangle each pixel shows (-1 = none).  Per pixel the nearest surface along its ray
        (pixel centres at integers), both windings, no parameter; a triangle that crosses the camera plane is rendered unclipped.
        self.last_render_counts = {"pairs", "covered", "large_pairs"} of the call."""
        cams = list(cams)
        n = len(cams)
        arr = (_abi.Camera * max(n, 1))(*cams)
        depths = [np.empty((max(int(c.height), 0), max(int(c.width), 0)), np.float32) for c in cams]
        tris = [np.empty(d.shape, np.int32) for d in depths] if want_tri else None
        dp = (C.c_void_p * max(n, 1))(*[d.ctypes.data for d in depths])
        tp = (C.c_void_p * max(n, 1))(*[t.ctypes.data for t in tris]) if want_tri else None
        counts = (C.c_longlong * 3)()
        rc = self._f["surface_render_depth"](self._h, n, arr, dp, tp, counts)
        if rc != 0:
            _raise(self._f, "surface_render_depth", rc)
        self.last_render_counts = {"pairs": int(counts[0]), "covered": int(counts[1]), "large_pairs": int(counts[2])}
        return (depths, tris) if want_tri else depths

    def render_ms(self):
        """device ms of the last render_depth call's kernels: (total, {"init", "small", "large", "resolve"})"""
        ms = (C.c_float * 4)()
        total = self._f["surface_render_ms"](self._h, ms)
        return float(total), dict(zip(("init", "small", "large", "resolve"), (float(v) for v in ms)))

    def render_work(self):
        """diagnostics of the last render_depth call: {"box_pixels": the pixels of the boxes the pairs were tested in, "atomics": the
        atomic minima issued (it depends on the order of the threads)}"""
        w = (C.c_longlong * 2)()
        rc = self._f["surface_render_work"](self._h, w)
        if rc != 0:
            _raise(self._f, "surface_render_work", rc)
        return {"box_pixels": int(w[0]), "atomics": int(w[1])}

    def simplify_ms(self):
        """device ms of the last simplify call, pass by pass"""
        ms = (C.c_float * 7)()
        rc = self._f["simplify_mesh_ms"](self._h, ms)
        if rc != 0:
            _raise(self._f, "simplify_mesh_ms", rc)
        return dict(zip(SIMPLIFY_PASSES, (float(v) for v in ms)))

    def pass_ms(self):
        """device ms of the last components, normals and select calls"""
        ms = (C.c_float * 8)()
        rc = self._f["mesh_pass_ms"](self._h, ms)
        if rc != 0:
            _raise(self._f, "mesh_pass_ms", rc)
        return dict(zip(("cc_hook", "cc_flatten", "cc_sizes", "normals_accumulate", "normals_finish", "select_flag", "select_scan", "select_emit"),
                        (float(v) for v in ms)))


def rank_components(label, tris, min_triangles=1, largest=None):
    """the keep mask of remove_small_components from the labels and per-vertex triangle counts of Mesh.components(): the vertices of
    the components with at least min_triangles triangles (never fewer than 1: a vertex no triangle names goes) and, with
    largest=K, of only the K largest of them by triangle count, ties to the smaller label.  Host work."""
    label, tris = np.asarray(label, np.int64), np.asarray(tris, np.int64)
    roots = np.flatnonzero((label == np.arange(len(label))) & (tris >= max(int(min_triangles), 1)))
    if largest is not None:
        if largest < 0:
            raise ValueError("largest must not be negative")
        roots = roots[np.argsort(-tris[roots], kind="stable")[:largest]]   # roots ascend: a stable sort sends ties to the smaller label
    good = np.zeros(len(label), bool)
    good[roots] = True
    return good[label] if len(label) else good


def remove_small_components(m, min_triangles=1, largest=None, device=0):
    """m: a mesh dict {"xyz", "tri", "rgb"}.  Keeps the components with at least min_triangles triangles; with largest=K only the K
    largest by triangle count, ties to the smaller label (the rule of cloud.remove_small_clusters).  Vertices no triangle names are
    dropped.  Returns the selected mesh dict {"xyz", "rgb", "tri", "src"} plus "keep" (bool [n]), "label", "tris", "counts".  The
    union-find and the compaction run on the device; the ranking is host work on the downloaded labels."""
    with Mesh(m["xyz"], m["tri"], m.get("rgb"), device=device) as h:
        label, _, tris, counts = h.components(want_verts=False)
        keep = rank_components(label, tris, min_triangles, largest)
        out = h.select(keep, drop_unreferenced=True)
        out["device_ms"] = h.pass_ms()
    out.update({"keep": keep, "label": label, "tris": tris, "counts": counts})
    return out


def vertex_normals(m, device=0):
    """m: a mesh dict -> (float32 [n, 3], n_defined): Mesh.normals() of it"""
    with Mesh(m["xyz"], m["tri"], None, device=device) as h:
        return h.normals()


def clean_and_shade(m, min_component=0, largest=None, normals=False, device=0):
    """what tools/mesh_ply.py and tools/clean_mesh.py do to a mesh dict after their flags: cleaned first (if min_component > 0 or
    largest is given), then shaded (if normals) -> ({"mesh": the mesh dict, "device_ms": {...}, and only for what was asked:
    "components", "largest_component", "removed_triangles", "normals_defined"}, normals or None)"""
    info, ms, nrm = {}, {}, None
    if min_component > 0 or largest is not None:
        before = len(m["tri"])
        c = remove_small_components(m, max(int(min_component), 1), largest, device=device)
        ms.update({k: v for k, v in c["device_ms"].items() if k.startswith(("cc_", "select_"))})
        info.update(components=c["counts"]["components"], largest_component=c["counts"]["largest_triangles"], removed_triangles=before - len(c["tri"]))
        m = {"xyz": c["xyz"], "rgb": c["rgb"], "tri": c["tri"]}
    if normals:
        with Mesh(m["xyz"], m["tri"], None, device=device) as h:
            nrm, info["normals_defined"] = h.normals()
            ms.update({k: v for k, v in h.pass_ms().items() if k.startswith("normals_")})
    info.update(mesh=m, device_ms=ms)
    return info, nrm


def simplify(m, cell, placement="quadric", drop_unreferenced=True, normals=False, device=0):
    """m: a mesh dict {"xyz", "tri", "rgb"}.  Mesh.simplify on it; with drop_unreferenced the clusters that no kept triangle names are
    removed (Mesh.select on the new mesh; "src"[new] = the cluster number); with normals the vertex normals of the new mesh.
    Returns the new mesh dict {"xyz", "rgb", "tri"} plus "cluster_of", "count", "placed" (all three by cluster number), "tri_src",
    "counts", "src" (or None), "normals" and "normals_defined" (or None) and "device_ms"."""
    with Mesh(m["xyz"], m["tri"], m.get("rgb"), device=device) as h:
        out = h.simplify(cell, placement)
        ms = h.simplify_ms()
    out.update(src=None, normals=None, normals_defined=None)
    if drop_unreferenced or normals:
        with Mesh(out["xyz"], out["tri"], out["rgb"], device=device) as h:
            if drop_unreferenced:
                sel = h.select(np.ones(h.n, np.uint8), drop_unreferenced=True)
                out.update(xyz=sel["xyz"], rgb=sel["rgb"], tri=sel["tri"], src=sel["src"])
                ms.update({k: v for k, v in h.pass_ms().items() if k.startswith("select_")})
        if normals:
            with Mesh(out["xyz"], out["tri"], None, device=device) as h:
                out["normals"], out["normals_defined"] = h.normals()
                ms.update({k: v for k, v in h.pass_ms().items() if k.startswith("normals_")})
    out["device_ms"] = ms
    return out


def surface_distances(points, mesh_handle, tolerances, device=0, on_level=None):
    """float32 [n]: per point the exact distance to the surface of `mesh_handle` (a Mesh) where that is within max(tolerances), else
    inf: cloud.distances with a mesh as the target.  The same cascade: tolerances ascending, one Mesh.distance call per tolerance
    with radius = tolerance, and only the points still unresolved go on.  A point with a candidate at one level is final, because a
    nearer triangle would be within that radius too.  The scatter of a triangle costs with the points in the cells around it, which
    grow with the cube of the radius, so a coarse level should see few points; but a cloud handle of its own per level costs more
    than the level itself while most points are still in play (the measurement is in DESIGN.md section 26.5).  So the resident cloud
    is kept from level to level and replaced by one of the unresolved points only once those are fewer than half of it.
    on_level(tolerance, n_points, mesh_handle), if given, is called after every level."""
    q = _cloud._xyz(points)
    out = np.full(len(q), np.inf, np.float32)
    left = np.arange(len(q))
    held, sub = None, None   # the points the resident cloud holds, and the cloud
    try:
        for t in sorted(set(float(t) for t in tolerances)):
            if len(left) == 0:
                break
            if sub is None or 2 * len(left) < len(held):
                if sub is not None:
                    sub.close()
                held, sub = left, _cloud.Cloud(q[left], device)
            d2 = mesh_handle.distance(sub, t, want_tri=False)
            if on_level:
                on_level(t, len(held), mesh_handle)
            d2 = d2[np.searchsorted(held, left)]   # held ascends and holds every unresolved point
            hit = np.isfinite(d2)
            out[left[hit]] = np.sqrt(d2[hit])
            left = left[~hit]
    finally:
        if sub is not None:
            sub.close()
    return out


def evaluate_mesh(m, gt_xyz, tolerances, spacing=None, voxel=None, device=0, timings=None):
    """Accuracy, completeness and F1 of a mesh dict {"xyz", "tri"} against a ground-truth cloud: the dict of cloud.score.
    Accuracy: the samples of the mesh (Mesh.sample at `spacing`; resampled with cloud.voxel_downsample first when `voxel` is given)
    against the scan, through Cloud.nearest (cloud.distances).  Completeness: the scan's points against the SURFACE of the mesh
    (surface_distances), not against its vertices or samples.  Points of the scan with a non-finite coordinate are dropped and
    counted.  spacing defaults to the smallest tolerance, so that no point of the surface is farther than two thirds of it from a
    sample: an untuned starting value.  The result also holds "spacing", "n_samples" and, with voxel, "voxel".
    timings (a dict, optional) receives "sample_s", "accuracy_s", "completeness_s" (wall) and "device_ms" per stage."""
    import time
    tol = [float(t) for t in tolerances]
    if not tol or not all(np.isfinite(t) and t > 0 for t in tol):
        raise ValueError("tolerances must be finite and positive")
    spacing = min(tol) if spacing is None else float(spacing)
    if not (np.isfinite(spacing) and spacing > 0):
        raise ValueError("spacing must be finite and positive")
    if voxel is not None and not (np.isfinite(voxel) and voxel > 0):
        raise ValueError("voxel must be finite and positive")
    gt, drop_g = _cloud.drop_nonfinite(gt_xyz)
    ms = {}
    with Mesh(m["xyz"], m["tri"], None, device=device) as h:
        t0 = time.perf_counter()
        smp = h.sample(spacing)["xyz"]
        ms["sample"] = h.sample_ms()["total"]
        n_samples = len(smp)
        if voxel is not None:
            smp = _cloud.voxel_downsample(smp, voxel, device=device)["xyz"]
        t1 = time.perf_counter()
        with _cloud.Cloud(gt, device) as c_gt:
            d_rec = _cloud.distances(smp, c_gt, tol)
        t2 = time.perf_counter()
        ms["distance"] = 0.0

        def on_level(t, n, mh):
            ms["distance"] += mh.distance_ms()["total"]

        d_gt = surface_distances(gt, h, tol, device=device, on_level=on_level)
        t3 = time.perf_counter()
    res = _cloud.score(d_rec, d_gt, tol, (0, drop_g))
    res.update(spacing=spacing, n_samples=n_samples)
    if voxel is not None:
        res["voxel"] = float(voxel)
    if timings is not None:
        timings.update(sample_s=t1 - t0, accuracy_s=t2 - t1, completeness_s=t3 - t2, device_ms=ms)
    return res


def triangle_coverage(tri_maps, m):
    """int64 [n_views, m]: the pixels each of the m triangles shows in each view, from the triangle-id maps of Mesh.render_depth
    (-1 = none): the visibility table that colouring a mesh from its images, or culling what no camera saw, starts from.  Host work."""
    out = np.zeros((len(tri_maps), int(m)), np.int64)
    for v, t in enumerate(tri_maps):
        t = np.asarray(t).reshape(-1)
        t = t[t >= 0]
        if len(t) and int(t.max()) >= m:
            raise ValueError(f"view {v} names triangle {int(t.max())}, the mesh has {m}")
        out[v] = np.bincount(t, minlength=int(m))
    return out


def _direction(d2):
    """the sums of one direction of compare() from the squared distances of Mesh.distance, on the host in fp64"""
    d2 = np.asarray(d2, np.float64)
    within = np.isfinite(d2)
    d = np.sqrt(d2[within])
    return {"n": int(d2.size), "beyond": int((~within).sum()), "max": float(d.max()) if d.size else None, "mean": float(d.mean()) if d.size else None,
            "rms": float(np.sqrt((d * d).mean())) if d.size else None}


def compare(m_a, m_b, spacing, radius, device=0):
    """How far two mesh dicts are apart, as surfaces: {"a_to_b", "b_to_a", "hausdorff", "spacing", "radius"}.  Per direction, over the
    samples of one mesh (Mesh.sample at `spacing`) against the surface of the other (Mesh.distance at `radius`): "n" samples, "beyond"
    (no point of the other surface within the radius), and "max", "mean" and "rms" of the distances within it (None when there is
    none).  "hausdorff" is the larger of the two maxima: the Hausdorff distance of the sample sets to the surfaces, capped at the
    radius -- a direction with samples beyond it says that the true value is larger.  The sums are taken on the host in fp64."""
    out = {"spacing": float(spacing), "radius": float(radius)}
    with Mesh(m_a["xyz"], m_a["tri"], None, device=device) as ha, Mesh(m_b["xyz"], m_b["tri"], None, device=device) as hb:
        for name, src, dst in (("a_to_b", ha, hb), ("b_to_a", hb, ha)):
            with _cloud.Cloud(src.sample(spacing)["xyz"], device) as c:
                out[name] = _direction(dst.distance(c, radius, want_tri=False))
    tops = [out[k]["max"] for k in ("a_to_b", "b_to_a") if out[k]["max"] is not None]
    out["hausdorff"] = max(tops) if tops else None
    return out


def write_ply_mesh(path, xyz, tri, rgb=None, normals=None):
    """binary little-endian PLY: vertex x y z (float), with normals nx ny nz (float) and, with rgb, red green blue (uchar); face: list
    uchar int vertex_indices"""
    xyz, tri = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3), np.ascontiguousarray(tri, np.int32).reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(xyz)}", "property float x", "property float y", "property float z"]
    if normals is not None:
        normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        if len(normals) != len(xyz):
            raise ValueError(f"{len(normals)} normals for {len(xyz)} vertices")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        head += ["property float nx", "property float ny", "property float nz"]
    if rgb is not None:
        rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
        if len(rgb) != len(xyz):
            raise ValueError(f"{len(rgb)} colours for {len(xyz)} vertices")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    if len(tri) and (tri.min() < 0 or tri.max() >= len(xyz)):
        raise ValueError("a triangle names a vertex that does not exist")
    head += [f"element face {len(tri)}", "property list uchar int vertex_indices", "end_header"]
    v = np.empty(len(xyz), np.dtype(fields))
    for a, name in enumerate("xyz"):
        v[name] = xyz[:, a]
    if normals is not None:
        for a, name in enumerate(("nx", "ny", "nz")):
            v[name] = normals[:, a]
    if rgb is not None:
        for a, name in enumerate(("red", "green", "blue")):
            v[name] = rgb[:, a]
    f = np.empty(len(tri), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    f["n"] = 3
    f["v"] = tri
    with open(path, "wb") as out:
        out.write(("\n".join(head) + "\n").encode("ascii"))
        out.write(v.tobytes())
        out.write(f.tobytes())


def read_ply_mesh(path):
    """what write_ply_mesh writes -> {"xyz": float32 [n, 3], "rgb": uint8 [n, 3] or None, "tri": int32 [m, 3], "normals": float32
    [n, 3] or None}.  Binary little-endian files with float x y z (then float nx ny nz, then uchar red green blue) per vertex and
    triangles only; anything else is a ValueError."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    nl = data.find(b"\n", end)
    if not data.startswith(b"ply") or end < 0 or nl < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = [ln.split() for ln in data[:end].decode("ascii", "replace").splitlines()[1:] if ln.strip() and ln.split()[0] != "comment"]
    if not lines or lines[0] != ["format", "binary_little_endian", "1.0"]:
        raise ValueError(f"{path}: only binary_little_endian 1.0 mesh files are read")
    elements = []
    for w in lines[1:]:
        if w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property" and elements:
            elements[-1][2].append(tuple(w[1:]))
        else:
            raise ValueError(f"{path}: unknown header line {' '.join(w)!r}")
    plain = [("float", "x"), ("float", "y"), ("float", "z")]
    shaded = [("float", "nx"), ("float", "ny"), ("float", "nz")]
    colour = [("uchar", "red"), ("uchar", "green"), ("uchar", "blue")]
    layouts = (plain, plain + colour, plain + shaded, plain + shaded + colour)
    if len(elements) != 2 or elements[0][0] != "vertex" or elements[1][0] != "face" or elements[0][2] not in layouts \
            or elements[1][2] != [("list", "uchar", "int", "vertex_indices")]:
        raise ValueError(f"{path}: not the layout of write_ply_mesh")
    nv, nf = elements[0][1], elements[1][1]
    has_nrm, has_rgb = shaded[0] in elements[0][2], colour[0] in elements[0][2]
    vdt = np.dtype([("xyz", "<f4", (3,))] + ([("nrm", "<f4", (3,))] if has_nrm else []) + ([("rgb", "u1", (3,))] if has_rgb else []))
    fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    at = nl + 1
    if at + nv * vdt.itemsize + nf * fdt.itemsize > len(data):
        raise ValueError(f"{path}: truncated body")
    v = np.frombuffer(data, vdt, nv, at)
    f = np.frombuffer(data, fdt, nf, at + nv * vdt.itemsize)
    if nf and (f["n"] != 3).any():
        raise ValueError(f"{path}: a face that is no triangle")
    return {"xyz": v["xyz"].copy().reshape(-1, 3), "rgb": v["rgb"].copy().reshape(-1, 3) if has_rgb else None, "tri": f["v"].copy().reshape(-1, 3),
            "normals": v["nrm"].copy().reshape(-1, 3) if has_nrm else None}
