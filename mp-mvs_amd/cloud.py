"""Point clouds: reading PLY files, the exact capped nearest-neighbour search on the GPU (mpmvs_cloud_*, csrc/pm_cloud.hpp),
the accuracy / completeness / F1 score of a fused cloud against a ground-truth scan and the z-buffer
render of a cloud into cameras (Cloud.render_depth, csrc/pm_render.hpp), and the registration of a
cloud to a target before it is scored: point-to-point ICP with a scale on the GPU (Aligner, solve, align; csrc/pm_align.hpp,
DESIGN.md section 15), and the voxel-grid downsampling of a cloud on the GPU (voxel_downsample; csrc/pm_voxel.hpp, DESIGN.md
section 16), and the k nearest neighbours within a cloud with the statistical / radius outlier filter on top of them (Cloud.knn,
Cloud.knn_self, remove_outliers; csrc/pm_knn.hpp), and a surface normal per point fitted to those neighbours
(Cloud.normals, estimate_normals; csrc/pm_normals.hpp), and point-to-plane ICP on those normals beside the
point-to-point one (Aligner.set_normals / plane_sums / plane_icp, plane_solve, align(method="plane"); csrc/pm_align_plane.hpp,
DESIGN.md section 19), and the connected components of a cloud under "within a radius", with the filter that drops small detached
clusters on top of them (Cloud.components, remove_small_clusters; csrc/pm_components.hpp), and the space the
scanners of a scan observed, as a range cube map per scanner position against which points are classified (Observer,
score_observed, evaluate(scanners=...), read_scan_alignment; csrc/pm_observe.hpp).

The score is the plain two-way nearest-neighbour measure (Tanks-and-Temples style).  Both clouds can be resampled on a voxel
grid first (evaluate(voxel=...)), as Tanks and Temples and ETH3D's official program do.  ETH3D's program additionally masks
the space the scanner did not observe; evaluate(scanners=...) does observed-space masking in our own formulation, not verified
against ETH3D's program, so the numbers are comparable between our own builds and settings, and not to the ETH3D leaderboard.
The search runs on the GPU; there is no CPU path."""
import ctypes as C
import math
import weakref

import numpy as np

from . import _abi, engine

_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply(path):
    """The `vertex` element of a binary_little_endian or ascii PLY file -> {"xyz": float32 [n, 3]} plus "normals" (float32
    [n, 3], from nx ny nz) and "colors" (uint8 [n, 3], from red green blue) when the file has them.  Other properties and
    other elements are skipped by their declared sizes; list properties inside `vertex` and big-endian files are refused
    (ValueError).  Reads back what hostlib.write_ply writes (the reference's 27-byte records)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header")
    nl = data.find(b"\n", end)
    if not data.startswith(b"ply") or end < 0 or nl < 0:
        raise ValueError(f"{path}: not a PLY file (no 'ply' ... 'end_header' header)")
    fmt, elements = None, []   # elements: [name, count, [(type, name) or ("list", count type, item type, name)]]
    for line in data[:end].decode("ascii", "replace").splitlines()[1:]:
        w = line.split()
        if not w or w[0] in ("comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append([w[1], int(w[2]), []])
        elif w[0] == "property":
            if not elements:
                raise ValueError(f"{path}: property before any element")
            if w[1] == "list":
                elements[-1][2].append(("list", w[2], w[3], w[4]))
            else:
                elements[-1][2].append((w[1], w[2]))
        else:
            raise ValueError(f"{path}: unknown header line {line!r}")
    if fmt == "binary_big_endian":
        raise ValueError(f"{path}: big-endian PLY files are not supported")
    if fmt not in ("binary_little_endian", "ascii"):
        raise ValueError(f"{path}: unknown PLY format {fmt!r}")
    for e in elements:
        for p in e[2]:
            if p[0] != "list" and p[0] not in _PLY_TYPES or p[0] == "list" and (p[1] not in _PLY_TYPES or p[2] not in _PLY_TYPES):
                raise ValueError(f"{path}: unknown property type in {p}")
    body = nl + 1
    vertex = None
    if fmt == "ascii":
        lines = data[body:].decode("ascii", "replace").split("\n")
        lines = [ln for ln in lines if ln.strip()]
        at = 0
        for name, count, props in elements:
            if name == "vertex":
                if any(p[0] == "list" for p in props):
                    raise ValueError(f"{path}: list properties inside the vertex element are not supported")
                if at + count > len(lines):
                    raise ValueError(f"{path}: truncated body: {len(lines) - at} of {count} vertex lines")
                try:
                    tab = np.array([ln.split() for ln in lines[at:at + count]], dtype=np.float64).reshape(count, -1)
                except ValueError:
                    raise ValueError(f"{path}: a vertex line does not hold numbers, or the lines differ in length") from None
                if tab.shape[1] != len(props) and count:
                    raise ValueError(f"{path}: vertex lines hold {tab.shape[1]} values, the header declares {len(props)}")
                vertex = {p[1]: tab[:, k].astype(_PLY_TYPES[p[0]]) for k, p in enumerate(props)}
                break
            at += count   # one line per entry of any other element, lists included
        if vertex is None and any(e[0] == "vertex" for e in elements):
            raise ValueError(f"{path}: truncated body")
    else:
        at = body
        for name, count, props in elements:
            if name == "vertex":
                if any(p[0] == "list" for p in props):
                    raise ValueError(f"{path}: list properties inside the vertex element are not supported")
                dt = np.dtype([(p[1], "<" + _PLY_TYPES[p[0]]) for p in props])
                if at + count * dt.itemsize > len(data):
                    raise ValueError(f"{path}: truncated body: {len(data) - at} bytes for {count} vertices of {dt.itemsize} bytes")
                rec = np.frombuffer(data, dt, count, at)
                vertex = {p[1]: rec[p[1]] for p in props}
                break
            if any(p[0] == "list" for p in props):   # entries of varying size: walk them
                for _ in range(count):
                    for p in props:
                        if p[0] == "list":
                            cdt, idt = np.dtype("<" + _PLY_TYPES[p[1]]), np.dtype("<" + _PLY_TYPES[p[2]])
                            if at + cdt.itemsize > len(data):
                                raise ValueError(f"{path}: truncated body in element {name}")
                            at += cdt.itemsize + int(np.frombuffer(data, cdt, 1, at)[0]) * idt.itemsize
                        else:
                            at += np.dtype(_PLY_TYPES[p[0]]).itemsize
            else:
                at += count * sum(np.dtype(_PLY_TYPES[p[0]]).itemsize for p in props)
            if at > len(data):
                raise ValueError(f"{path}: truncated body in element {name}")
    if vertex is None:
        raise ValueError(f"{path}: no vertex element")
    if not all(k in vertex for k in "xyz"):
        raise ValueError(f"{path}: the vertex element has no x y z")
    out = {"xyz": np.stack([np.asarray(vertex[k], np.float32) for k in "xyz"], 1)}
    if all(k in vertex for k in ("nx", "ny", "nz")):
        out["normals"] = np.stack([np.asarray(vertex[k], np.float32) for k in ("nx", "ny", "nz")], 1)
    if all(k in vertex for k in ("red", "green", "blue")):
        out["colors"] = np.stack([np.asarray(vertex[k], np.uint8) for k in ("red", "green", "blue")], 1)
    return out


def _xyz(a):
    a = np.ascontiguousarray(a, np.float32)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"need an [n, 3] array of points, got {a.shape}")
    return a


class Cloud:
    """A target cloud in the HBM of one MI355X (mpmvs_cloud_create); a context manager around the handle."""

    def __init__(self, xyz, device=0):
        _, self._f = engine.load()
        a = _xyz(xyz)
        self.n = len(a)
        self._h = None
        self._aligners = weakref.WeakSet()   # Aligner handles borrow this one: close() closes them first
        ok = np.isfinite(a).all(1)
        fin = a if ok.all() else a[ok]
        self.bbox = (fin.min(0), fin.max(0)) if len(fin) else None   # finite bounding box, fp32 (what the handle keeps)
        h = C.c_void_p(None)
        rc = self._f["cloud_create"](int(device), self.n, a.ctypes.data, C.byref(h))
        if rc != 0:
            self._raise("cloud_create", rc)
        self._h = h

    def _raise(self, what, rc):
        msg = self._f["last_error"](None)
        text = f"mpmvs_{what} failed ({rc}): " + (msg.decode() if msg else "")
        raise (ValueError if rc in (-2, -3) else RuntimeError)(text)

    def close(self):
        if self._h:
            for al in list(self._aligners):
                al.close()
            self._f["cloud_destroy"](self._h)
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

    def frame(self, radius):
        """the frame of an align pass at `radius` (float64 [4]: o, u), in the arithmetic of include/mpmvs.h, on the host;
        all zero for a cloud without a finite point"""
        if self.bbox is None:
            return np.zeros(4)
        mn, mx = self.bbox[0].astype(np.float64), self.bbox[1].astype(np.float64)
        h = 0.5 * float((mx - mn).max()) + 2.0 * float(np.float32(radius))
        m, e = math.frexp(h)
        return np.array([*(0.5 * (mn + mx)), h if m == 0.5 else math.ldexp(1.0, e)])

    def nearest(self, q, radius, want_idx=True):
        """(d2 float32 [n_q], idx int32 [n_q]) of mpmvs_cloud_nearest: the squared distance to, and the index of, the nearest
        target within `radius` (inf / -1 where there is none); idx is None with want_idx=False"""
        a = _xyz(q)
        d2 = np.empty(len(a), np.float32)
        idx = np.empty(len(a), np.int32) if want_idx else None
        rc = self._f["cloud_nearest"](self._h, float(radius), len(a), a.ctypes.data, d2.ctypes.data, idx.ctypes.data if want_idx else None)
        if rc != 0:
            self._raise("cloud_nearest", rc)
        return d2, idx

    def stats(self):
        """grid of the last call: {"finite", "cells", "fullest", "slots"}"""
        s = (C.c_longlong * 4)()
        self._f["cloud_stats"](self._h, s)
        return dict(zip(("finite", "cells", "fullest", "slots"), (int(v) for v in s)))

    def kernel_ms(self):
        """(query ms, build ms) of the last call, device time; build ms is 0 when the grid was reused"""
        b = C.c_float(0.0)
        q = self._f["cloud_kernel_ms"](self._h, C.byref(b))
        return float(q), float(b.value)

    def knn(self, q, radius, k, want_idx=True, want_within=False):
        """mpmvs_cloud_knn: per query the k nearest targets within `radius` -> (d2 float32 [n_q, k] ascending, idx int32 [n_q, k]);
        rows with fewer than k candidates end in inf / -1.  idx is None with want_idx=False; with want_within=True a third
        entry, int32 [n_q]: the number of all targets within the radius, not capped by k"""
        return self._knn(_xyz(q), radius, k, want_idx, want_within)

    def knn_self(self, radius, k, want_idx=True, want_within=False):
        """knn() of the cloud's own points among themselves: point i is not its own neighbour (the exclusion is by index: an
        exact duplicate of it is a neighbour at d2 = 0)"""
        return self._knn(None, radius, k, want_idx, want_within)

    def _knn(self, a, radius, k, want_idx, want_within):
        nq, k = (self.n if a is None else len(a)), int(k)
        cols = k if 1 <= k <= 32 else 0   # a refused k writes nothing
        d2 = np.empty((nq, cols), np.float32)
        idx = np.empty((nq, cols), np.int32) if want_idx else None
        within = np.empty(nq, np.int32) if want_within else None
        rc = self._f["cloud_knn"](self._h, float(radius), k, nq, a.ctypes.data if a is not None else None, d2.ctypes.data,
                                  idx.ctypes.data if want_idx else None, within.ctypes.data if want_within else None)
        if rc != 0:
            self._raise("cloud_knn", rc)
        return (d2, idx, within) if want_within else (d2, idx)

    def knn_ms(self):
        """(query ms, build ms) of the last knn / knn_self call, device time; build ms is 0 when the grid was reused"""
        b = C.c_float(0.0)
        q = self._f["cloud_knn_ms"](self._h, C.byref(b))
        return float(q), float(b.value)

    def normals(self, radius, k=16, viewpoint=None, reference=None, want_curvature=True, want_within=False):
        """mpmvs_cloud_normals: per point the normal of the plane fitted to its k nearest neighbours within `radius` (the point
        itself is part of the fit) -> (normals float32 [n, 3] of unit length, curvature float32 [n] or None); with want_within=True
        a third entry, int32 [n]: the neighbours within the radius, not capped by k.  The curvature is the surface variation, the
        smallest eigenvalue of the neighbourhood's scatter matrix over the sum of all three: 0 on a plane, at most 1/3.  A point
        with fewer than two neighbours, with all of them on itself or on one exact line, or with a non-finite coordinate has the
        normal 0 0 0 and the curvature inf.
        The sign: with `viewpoint` (3 numbers) every normal looks at that point; with `reference` (float32 [n, 3], e.g. the
        PatchMatch normals of a fused cloud) it is the one with a positive dot product with the point's reference normal;
        with neither, the component of the largest magnitude is positive.  The arithmetic is that of include/mpmvs.h, bit for bit."""
        if viewpoint is not None and reference is not None:
            raise ValueError("viewpoint and reference are mutually exclusive")
        orient, view, ref = 0, None, None
        if viewpoint is not None:
            view = np.ascontiguousarray(viewpoint, np.float64)
            if view.shape != (3,):
                raise ValueError(f"need a viewpoint of 3 numbers, got {view.shape}")
            orient = 1
        if reference is not None:
            ref = np.ascontiguousarray(reference, np.float32)
            if ref.shape != (self.n, 3):
                raise ValueError(f"need {(self.n, 3)} reference normals, got {ref.shape}")
            orient = 2
        nrm = np.empty((self.n, 3), np.float32)
        curv = np.empty(self.n, np.float32) if want_curvature else None
        within = np.empty(self.n, np.int32) if want_within else None
        rc = self._f["cloud_normals"](self._h, float(radius), int(k), orient, view.ctypes.data_as(_PD) if view is not None else None,
                                      ref.ctypes.data if ref is not None else None, nrm.ctypes.data, curv.ctypes.data if want_curvature else None,
                                      within.ctypes.data if want_within else None)
        if rc != 0:
            self._raise("cloud_normals", rc)
        return (nrm, curv, within) if want_within else (nrm, curv)

    def normals_ms(self):
        """(query ms, build ms) of the last normals call, device time; build ms is 0 when the grid was reused"""
        b = C.c_float(0.0)
        q = self._f["cloud_normals_ms"](self._h, C.byref(b))
        return float(q), float(b.value)

    def components(self, radius, want_size=True):
        """mpmvs_cloud_components: the connected components of the graph "two points are neighbours iff they are within `radius`"
        (inclusive, the candidate rule of nearest()) -> (label int32 [n], size int32 [n] or None, counts int64 [4]).  label[i] is the
        smallest index among the points of i's component (-1: a non-finite coordinate), size[i] the number of its points (0 likewise);
        counts = (points taking part, components, size of the largest component, its label; ties go to the smallest label).  The
        labels are a pure function of the point set, bit for bit those of include/mpmvs.h."""
        label = np.empty(self.n, np.int32)
        size = np.empty(self.n, np.int32) if want_size else None
        counts = (C.c_longlong * 4)()
        rc = self._f["cloud_components"](self._h, float(radius), label.ctypes.data, size.ctypes.data if want_size else None, counts)
        if rc != 0:
            self._raise("cloud_components", rc)
        return label, size, np.array(list(counts), np.int64)

    def components_ms(self, passes=False):
        """(device ms, build ms) of the last components call; build ms is 0 when the grid was reused.  With passes=True a third
        entry: {"hook", "flatten", "size"}, the device ms per pass (hook: initialisation, binning and the union-find pass)"""
        b = C.c_float(0.0)
        q = self._f["cloud_components_ms"](self._h, C.byref(b))
        if not passes:
            return float(q), float(b.value)
        ms = (C.c_float * 3)()
        self._f["cloud_components_pass_ms"](self._h, ms)
        return float(q), float(b.value), dict(zip(("hook", "flatten", "size"), (float(v) for v in ms)))

    def render_depth(self, cams, splat=1, occl_rel=0.02, want_idx=False):
        """mpmvs_cloud_render_depth: the cloud rendered into every camera of `cams` (_abi.Camera; width and height give the map's
        size) -> a list of float32 [H, W] depth maps along the camera's z axis, 0 = no depth; with want_idx=True
        (depths, idxs), idxs a list of int32 [H, W] maps of the point each pixel shows (-1 = none).

        Per pixel the nearest point that lands in it (pixel centres at integers) stays unless a point within `splat` pixels
        (Chebyshev) is nearer by more than the factor 1 + occl_rel: the back of the scene does not shine through the gaps
        between front points.  splat=0 is the plain z-buffer.  The slope rule: a slanted surface hides itself once occl_rel is
        below splat x the relative change of depth per pixel; raise occl_rel with splat on steep or close scenes.  The defaults
        are starting values from the synthetic scene, not tuned on a real scan."""
        cams = list(cams)
        n = len(cams)
        arr = (_abi.Camera * max(n, 1))(*cams)
        depths = [np.empty((max(int(c.height), 0), max(int(c.width), 0)), np.float32) for c in cams]
        idxs = [np.empty(d.shape, np.int32) for d in depths] if want_idx else None
        dp = (C.c_void_p * max(n, 1))(*[d.ctypes.data for d in depths])
        ip = (C.c_void_p * max(n, 1))(*[i.ctypes.data for i in idxs]) if want_idx else None
        rc = self._f["cloud_render_depth"](self._h, n, arr, int(splat), float(occl_rel), dp, ip)
        if rc != 0:
            self._raise("cloud_render_depth", rc)
        return (depths, idxs) if want_idx else depths

    def render_ms(self):
        """device ms of the last render_depth call's kernels: (total, {"zmin", "index", "resolve"})"""
        ms = (C.c_float * 3)()
        self._f["cloud_render_pass_ms"](self._h, ms)
        return float(self._f["cloud_render_ms"](self._h)), {"zmin": float(ms[0]), "index": float(ms[1]), "resolve": float(ms[2])}


class Observer:
    """The space the scanners of a scan observed (mpmvs_observer_create; csrc/pm_observe.hpp): per scanner
    position a range cube map of six face_size x face_size faces in HBM, made on the device from the points of `scan_cloud` (a
    Cloud; read during the constructor only, so the Cloud may be closed afterwards, and its search grids are not touched).

    scanners: float32 [m, 3], 1 <= m <= 64, in the scan's frame.  owner (int32 [n], optional): the scanner that measured each scan
    point, -1 for none; without it every point counts for every scanner, which is right only when the scanners saw the same
    surfaces.  window: a pixel's range is the smallest of the (2 window + 1)^2 pixels around it on its face, so that a query
    just beside a silhouette is not called free against the background.

    The defaults (face_size 1024, window 1, and rel 0.02 / abs_margin 0 of classify) are starting values, not tuned on a real
    scan.  This is observed-space masking in the project's own formulation, not verified against ETH3D's program."""

    def __init__(self, scan_cloud, scanners, owner=None, face_size=1024, window=1):
        _, self._f = engine.load()
        s = _xyz(scanners)
        self.n_scanners, self.face_size, self.window = len(s), int(face_size), int(window)
        self._h = None
        own = None
        if owner is not None:
            own = np.ascontiguousarray(owner, np.int32)
            if own.shape != (scan_cloud.n,):
                raise ValueError(f"owner needs one entry per scan point ({scan_cloud.n}), got shape {own.shape}")
        h = C.c_void_p(None)
        rc = self._f["observer_create"](scan_cloud._h, self.n_scanners, s.ctypes.data, own.ctypes.data if own is not None else None, self.face_size,
                                        self.window, C.byref(h))
        if rc != 0:
            self._raise("observer_create", rc)
        self._h = h

    _raise = Cloud._raise

    def close(self):
        if self._h:
            self._f["observer_destroy"](self._h)
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

    def classify(self, xyz, rel=0.02, abs_margin=0.0, want_covered=True):
        """mpmvs_observer_classify -> (free int32 [n], covered int32 [n] or None): per point the number of scanners that saw
        through it (its range plus abs_margin lies below the map's range times 1 - rel: observed free space), and the number
        whose map holds any range in its direction.  free == 0 with covered > 0: at or behind a scanned surface; covered == 0:
        no scanner looked there."""
        a = _xyz(xyz)
        free = np.empty(len(a), np.int32)
        cov = np.empty(len(a), np.int32) if want_covered else None
        rc = self._f["observer_classify"](self._h, len(a), a.ctypes.data, float(rel), float(abs_margin), free.ctypes.data,
                                          cov.ctypes.data if want_covered else None)
        if rc != 0:
            self._raise("observer_classify", rc)
        return free, cov

    def near_map(self, j):
        """float32 [6, R, R]: the windowed nearest range of scanner j per face (+x -x +y -y +z -z) and pixel, inf = nothing"""
        out = np.empty((6, self.face_size, self.face_size), np.float32)
        rc = self._f["observer_maps"](self._h, int(j), out.ctypes.data)
        if rc != 0:
            self._raise("observer_maps", rc)
        return out

    def stats(self):
        """{"covered_pixels": pixels with a finite range, "pixels": all pixels of all scanners}"""
        s = (C.c_longlong * 2)()
        self._f["observer_stats"](self._h, s)
        return {"covered_pixels": int(s[0]), "pixels": int(s[1])}

    def ms(self):
        """device ms: (the last classify call, {"zmin", "near"} of the constructor's two passes)"""
        b = (C.c_float * 2)()
        q = self._f["observer_ms"](self._h, b)
        return float(q), {"zmin": float(b[0]), "near": float(b[1])}


def read_scan_alignment(path):
    """The MeshLab project file ETH3D ships with its scans (scan_alignment.mlp) -> [(filename, T float64 [4, 4])]: every MLMesh
    element's `filename` attribute and the 16 numbers of its MLMatrix44 child, row-major.  T takes the scan into the common
    frame, so T[:3, 3] is the scanner's position there.  Restated from the format's description; no real ETH3D file has been
    read with it here.  A file that does not parse, or an MLMesh without a name or 16 numbers, raises ValueError."""
    import xml.etree.ElementTree as ET
    try:
        root = ET.parse(path).getroot()
    except ET.ParseError as e:
        raise ValueError(f"{path}: not an XML file: {e}") from None
    out = []
    for mesh in root.iter("MLMesh"):
        name, mat = mesh.get("filename"), mesh.find("MLMatrix44")
        if not name or mat is None:
            raise ValueError(f"{path}: an MLMesh element without a filename or an MLMatrix44")
        try:
            T = np.array((mat.text or "").split(), np.float64)
        except ValueError:
            raise ValueError(f"{path}: the matrix of {name} does not hold numbers") from None
        if T.size != 16 or not np.isfinite(T).all():
            raise ValueError(f"{path}: the matrix of {name} needs 16 finite numbers, got {T.size}")
        out.append((name, T.reshape(4, 4)))
    if not out:
        raise ValueError(f"{path}: no MLMesh element")
    return out


def _m12(M):
    """a 3 x 4 or 4 x 4 (last row 0 0 0 1) matrix -> 12 contiguous doubles, row-major 3 x 4"""
    a = np.asarray(M, np.float64)
    if a.shape == (4, 4):
        if not np.array_equal(a[3], [0.0, 0.0, 0.0, 1.0]):
            raise ValueError("the last row of a 4 x 4 transform must be 0 0 0 1")
        a = a[:3]
    if a.shape != (3, 4):
        raise ValueError(f"need a 3 x 4 or 4 x 4 transform, got {a.shape}")
    return np.ascontiguousarray(a).reshape(12)


_PD = C.POINTER(C.c_double)
_PL = C.POINTER(C.c_longlong)


class Aligner:
    """A moving ("source") cloud next to a target Cloud in HBM (mpmvs_align_create): uploaded once, transformed and matched on
    the device per pass.  The handle borrows the target's: the Aligner keeps a reference to the Cloud, and closing the Cloud
    closes its Aligners first."""

    def __init__(self, target_cloud, source_xyz):
        _, self._f = engine.load()
        a = _xyz(source_xyz)
        self.n = len(a)
        self.target = target_cloud
        self._h = None
        h = C.c_void_p(None)
        rc = self._f["align_create"](target_cloud._h, self.n, a.ctypes.data, C.byref(h))
        if rc != 0:
            target_cloud._raise("align_create", rc)
        self._h = h
        target_cloud._aligners.add(self)

    def close(self):
        if self._h:   # the target is still open: its close() comes here first
            self._f["align_destroy"](self._h)
            self._h = None
            self.target._aligners.discard(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sums(self, radius, M):
        """one pass (mpmvs_align_sums) at the transform M (3 x 4 or 4 x 4): (sums int64 [18], frame float64 [4])"""
        m = _m12(M)
        sums, frame = np.zeros(18, np.int64), np.zeros(4, np.float64)
        rc = self._f["align_sums"](self._h, float(radius), m.ctypes.data_as(_PD), sums.ctypes.data_as(_PL), frame.ctypes.data_as(_PD))
        if rc != 0:
            self.target._raise("align_sums", rc)
        return sums, frame

    def icp(self, radius, M, with_scale=True, max_iter=30, eps=0.0):
        """mpmvs_align_icp from the transform M: (M float64 [3, 4], passes run, inliers and rmse of the last pass)"""
        m = _m12(M).copy()
        it, inl, rmse = C.c_longlong(0), C.c_longlong(0), C.c_double(0.0)
        rc = self._f["align_icp"](self._h, float(radius), 1 if with_scale else 0, int(max_iter), float(eps), m.ctypes.data_as(_PD), C.byref(it),
                                  C.byref(inl), C.byref(rmse))
        if rc != 0:
            self.target._raise("align_icp", rc)
        return m.reshape(3, 4), int(it.value), int(inl.value), float(rmse.value)

    def ms(self):
        """device ms of the last pass of either kind: binning + kernel"""
        return float(self._f["align_ms"](self._h))

    def set_normals(self, normals):
        """mpmvs_align_set_normals: one normal per target point (float32 [target.n, 3], the target's order; any sign, any
        length; 0 0 0, NaN and inf mark a target that takes no part) for the point-to-plane pass, uploaded once onto this
        handle.  None drops them."""
        a = None
        if normals is not None:
            a = np.ascontiguousarray(normals, np.float32)
            if a.shape != (self.target.n, 3):
                raise ValueError(f"need {(self.target.n, 3)} target normals, got {a.shape}")
        rc = self._f["align_set_normals"](self._h, a.ctypes.data if a is not None else None)
        if rc != 0:
            self.target._raise("align_set_normals", rc)

    def plane_sums(self, radius, M):
        """one point-to-plane pass (mpmvs_align_plane_sums) at the transform M: (sums int64 [38], frame float64 [4])"""
        m = _m12(M)
        sums, frame = np.zeros(38, np.int64), np.zeros(4, np.float64)
        rc = self._f["align_plane_sums"](self._h, float(radius), m.ctypes.data_as(_PD), sums.ctypes.data_as(_PL), frame.ctypes.data_as(_PD))
        if rc != 0:
            self.target._raise("align_plane_sums", rc)
        return sums, frame

    def plane_icp(self, radius, M, with_scale=True, max_iter=30, eps=0.0):
        """mpmvs_align_plane_icp from the transform M: (M float64 [3, 4], passes run, inliers, rmse_plane and rmse_point of the
        last pass)"""
        m = _m12(M).copy()
        it, inl, rp, rq = C.c_longlong(0), C.c_longlong(0), C.c_double(0.0), C.c_double(0.0)
        rc = self._f["align_plane_icp"](self._h, float(radius), 1 if with_scale else 0, int(max_iter), float(eps), m.ctypes.data_as(_PD), C.byref(it),
                                        C.byref(inl), C.byref(rp), C.byref(rq))
        if rc != 0:
            self.target._raise("align_plane_icp", rc)
        return m.reshape(3, 4), int(it.value), int(inl.value), float(rp.value), float(rq.value)


def solve(sums, frame, M, with_scale=True):
    """mpmvs_align_solve (host code, no GPU): (status, M_out float64 [3, 4], rmse).  status 1: fewer than 3 pairs, no source
    variance or no covariance; M_out is M then."""
    _, f = engine.load()
    s = np.ascontiguousarray(sums, np.int64)
    fr = np.ascontiguousarray(frame, np.float64)
    if s.shape != (18,) or fr.shape != (4,):
        raise ValueError("need 18 sums and a frame of 4")
    m, out, rmse = _m12(M), np.zeros(12, np.float64), C.c_double(0.0)
    rc = f["align_solve"](s.ctypes.data_as(_PL), fr.ctypes.data_as(_PD), 1 if with_scale else 0, m.ctypes.data_as(_PD), out.ctypes.data_as(_PD), C.byref(rmse))
    if rc < 0:
        raise ValueError(f"mpmvs_align_solve failed ({rc})")
    return rc, out.reshape(3, 4), float(rmse.value)


def update_move(D, frame):
    """the stop rule of mpmvs_align_icp in the header's arithmetic: the largest distance by which the update D (3 x 4) moves a
    corner of the box frame[:3] +- frame[3]"""
    D, fr = np.asarray(D, np.float64).reshape(3, 4), np.asarray(frame, np.float64)
    worst = 0.0
    for c in range(8):
        x = [fr[k] + fr[3] if (c >> k) & 1 else fr[k] - fr[3] for k in range(3)]
        d = [(((D[k, 0] * x[0] + D[k, 1] * x[1]) + D[k, 2] * x[2]) + D[k, 3]) - x[k] for k in range(3)]
        worst = max(worst, float(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])))
    return worst


IDENTITY34 = np.eye(4)[:3]


def icp_loop(pass_fn, radius, M, with_scale=True, max_iter=30, eps=0.0):
    """the loop mpmvs_align_icp is defined as, over the two public calls: pass_fn(radius, M) -> (sums, frame) is Aligner.sums
    (or the numpy statement in the tests).  Returns what Aligner.icp returns, bit for bit."""
    M = _m12(M).reshape(3, 4).copy()
    passes, inliers, rmse = 0, 0, 0.0
    for _ in range(int(max_iter)):
        sums, frame = pass_fn(radius, M)
        passes += 1
        inliers = int(sums[0])
        rc, M_out, rmse = solve(sums, frame, M, with_scale)
        if rc == 1:
            break
        M = M_out
        if update_move(solve(sums, frame, IDENTITY34, with_scale)[1], frame) <= eps:
            break
    return M, passes, inliers, rmse


def plane_solve(sums, frame, M, with_scale=True):
    """mpmvs_align_plane_solve (host code, no GPU): (status, M_out float64 [3, 4], rmse_plane, rmse_point).  status 1: fewer pairs
    than unknowns (7 with scale, 6 without), a direction the pairs do not observe (a pivot at or below 2^-20 of its diagonal
    entry: one plane, parallel planes, the scale about the apex of a three-plane corner) or a scale that is not positive; M_out
    is M then."""
    _, f = engine.load()
    s = np.ascontiguousarray(sums, np.int64)
    fr = np.ascontiguousarray(frame, np.float64)
    if s.shape != (38,) or fr.shape != (4,):
        raise ValueError("need 38 sums and a frame of 4")
    m, out, rp, rq = _m12(M), np.zeros(12, np.float64), C.c_double(0.0), C.c_double(0.0)
    rc = f["align_plane_solve"](s.ctypes.data_as(_PL), fr.ctypes.data_as(_PD), 1 if with_scale else 0, m.ctypes.data_as(_PD), out.ctypes.data_as(_PD),
                                C.byref(rp), C.byref(rq))
    if rc < 0:
        raise ValueError(f"mpmvs_align_plane_solve failed ({rc})")
    return rc, out.reshape(3, 4), float(rp.value), float(rq.value)


def plane_icp_loop(pass_fn, radius, M, with_scale=True, max_iter=30, eps=0.0):
    """the loop mpmvs_align_plane_icp is defined as, over the two public calls: pass_fn(radius, M) -> (sums, frame) is
    Aligner.plane_sums (or the numpy statement in the tests).  Returns what Aligner.plane_icp returns, bit for bit."""
    M = _m12(M).reshape(3, 4).copy()
    passes, inliers, rmse_plane, rmse_point = 0, 0, 0.0, 0.0
    for _ in range(int(max_iter)):
        sums, frame = pass_fn(radius, M)
        passes += 1
        inliers = int(sums[0])
        rc, M_out, rmse_plane, rmse_point = plane_solve(sums, frame, M, with_scale)
        if rc == 1:
            break
        M = M_out
        if update_move(plane_solve(sums, frame, IDENTITY34, with_scale)[1], frame) <= eps:
            break
    return M, passes, inliers, rmse_plane, rmse_point


def align(source_xyz, target_cloud, T0=None, radii=None, with_scale=True, max_iter=30, eps=None, method="point", target_normals=None,
          normal_radius=None, normal_k=16):
    """Refines the transform T0 (4 x 4, identity if None) that takes `source_xyz` into the frame of `target_cloud` (a Cloud) by
    ICP in coarse-to-fine rounds: one Aligner.icp per radius of `radii`, in descending order, each starting from
    the result of the one before.  Returns (T float64 [4, 4], report), report = a list of {"radius", "passes", "inliers", "rmse"}
    per round.  `radii` has no default: it is a property of the scene (tools/eval_ply.py derives it from its tolerances).
    eps=None means 2^-20 of the frame's unit u, the power of two that covers half the target's bounding box plus two radii: a
    round ends when an update moves no corner of that box by more than a millionth of its size.
    method="point" is point-to-point ICP; method="plane" is point-to-plane ICP (Aligner.plane_icp, section
    19), which measures each pair along the target's normal and so does not hold a source to samples that are not its own.  Its
    normals are `target_normals` (float32 [target_cloud.n, 3]) or, if None, target_cloud.normals(normal_radius, normal_k);
    normal_radius is then required.  Each report row gains "rmse_plane", and "rmse" stays the point-to-point figure."""
    if radii is None or len(radii) == 0:
        raise ValueError("align needs the radii of its rounds")
    if method not in ("point", "plane"):
        raise ValueError(f"align knows the methods 'point' and 'plane', not {method!r}")
    if method == "point" and (target_normals is not None or normal_radius is not None):
        raise ValueError("target_normals and normal_radius belong to method='plane'")
    rad = sorted((float(r) for r in radii), reverse=True)
    T = np.eye(4) if T0 is None else np.array(T0, np.float64)
    M = _m12(T).reshape(3, 4)
    report = []
    if method == "plane" and target_normals is None:
        if normal_radius is None:
            raise ValueError("method='plane' needs target_normals or a normal_radius to estimate them with")
        target_normals = target_cloud.normals(normal_radius, normal_k, want_curvature=False)[0]
    with Aligner(target_cloud, source_xyz) as al:
        if method == "plane":
            al.set_normals(target_normals)
        for r in rad:
            e = float(target_cloud.frame(r)[3]) * 2.0 ** -20 if eps is None else eps
            if method == "plane":
                M, passes, inliers, rmse_plane, rmse = al.plane_icp(r, M, with_scale, max_iter, e)
                report.append({"radius": r, "passes": passes, "inliers": inliers, "rmse": rmse, "rmse_plane": rmse_plane})
                continue
            M, passes, inliers, rmse = al.icp(r, M, with_scale, max_iter, e)
            report.append({"radius": r, "passes": passes, "inliers": inliers, "rmse": rmse})
    T = np.eye(4)
    T[:3] = M
    return T, report


def distances(query, target_cloud, tolerances, on_level=None):
    """float32 [n]: per query point the exact distance to its nearest point of `target_cloud` (a Cloud) where that is within
    max(tolerances), else inf.

    Computed as a cascade: tolerances ascending, one nearest() call per tolerance with radius = tolerance, and only the queries
    still unresolved go on to the next one.  A query whose nearest d2 <= r2 at one level is final, because any nearer point
    would also be within that radius.  The grid's cells are thus about tolerance-sized at every level, so a fine tolerance never
    scans the population of coarse cells.  on_level(tolerance, n_queries, cloud), if given, is called after every level."""
    q = _xyz(query)
    out = np.full(len(q), np.inf, np.float32)
    left = np.arange(len(q))
    for t in sorted(set(float(t) for t in tolerances)):
        if len(left) == 0:
            break
        d2, _ = target_cloud.nearest(q[left], t, want_idx=False)
        if on_level:
            on_level(t, len(left), target_cloud)
        hit = np.isfinite(d2)
        out[left[hit]] = np.sqrt(d2[hit])
        left = left[~hit]
    return out


def score(d_recon, d_gt, tolerances, dropped=(0, 0)):
    """the metric arithmetic of evaluate() on precomputed nearest distances (inf = none within the largest tolerance):
    d_recon per reconstruction point to the ground truth, d_gt per ground-truth point to the reconstruction"""
    d_recon, d_gt = np.asarray(d_recon, np.float32), np.asarray(d_gt, np.float32)
    res = {"n_reconstruction": int(d_recon.size), "n_ground_truth": int(d_gt.size),
           "dropped_reconstruction": int(dropped[0]), "dropped_ground_truth": int(dropped[1]), "tolerances": []}
    for t in tolerances:
        t32 = np.float32(t)
        na, nc = int((d_recon <= t32).sum()), int((d_gt <= t32).sum())   # inclusive
        acc = na / d_recon.size if d_recon.size else 0.0
        com = nc / d_gt.size if d_gt.size else 0.0
        res["tolerances"].append({"tolerance": float(t), "accuracy": acc, "completeness": com,
                                  "f1": 2 * acc * com / (acc + com) if acc + com > 0 else 0.0, "n_accurate": na, "n_complete": nc})
    for name, d in (("reconstruction_to_ground_truth", d_recon), ("ground_truth_to_reconstruction", d_gt)):
        r = d[np.isfinite(d)].astype(np.float64)
        res[name] = {"resolved": int(r.size), "mean": float(r.mean()) if r.size else None, "median": float(np.median(r)) if r.size else None}
    return res


def score_observed(d_recon, d_gt, free, tolerances, dropped=(0, 0)):
    """score() plus the observed-space keys of evaluate(scanners=...): `free` holds, per reconstruction point, the number of
    scanners that saw through it (Observer.classify).  Per tolerance t a point with d > t counts as "n_free_inaccurate" when
    free >= 1 (it lies in space a scanner saw to be empty: certainly wrong) and as "n_unobserved" when free == 0 (nobody measured
    there: it leaves the denominator);  accuracy_observed = n_accurate / (n_accurate + n_free_inaccurate), 0 for an empty
    denominator;  f1_observed is the harmonic mean of accuracy_observed and the unchanged completeness."""
    res = score(d_recon, d_gt, tolerances, dropped)
    d, seen = np.asarray(d_recon, np.float32), np.asarray(free) >= 1
    if seen.shape != d.shape:
        raise ValueError(f"free needs one entry per reconstruction point ({d.size}), got shape {seen.shape}")
    for row in res["tolerances"]:
        far = d > np.float32(row["tolerance"])
        nf, nu = int((far & seen).sum()), int((far & ~seen).sum())
        den = row["n_accurate"] + nf
        acc, com = (row["n_accurate"] / den if den else 0.0), row["completeness"]
        row.update({"n_free_inaccurate": nf, "n_unobserved": nu, "accuracy_observed": acc,
                    "f1_observed": 2 * acc * com / (acc + com) if acc + com > 0 else 0.0})
    return res


def drop_nonfinite(xyz):
    """(the points with finite coordinates, the number dropped)"""
    a = _xyz(xyz)
    ok = np.isfinite(a).all(1)
    return (a if ok.all() else a[ok]), int((~ok).sum())


def voxel_downsample(xyz, voxel, normals=None, colors=None, device=0, want_map=False):
    """mpmvs_cloud_voxel_downsample: one point per occupied cell of a grid of edge `voxel` -> {"xyz": float32 [m, 3], "count":
    int32 [m] members per voxel, "first": int32 [m] the smallest member index; "normals" float32 [m, 3] and "colors" uint8 [m, 3]
    when given; "voxel_of": int32 [n], the voxel of every input point (-1: a non-finite coordinate), with want_map=True}.  The
    voxels come in the order of their first member.  The arithmetic is that of include/mpmvs.h, bit for bit."""
    lib, f = engine.load()
    a = _xyz(xyz)
    n = len(a)
    nrm = col = None
    if normals is not None:
        nrm = np.ascontiguousarray(normals, np.float32)
        if nrm.shape != a.shape:
            raise ValueError(f"need {a.shape} normals, got {nrm.shape}")
    if colors is not None:
        col = np.ascontiguousarray(colors, np.uint8)
        if col.shape != a.shape:
            raise ValueError(f"need {a.shape} colours, got {col.shape}")
    vmap = np.empty(n, np.int32) if want_map else None
    p = [C.c_void_p(None) for _ in range(5)]   # xyz, normals, rgb, count, first
    m = f["cloud_voxel_downsample"](int(device), n, a.ctypes.data if n else None, nrm.ctypes.data if nrm is not None and n else None,
                                    col.ctypes.data if col is not None and n else None, float(voxel), C.byref(p[0]),
                                    C.byref(p[1]) if nrm is not None else None, C.byref(p[2]) if col is not None else None, C.byref(p[3]), C.byref(p[4]),
                                    vmap.ctypes.data if want_map and n else None)
    if m < 0:
        msg = f["last_error"](None)
        text = f"mpmvs_cloud_voxel_downsample failed ({m}): " + (msg.decode() if msg else "")
        raise (ValueError if m in (-2, -3) else RuntimeError)(text)
    lib.mpmvs_free.argtypes = [C.c_void_p]
    lib.mpmvs_free.restype = None

    def take(ptr, dtype, cols):
        shape = (m, cols) if cols else (m,)
        if not m:
            return np.empty(shape, dtype)
        out = np.frombuffer((C.c_char * (m * max(cols, 1) * np.dtype(dtype).itemsize)).from_address(ptr.value), dtype).reshape(shape).copy()
        lib.mpmvs_free(ptr)
        return out

    res = {"xyz": take(p[0], np.float32, 3)}
    if nrm is not None:
        res["normals"] = take(p[1], np.float32, 3)
    if col is not None:
        res["colors"] = take(p[2], np.uint8, 3)
    res["count"] = take(p[3], np.int32, 0)
    res["first"] = take(p[4], np.int32, 0)
    if want_map:
        res["voxel_of"] = vmap
    return res


def last_voxel_ms(passes=False):
    """device ms of the calling thread's last voxel_downsample (mpmvs_cloud_voxel_ms); with passes=True (total, {"insert",
    "first", "scan", "number", "accumulate", "finish"})"""
    _, f = engine.load()
    total = float(f["cloud_voxel_ms"]())
    if not passes:
        return total
    ms = (C.c_float * 6)()
    f["cloud_voxel_pass_ms"](ms)
    return total, dict(zip(("insert", "first", "scan", "number", "accumulate", "finish"), (float(v) for v in ms)))


def remove_outliers(xyz, radius, k=16, std_ratio=2.0, min_within=0, device=0):
    """mpmvs_cloud_outliers: the statistical and the radius outlier filter over the k nearest neighbours of every point within
    `radius` -> {"keep": bool [n], "mean_dist": float32 [n] the mean distance to the k nearest (inf: fewer than k within the
    radius, or a non-finite point), "within": int32 [n] the neighbours within the radius, "counts": int64 [3] (finite points,
    points with a finite mean distance, points kept), "stats": float64 [3] (mean, sigma, threshold of the finite mean distances)}.
    A point stays iff its mean distance is finite and at most mean + std_ratio x sigma
    of all finite ones, and it has at least min_within neighbours.  std_ratio=inf switches the statistical test off, min_within=0
    the radius rule.  The arithmetic is that of include/mpmvs.h, bit for bit."""
    _, f = engine.load()
    a = _xyz(xyz)
    n = len(a)
    keep = np.zeros(n, np.uint8)
    mean = np.full(n, np.inf, np.float32)
    within = np.zeros(n, np.int32)
    counts, stats = (C.c_longlong * 3)(), (C.c_double * 3)()
    rc = f["cloud_outliers"](int(device), n, a.ctypes.data if n else None, float(radius), int(k), float(std_ratio), int(min_within),
                             keep.ctypes.data if n else None, mean.ctypes.data if n else None, within.ctypes.data if n else None, counts, stats)
    if rc < 0:
        msg = f["last_error"](None)
        text = f"mpmvs_cloud_outliers failed ({rc}): " + (msg.decode() if msg else "")
        raise (ValueError if rc in (-2, -3) else RuntimeError)(text)
    return {"keep": keep.astype(bool), "mean_dist": mean, "within": within, "counts": np.array(list(counts), np.int64),
            "stats": np.array(list(stats), np.float64)}


def last_outliers_ms():
    """device ms of the calling thread's last remove_outliers (mpmvs_cloud_outliers_ms): the grid build and the query passes"""
    _, f = engine.load()
    return float(f["cloud_outliers_ms"]())


def cluster_keep(label, size, min_size=2, largest=None):
    """the keep rule of remove_small_clusters, a few lines of numpy on the host: keep[i] iff size[i] >= min_size and, with
    largest=K, i's component is among the K largest (by size descending, then label ascending)"""
    keep = size >= min_size
    if largest is not None:
        roots = np.flatnonzero(label == np.arange(len(label)))          # one entry per component, labels ascending
        top = roots[np.argsort(-size[roots].astype(np.int64), kind="stable")[:largest]]
        keep &= np.isin(label, top)
    return keep


def remove_small_clusters(xyz, radius, min_size=2, largest=None, device=0):
    """Euclidean cluster extraction: Cloud.components over a Cloud of the call's own -> {"keep": bool [n], "label": int32 [n],
    "size": int32 [n], "counts": int64 [4]}.  keep[i] iff the connected component of point i (neighbours: within `radius`) has at
    least min_size points; with largest=K a point stays only if its component is also among the K largest (by size descending,
    then label ascending).  A point with a non-finite coordinate is never kept.  This drops the small detached clusters that
    remove_outliers keeps, because inside such a cluster every point has close neighbours.  The components come from the GPU; the
    keep rule is a few lines of numpy on the host (cluster_keep).  A cloud without a finite point is answered on the host."""
    a = _xyz(xyz)
    if not (np.isfinite(radius) and radius > 0):
        raise ValueError("radius must be finite and positive")
    if int(min_size) != min_size or min_size < 1:
        raise ValueError("min_size must be an integer of at least 1")
    if largest is not None and (int(largest) != largest or largest < 1):
        raise ValueError("largest must be None or an integer of at least 1")
    global _clusters_ms
    _clusters_ms = 0.0
    if not np.isfinite(a).all(1).any():
        label, size, counts = np.full(len(a), -1, np.int32), np.zeros(len(a), np.int32), np.array([0, 0, 0, -1], np.int64)
    else:
        with Cloud(a, device) as c:
            label, size, counts = c.components(radius)
            _clusters_ms = sum(c.components_ms())
    return {"keep": cluster_keep(label, size, int(min_size), None if largest is None else int(largest)), "label": label, "size": size, "counts": counts}


_clusters_ms = 0.0


def last_clusters_ms():
    """device ms of the last remove_small_clusters of this process: the grid build and the three passes; 0 when it launched nothing"""
    return _clusters_ms


def estimate_normals(xyz, radius, k=16, viewpoint=None, reference=None, device=0):
    """Cloud.normals over a Cloud of the call's own -> {"normals": float32 [n, 3], "curvature": float32 [n], "within": int32 [n]}"""
    with Cloud(xyz, device) as c:
        nrm, curv, within = c.normals(radius, k, viewpoint, reference, want_within=True)
    return {"normals": nrm, "curvature": curv, "within": within}


def write_ply(path, xyz, normals=None, colors=None):
    """the reference's 27-byte records (hostlib.write_ply: x y z nx ny nz red green blue); normals or colours that are not given
    are written as zeros"""
    from . import hostlib
    a = _xyz(xyz)
    p9 = np.zeros((len(a), 9), np.float32)
    p9[:, 0:3] = a
    if normals is not None:
        p9[:, 3:6] = normals
    if colors is not None:
        p9[:, 6:9] = np.asarray(colors)[:, ::-1]   # the record's colour triple is held blue, green, red and written red, green, blue
    hostlib.write_ply(path, p9)


def evaluate(recon_xyz, gt_xyz, tolerances, device=0, timings=None, voxel=None, scanners=None, owner=None, face_size=1024, window=1, free_rel=0.02,
             free_abs=0.0):
    """Accuracy, completeness and F1 of a reconstructed cloud against a ground-truth cloud at every tolerance.

    Per tolerance t: accuracy = the share of reconstruction points whose nearest ground-truth point is within t (inclusive),
    completeness = the share of ground-truth points whose nearest reconstruction point is within t, f1 = their harmonic mean
    (0 if both are 0); also the counts, the two point totals and the mean and median of the resolved distances each way.
    Points with a non-finite coordinate are dropped and counted.

    voxel (None, or a positive edge length): both clouds are resampled on a voxel grid of that edge (voxel_downsample) after the
    non-finite points are dropped and before anything else, so that a surface does not count by how densely it was sampled
    (Tanks and Temples uses half its tolerance); the result then also holds "voxel" and the point counts before the resampling,
    "n_reconstruction_in" and "n_ground_truth_in".  None leaves the clouds as they are.

    scanners (None, or float32 [m, 3] scanner positions in the ground truth's frame): the accuracy is also given over observed
    space only (Observer).  The range cube maps are made from the ground truth after the non-finite points
    are dropped and before any voxel resampling; owner (optional, one scanner index or -1 per ground-truth point as passed in) is
    filtered with the points.  The reconstruction as scored (after the resampling) is classified with the margins free_rel and
    free_abs, and every tolerance row gains "n_free_inaccurate", "n_unobserved", "accuracy_observed" and "f1_observed"
    (score_observed), the result "observed": {"scanners", "face_size", "window", "free_rel", "free_abs", "covered_pixels",
    "pixels"}.  A reconstruction point beyond the scanned surface, or in a direction that returned nothing, then no longer counts
    as inaccurate.  face_size 1024, window 1, free_rel 0.02 and free_abs 0 are starting values, not tuned on a real scan.  An
    Observer the caller made (of a scan that these clouds were resampled from, say) may be given in place of the positions: it is
    used as it is and left open.  None changes nothing: the keys and values are those of the plain measure.

    The plain keys are the two-way nearest-neighbour measure (Tanks-and-Temples style).  ETH3D's official program additionally
    masks the space the scanner did not observe; the observed-space keys do that in our own formulation, not verified against
    ETH3D's program: the numbers are comparable between our own builds and settings, and not to the ETH3D leaderboard.
    timings (a dict, optional) receives seconds of upload + build and of query, and "observe_s" with scanners."""
    import time
    rec, drop_r = drop_nonfinite(recon_xyz)
    gt, drop_g = drop_nonfinite(gt_xyz)
    tol = [float(t) for t in tolerances]
    if not tol or not all(np.isfinite(t) and t > 0 for t in tol):
        raise ValueError("tolerances must be finite and positive")
    obs, t_obs = None, 0.0
    if isinstance(scanners, Observer):
        obs = scanners
    elif scanners is not None:
        if owner is not None:
            owner = np.asarray(owner, np.int32)
            if owner.shape != (len(_xyz(gt_xyz)),):
                raise ValueError(f"owner needs one entry per ground-truth point, got shape {owner.shape}")
            owner = owner[np.isfinite(_xyz(gt_xyz)).all(1)]
        t_o = time.perf_counter()
        with Cloud(gt, device) as c_scan:
            obs = Observer(c_scan, scanners, owner, face_size, window)
        t_obs = time.perf_counter() - t_o
    if voxel is not None:
        if not (np.isfinite(voxel) and voxel > 0):
            raise ValueError("voxel must be finite and positive")
        n_in = (len(rec), len(gt))
        rec = voxel_downsample(rec, voxel, device=device)["xyz"]
        gt = voxel_downsample(gt, voxel, device=device)["xyz"]
    t_build = [0.0]

    def on_level(t, n, cloud):
        t_build[0] += cloud.kernel_ms()[1] * 1e-3

    t0 = time.perf_counter()
    with Cloud(gt, device) as c_gt:
        t1 = time.perf_counter()
        d_rec = distances(rec, c_gt, tol, on_level)
    t2 = time.perf_counter()
    with Cloud(rec, device) as c_rec:
        t3 = time.perf_counter()
        d_gt = distances(gt, c_rec, tol, on_level)
    t4 = time.perf_counter()
    if timings is not None:
        timings["upload_build_s"] = (t1 - t0) + (t3 - t2) + t_build[0]
        timings["query_s"] = (t2 - t1) + (t4 - t3) - t_build[0]
    if obs is None:
        res = score(d_rec, d_gt, tol, (drop_r, drop_g))
    else:
        t_o = time.perf_counter()
        try:
            free, _ = obs.classify(rec, free_rel, free_abs, want_covered=False)
            res = score_observed(d_rec, d_gt, free, tol, (drop_r, drop_g))
            res["observed"] = {"scanners": obs.n_scanners, "face_size": obs.face_size, "window": obs.window, "free_rel": float(free_rel),
                               "free_abs": float(free_abs), **obs.stats()}
        finally:
            if obs is not scanners:
                obs.close()
        if timings is not None:
            timings["observe_s"] = t_obs + (time.perf_counter() - t_o)
    if voxel is not None:
        res["voxel"], res["n_reconstruction_in"], res["n_ground_truth_in"] = float(voxel), n_in[0], n_in[1]
    return res
