"""COLMAP sparse model -> MVSNet-style folder, the parts without a GPU: the C++ model reader, cams/ and pair.txt against
the reference converter's recorded outputs (tests/golden/colmap_v1), and the folder the pipeline reads."""
import importlib
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from colmap_common import FIXTURE, check_cams, expected_order, literal_score, parse_pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPARSE = os.path.join(FIXTURE, "sparse")


@pytest.fixture(scope="module")
def colmap(pm):
    return importlib.import_module("mp-mvs_amd.colmap")


def _numpy_parse_txt(d):
    """an independent parse of the text model: images by ascending id, point ids mapped to their line index"""
    lines = lambda f: [l.rstrip("\n") for l in open(os.path.join(d, f)) if not l.startswith("#")]
    pts = [l.split() for l in lines("points3D.txt") if l.strip()]
    pid = np.array([int(p[0]) for p in pts], np.int64)
    xyz = np.array([[float(v) for v in p[1:4]] for p in pts])
    index = {int(v): k for k, v in enumerate(pid)}
    raw = lines("images.txt")
    imgs = []
    for k in range(0, len(raw), 2):
        h = raw[k].split()
        ids = [int(v) for v in raw[k + 1].split()[2::3]]
        imgs.append((int(h[0]), [float(v) for v in h[1:5]], [float(v) for v in h[5:8]], int(h[8]), h[9], [index[v] if v != -1 else -1 for v in ids]))
    imgs.sort()
    off = np.cumsum([0] + [len(i[5]) for i in imgs])
    return dict(image_id=np.array([i[0] for i in imgs]), qvec=np.array([i[1] for i in imgs]), tvec=np.array([i[2] for i in imgs]),
                image_cam=np.array([i[3] for i in imgs]), names=[i[4] for i in imgs], obs_off=off,
                obs_pt=np.array(sum((i[5] for i in imgs), [])), point_id=pid, xyz=xyz)


def test_reader_txt_bin_and_numpy_agree(colmap):
    t = colmap.read_model(SPARSE, ".txt")
    b = colmap.read_model(SPARSE, ".bin")
    auto = colmap.read_model(SPARSE)   # .bin preferred
    for f in t.__dataclass_fields__:
        assert np.array_equal(np.asarray(getattr(t, f)), np.asarray(getattr(b, f))), f
        assert np.array_equal(np.asarray(getattr(b, f)), np.asarray(getattr(auto, f))), f
    ref = _numpy_parse_txt(SPARSE)
    for f, v in ref.items():
        assert np.array_equal(np.asarray(getattr(t, f)), np.asarray(v)), f
    assert t.n_images == 14 and len(t.point_id) == 700
    assert list(t.image_id) == sorted(t.image_id) and np.any(np.diff(t.image_id) > 1)
    assert (t.obs_pt == -1).any()
    assert sorted(colmap.CAMERA_MODELS[m] for m in t.cam_model) == ["PINHOLE", "SIMPLE_RADIAL"]


def _copy_model(tmp_path):
    d = tmp_path / "sparse"
    shutil.copytree(SPARSE, d)
    return d


def test_reader_errors(colmap, tmp_path):
    d = _copy_model(tmp_path)
    data = (d / "images.bin").read_bytes()
    (d / "images.bin").write_bytes(data[:len(data) // 2])
    with pytest.raises(ValueError, match="truncated"):
        colmap.read_model(d, ".bin")
    (d / "images.bin").write_bytes(data)
    cam = bytearray((d / "cameras.bin").read_bytes())
    cam[12:16] = struct.pack("<i", 11)   # model id of the first camera
    (d / "cameras.bin").write_bytes(bytes(cam))
    with pytest.raises(ValueError, match="unknown model id 11"):
        colmap.read_model(d, ".bin")
    txt = (d / "cameras.txt").read_text().replace("PINHOLE", "PINHOLE_X", 1)
    (d / "cameras.txt").write_text(txt)
    with pytest.raises(ValueError, match="unknown camera model"):
        colmap.read_model(d, ".txt")
    shutil.copy(os.path.join(SPARSE, "cameras.txt"), d / "cameras.txt")
    pts = (d / "points3D.txt").read_text().splitlines()
    first_id = next(l for l in pts if not l.startswith("#")).split()[0]
    (d / "points3D.txt").write_text("\n".join(l for l in pts if l.split()[0] != first_id) + "\n")
    with pytest.raises(ValueError, match=f"point3D {first_id}, which is not in points3D"):
        colmap.read_model(d, ".txt")
    shutil.copy(os.path.join(SPARSE, "points3D.txt"), d / "points3D.txt")
    lines = (d / "images.txt").read_text().splitlines()
    k = next(i for i, l in enumerate(lines) if not l.startswith("#"))
    lines[k + 1] = " ".join("%s %s -1" % tuple(t) for t in zip(lines[k + 1].split()[0::3], lines[k + 1].split()[1::3]))
    (d / "images.txt").write_text("\n".join(lines) + "\n")
    with pytest.raises(ValueError, match="has no observation of a 3D point"):
        colmap.read_model(d, ".txt")
    with pytest.raises(ValueError, match="cannot open"):
        colmap.read_model(tmp_path / "nowhere", ".txt")


@pytest.mark.parametrize("max_d", [192, 0])
def test_write_cams_matches_reference(colmap, tmp_path, max_d):
    model = colmap.read_model(SPARSE, ".bin")
    colmap.write_cams(model, tmp_path, max_d=max_d)
    check_cams(tmp_path / "cams", os.path.join(FIXTURE, "expected_d%d" % max_d, "cams"), model.n_images)


def test_write_pairs_roundtrip(colmap, tmp_path):
    for d in ("expected_d192", "expected_d0"):
        path = os.path.join(FIXTURE, d, "pair.txt")
        ids, scores = parse_pairs(path)
        assert ids.shape == (14, 13)
        colmap.write_pairs(tmp_path / "pair.txt", ids, scores)
        assert (tmp_path / "pair.txt").read_bytes() == open(path, "rb").read()


def test_literal_score_matches_reference(colmap):
    """the tests' own pairwise statement of the score agrees with every score the reference recorded"""
    m = colmap.read_model(SPARSE, ".txt")
    C = colmap.centers(m)
    lists = [m.obs_pt[m.obs_off[i]:m.obs_off[i + 1]] for i in range(m.n_images)]
    S = np.zeros((m.n_images, m.n_images), np.int64)
    for i in range(m.n_images):
        for j in range(i + 1, m.n_images):
            S[i, j] = S[j, i] = literal_score(lists[i], lists[j], C[i], C[j], m.xyz)
    ids, scores = parse_pairs(os.path.join(FIXTURE, "expected_d192", "pair.txt"))
    for i in range(m.n_images):
        assert np.array_equal(S[i, ids[i]], scores[i]), i
        assert np.array_equal(np.sort(S[i])[::-1][:13], scores[i]), i   # the rows are the 13 best
        assert np.array_equal(S[i, expected_order(S[i], 13)], scores[i])
    # the co-located pair shares many points and is zeroed by the 1-degree rule
    shared = np.array([[len(set(lists[i][lists[i] >= 0]) & set(lists[j][lists[j] >= 0])) for j in range(m.n_images)] for i in range(m.n_images)])
    np.fill_diagonal(shared, 0)
    i, j = np.unravel_index(np.argmax(shared), shared.shape)
    assert shared[i, j] >= 100 and S[i, j] == 0


def test_pipeline_reads_converted_folder(colmap, hostlib, tmp_path):
    m = colmap.read_model(SPARSE)
    colmap.write_cams(m, tmp_path)
    ids, scores = parse_pairs(os.path.join(FIXTURE, "expected_d192", "pair.txt"))
    colmap.write_pairs(tmp_path / "pair.txt", ids, scores)
    colmap.copy_images(m, os.path.join(FIXTURE, "images"), tmp_path / "images")
    for i, name in enumerate(m.names):
        assert (tmp_path / "images" / ("%08d.jpg" % i)).read_bytes() == open(os.path.join(FIXTURE, "images", name), "rb").read()
    cam = hostlib.read_camera(tmp_path / "cams" / "00000003_cam.txt")
    K = colmap.intrinsics(m, warn=False)[int(m.image_cam[3])]
    assert np.allclose(np.array(cam.K).reshape(3, 3), K)
    assert np.allclose(np.array(cam.R).reshape(3, 3), colmap.extrinsics(m)[3, :3, :3], atol=1e-7)
    rng = colmap.depth_ranges(m)[3]
    assert cam.depth_min == pytest.approx(rng[0], rel=1e-6) and cam.depth_max == pytest.approx(rng[3], rel=1e-6)
    lst = hostlib.sample_list(tmp_path, max_src=20)
    assert len(lst) == 14
    for i, (est, ref, src) in enumerate(lst):
        assert est and ref == i and src[0] == i
        assert src[1:] == [int(k) for k, s in zip(ids[i], scores[i]) if s > 0]


def test_other_image_formats(colmap, tmp_path):
    from PIL import Image
    m = colmap.read_model(SPARSE)
    src = tmp_path / "in"
    src.mkdir()
    a = (np.arange(12 * 8) % 251).astype(np.uint8).reshape(8, 12)
    rgb = np.stack([a, a[::-1], 255 - a], -1)
    for i, name in enumerate(m.names):
        m.names[i] = ["x%d.png" % i, "x%d.jpeg" % i, "x%d.bmp" % i][i % 3]
        if i % 3 == 0:
            Image.fromarray(a).save(src / m.names[i])
        elif i % 3 == 1:
            shutil.copy(os.path.join(FIXTURE, "images", name), src / m.names[i])
        else:
            Image.fromarray(rgb).save(src / m.names[i])
    colmap.copy_images(m, src, tmp_path / "out")
    assert (tmp_path / "out" / "00000001.jpg").read_bytes() == (src / "x1.jpeg").read_bytes()
    assert (tmp_path / "out" / "00000000.pgm").read_bytes() == b"P5\n12 8\n255\n" + a.tobytes()
    assert (tmp_path / "out" / "00000002.ppm").read_bytes() == b"P6\n12 8\n255\n" + rgb.tobytes()


def test_existing_outputs_refused(colmap, tmp_path):
    out = tmp_path / "out"
    (out / "cams").mkdir(parents=True)
    (out / "cams" / "keep.txt").write_text("x")
    with pytest.raises(FileExistsError, match="overwrite"):
        colmap.convert(FIXTURE, out)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "colmap2mvs.py"), "--dense_folder", FIXTURE, "--save_folder", str(out)],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "--overwrite" in r.stderr
    assert (out / "cams" / "keep.txt").read_text() == "x"
