"""What the TSDF sweeps of tests/test_tsdf_fuzz_gpu.py cover, asserted on the numpy statements alone (no GPU): the generators of
tests/tsdf_fuzz_common.py reach the culled and the nearly culled boxes, the chunk boundaries, every (tetrahedron, case) pair emitting
and suppressed, the special values of the mesh contract and every kind of operation in a sparse handle's life; and the block test
tsdf_box_live -- restated in numpy, and as csrc/pm_tsdf.hpp has it, compiled for the host (tests/tsdf_host_main.cpp) -- never calls a
box dead that holds a voxel the statement would project into the image; tsdf_byte of the header is the contract's byte.  These are
conditions on the generators as committed, not measurements: the counts each test prints are quoted in DESIGN.md sections 22 and 23."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import tsdf_common as tc
import tsdf_fuzz_common as fz
import tsdf_sparse_common as sc

F = np.float32
N_A, N_B, N_C = (fz.DEFAULT_CASES[s] for s in "ABC")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    """tests/tsdf_host_main.cpp: tsdf_box_live and tsdf_byte of csrc/pm_tsdf.hpp compiled for the host -> a function from the program's
    input to its output lines"""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path_factory.mktemp("tsdf_host") / "tsdf_host")
    build = subprocess.run([hipcc, "-std=c++17", "-O1", "--offload-arch=gfx950", "-ffp-contract=off", "-I", os.path.join(ROOT, "mp-mvs_amd", "csrc"),
                            "-x", "hip", os.path.join(ROOT, "tests", "tsdf_host_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def _num(x):
    return repr(float(x))      # the shortest decimal that names the float's value: strtod gives it back exactly


# ---- sweep A ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cull_census(pm):
    """per kind of box ("tile", "brick") the (case, view, box) records of sweep A: the verdict of the block test and the number of the
    box's voxels that pass steps 2 and 4"""
    out = {"tile": [], "brick": []}
    for k in range(N_A):
        c = fz.integrate_case(pm, k)
        pos = tc.positions(c.origin, c.voxel, c.dims)
        boxes = {"tile": fz.tile_boxes(c.dims), "brick": fz.brick_boxes(c.dims)}
        for cam in c.cams:
            seen = fz.in_image(cam, pos)
            for kind, b in boxes.items():
                out[kind].append((fz.box_live_many(cam, pos, b), fz.count_in_boxes(seen, b)))
    return {kind: (np.concatenate([r[0] for r in recs]), np.concatenate([r[1] for r in recs])) for kind, recs in out.items()}


@pytest.mark.parametrize("kind", ["tile", "brick"])
def test_block_test_is_sound_and_the_sweep_reaches_nearly_dead_boxes(cull_census, kind):
    verdict, inside = cull_census[kind]
    dead = verdict != "live"
    near = (verdict == "live") & (inside >= 1) & (inside <= 4)
    print(f"{kind}: {len(verdict)} (box, view) pairs, dead by the image {int((verdict == 'image').sum())}, behind {int((verdict == 'behind').sum())}, "
          f"live {int((~dead).sum())}, live with 1..4 voxels in the image {int(near.sum())}, live with none {int((~dead & (inside == 0)).sum())}, "
          f"unsound {int((dead & (inside > 0)).sum())}")
    assert not (dead & (inside > 0)).any()           # soundness: a dead box holds no voxel that passes steps 2 and 4
    assert (verdict == "image").sum() >= 200 and (verdict == "behind").sum() >= 20 and near.sum() >= 20


def test_compiled_block_test_is_sound_and_equals_the_restated_one(pm, host_program):
    """tsdf_box_live<4> on every (tile, view) and tsdf_box_live<8> on every (brick, view) of sweep A, from the header itself: never dead
    where a voxel of the box passes steps 2 and 4, and dead exactly where the numpy restatement says so (which is what entitles the
    census above to speak about the kernels' cull)"""
    text, want, inside = [], [], []
    for k in range(N_A):
        c = fz.integrate_case(pm, k)
        pos = tc.positions(c.origin, c.voxel, c.dims)
        seen = [fz.in_image(cam, pos) for cam in c.cams]
        for corners, boxes in ((4, fz.tile_boxes(c.dims)), (8, fz.brick_boxes(c.dims))):
            words = ["live"] + [_num(x) for x in c.origin] + [_num(c.voxel)] + [str(n) for n in c.dims] + [str(corners), str(len(c.cams)), str(len(boxes))]
            for cam in c.cams:
                K, R, t, W, H = tc.cam_arrays(cam)
                words += [_num(x) for x in list(R) + list(t) + [K[0], K[2], K[4], K[5]]] + [str(W), str(H), str(int(fz.cull_allowed(cam, pos)))]
            words += [str(int(x)) for x in boxes.reshape(-1)]
            text.append(" ".join(words))
            for cam, m in zip(c.cams, seen):
                want.append(fz.box_live_many(cam, pos, boxes) == "live")
                inside.append(fz.count_in_boxes(m, boxes))
    lines = host_program("\n".join(text) + "\n")
    assert len(lines) == len(want)
    got = [np.array([ch == "1" for ch in line]) for line in lines]
    assert all(g.shape == w.shape for g, w in zip(got, want))
    got, want, inside = np.concatenate(got), np.concatenate(want), np.concatenate(inside)
    print(f"{len(got)} (box, view) pairs through the compiled test: {int((~got).sum())} dead, {int((~got & (inside > 0)).sum())} of them unsound, "
          f"{int((got != want).sum())} unlike the restatement")
    assert not (~got & (inside > 0)).any()
    assert np.array_equal(got, want)


def test_compiled_colour_byte_is_the_contracts(host_program):
    rng = np.random.default_rng(3)
    val = np.concatenate([np.array([-np.inf, -1e9, -3.0, -0.6, -0.5, -0.4, 0.0, 0.49, 0.5, 127.5, 254.4, 254.5, 255.0, 300.0, 1e9, 4e9, 3e38, np.inf, np.nan], F),
                          rng.uniform(-300, 600, 500).astype(F)])
    got = host_program("byte " + str(len(val)) + " " + " ".join(_num(v) for v in val) + "\n")
    assert len(got) == 1 and [int(x) for x in got[0].split()] == tc.color_byte(val).tolist()


def test_box_live_statement_on_boxes_worked_by_hand(pm):
    """the restated block test itself, on a camera at the origin looking along +z (f = 32, 32 x 24, principal point 15.5, 11.5) and
    the lattice P = (-1.5 + i/4, -0.75 + j/4, -0.5 + k/4): fu = 32 Px / Pz + 16"""
    cam = pm.make_camera(np.array([[32.0, 0, 15.5], [0, 32.0, 11.5], [0, 0, 1]]), np.eye(3), np.zeros(3), 24, 32, 0.5, 20.0)
    pos = tc.positions((-1.5, -0.75, -0.5), 0.25, (13, 7, 13))
    assert fz.box_live_statement(cam, pos, (0, 12, 0, 6, 0, 2)) == "behind"        # z <= 0 throughout (k = 2 is z = 0)
    assert fz.box_live_statement(cam, pos, (0, 12, 0, 6, 2, 3)) == "live"          # z0 = 0: not decided
    assert fz.box_live_statement(cam, pos, (0, 1, 0, 6, 6, 6)) == "image"          # z = 1, Px <= -1.25: fu <= -24
    assert fz.box_live_statement(cam, pos, (0, 4, 0, 6, 6, 6)) == "live"           # Px = -0.5: fu = 0, the border is inside
    assert fz.box_live_statement(cam, pos, (8, 12, 3, 3, 6, 6)) == "image"         # Px >= 0.5: fu >= 32 = W, the border is outside
    assert fz.box_live_statement(cam, pos, (7, 12, 3, 3, 6, 6)) == "live"
    far = pm.make_camera(np.array([[32.0, 0, 15.5], [0, 32.0, 11.5], [0, 0, 1]]), np.eye(3), np.array([0.0, 0.0, 2.0 ** 41]), 24, 32, 0.5, 20.0)
    assert not fz.cull_allowed(far, pos) and fz.box_live_statement(far, pos, (0, 1, 0, 6, 6, 6)) == "live"
    for a, b in zip(fz.box_live_many(cam, pos, fz.tile_boxes((13, 7, 13))), fz.tile_boxes((13, 7, 13))):
        assert a == fz.box_live_statement(cam, pos, tuple(b))


def test_sweep_a_covers_chunks_colours_splits_and_branches(pm):
    cases = [fz.integrate_case(pm, k) for k in range(N_A)]
    views = [len(c.cams) for c in cases]
    assert set(fz.FORCED_VIEWS) <= set(views) and min(views) == 1 and max(views) == 19, sorted(set(views))
    assert {c.color for c in cases} == {"none", "bgr", "grey"} and {len(c.calls) for c in cases} == {1, 2, 3}
    assert all(c.calls[0].start == 0 and c.calls[-1].stop == len(c.cams) and all(a.stop == b.start for a, b in zip(c.calls, c.calls[1:])) for c in cases)
    modes = {m: sum(1 for c in cases if c.brick_mode == m) for m in ("allocate", "mask", "all")}
    partial = sum(1 for c in cases if c.bricks.any() and not c.bricks.all())
    seen = {"weight >= 4": 0, "clamped (s > trunc)": 0, "-trunc <= s < 0": 0, "painted": 0, "an existing brick that no view observes": 0}
    bad_under = {name: 0 for name in fz.BAD_DEPTHS}
    for c in cases:
        want = fz.integrate_want(c)
        seen["weight >= 4"] += bool(want[1].max() >= 4)
        seen["painted"] += bool(want[2] is not None and want[2][..., 3].any())
        seen["an existing brick that no view observes"] += bool((c.bricks & ~_touched_bricks(c, want[1])).any())
        pos = tc.positions(c.origin, c.voxel, c.dims)
        Pz, Py, Px = np.meshgrid(pos[2], pos[1], pos[0], indexing="ij")
        for cam, depth, names in zip(c.cams, c.depths, c.bad):
            ok = fz.in_image(cam, pos)
            z, fu, fv = tc.project(cam, Px, Py, Pz)
            with np.errstate(all="ignore"):
                d = depth[np.where(ok, np.floor(fv), 0).astype(np.int64), np.where(ok, np.floor(fu), 0).astype(np.int64)]
                good = ok & np.isfinite(d) & (d > 0)
                s = d - z
                seen["clamped (s > trunc)"] += bool((good & (s > F(c.trunc))).any())
                seen["-trunc <= s < 0"] += bool((good & (s < 0) & ~(s < -F(c.trunc))).any())
            under = d[ok]
            found = {"zero": (under == 0).any(), "negative": (under == -1).any(), "nan": np.isnan(under).any(), "+inf": (under == np.inf).any(),
                     "denormal": ((under > 0) & (under < 1e-38)).any()}
            for name in names:
                bad_under[name] += bool(found[name])
    print("views per case", sorted(views), "brick modes", modes, "cases with some but not all bricks", partial)
    print("cases (per view for the two branches) that reach:", seen, "views with a planted value under a projected voxel:", bad_under)
    assert min(modes.values()) >= 10 and partial >= 15
    assert all(v >= 10 for v in seen.values()) and all(v >= 10 for v in bad_under.values())


def _touched_bricks(c, weight):
    """bool brick grid: some voxel of the brick was observed"""
    bx, by, bz = sc.brick_grid(c.dims)
    nx, ny, nz = c.dims
    big = np.zeros((8 * bz, 8 * by, 8 * bx), bool)
    big[:nz, :ny, :nx] = weight > 0
    return big.reshape(bz, 8, by, 8, bx, 8).any(axis=(1, 3, 5))


# ---- sweep B ------------------------------------------------------------------------------------------------------------------------
def test_sweep_b_reaches_every_tetrahedron_case_and_every_special_value():
    every = {(t, m) for t in range(6) for m in range(1, 15)}
    emitting, by_invalid, by_brick = set(), set(), set()
    special_on_vertex = {name: 0 for name in fz.SPECIAL_SUMS}
    seen = {"NaN positions": 0, "colour value above 255": 0, "NaN colour value": 0, "a denormal negative f decides inside": 0,
            "far ends of a brick's edges in all eight bricks": 0, "a brick's cells use owners in all seven bricks that can own": 0,
            "an emitting cell with a corner in a brick that does not exist": 0, "more than 256 scan tiles": 0, "more than 128 bricks": 0,
            "sparse mesh smaller than the dense one": 0, "empty mesh": 0}
    modes = {}
    for k in range(N_B):
        c = fz.mesh_case(k)
        nx, ny, nz = c.dims
        dense, sparse = fz.mesh_want(c)
        modes[c.brick_mode] = modes.get(c.brick_mode, 0) + 1
        valid, f, inside = fz.corner_values(c.total, c.weight, c.min_weight)
        exists = sc.voxel_exists(c.dims, c.bricks)
        tiny_inside = inside & (np.abs(f) < F(1e-38))
        decided = False
        for t, ((allv, m), (alle, _), (tiny, _)) in enumerate(zip(fz.tet_cases(valid, inside), fz.tet_cases(exists, inside), fz.tet_cases(~tiny_inside, inside))):
            mixed = (m > 0) & (m < 15)
            emitting |= {(t, int(x)) for x in np.unique(m[allv & mixed])}
            by_invalid |= {(t, int(x)) for x in np.unique(m[~allv & mixed])}
            by_brick |= {(t, int(x)) for x in np.unique(m[allv & mixed & ~alle])}
            decided |= bool((allv & mixed & ~tiny).any())
        seen["a denormal negative f decides inside"] += decided
        # the vertices: their two ends
        owner, slot = dense["keys"] // 7, dense["keys"] % 7
        off = np.array(tc.SLOTS, np.int64)[slot]
        ia = np.stack([owner % nx, (owner // nx) % ny, owner // (nx * ny)], 1)
        ib = ia + off
        ends = np.concatenate([c.total[ia[:, 2], ia[:, 1], ia[:, 0]], c.total[ib[:, 2], ib[:, 1], ib[:, 0]]])
        for name, value in fz.SPECIAL_SUMS.items():
            hit = np.isnan(ends) if name == "nan" else (ends == F(value)) & (np.signbit(ends) == np.signbit(F(value)))
            special_on_vertex[name] += bool(hit.any())
        seen["NaN positions"] += bool(np.isnan(dense["xyz"]).any())
        if dense["val"] is not None and len(dense["val"]):
            seen["colour value above 255"] += bool((dense["val"] > 255.5).any())
            seen["NaN colour value"] += bool(np.isnan(dense["val"]).any())
            assert np.array_equal(dense["rgb"][:, ::-1], tc.color_byte(dense["val"]))
        # bricks: where the far ends and the owners of a brick's edges lie
        if len(owner):
            code = ((ib[:, 0] >> 3) - (ia[:, 0] >> 3)) | (((ib[:, 1] >> 3) - (ia[:, 1] >> 3)) << 1) | (((ib[:, 2] >> 3) - (ia[:, 2] >> 3)) << 2)
            brick = ((ia[:, 2] >> 3) * 64 + (ia[:, 1] >> 3)) * 64 + (ia[:, 0] >> 3)
            seen["far ends of a brick's edges in all eight bricks"] += any(len(set(code[brick == b].tolist())) == 8 for b in np.unique(brick))
        st = tc.mesh_statement(*sc.mask_dense(c.dims, c.bricks, c.total, c.weight, c.color4), c.dims, c.origin, c.voxel, c.min_weight, details=True)
        if len(st["tri"]):
            keys = st["keys"][st["tri"]]                    # [m, 3]: the owners a cell's triangles use
            cell = np.repeat(st["tri_cell"][:, None], 3, 1)
            own = keys // 7
            bo = lambda v: np.stack([(v % nx) >> 3, ((v // nx) % ny) >> 3, (v // (nx * ny)) >> 3], -1)
            rel = bo(own) - bo(cell)
            code = (rel[..., 0] | (rel[..., 1] << 1) | (rel[..., 2] << 2)).reshape(-1)
            b3 = bo(cell).reshape(-1, 3)
            brick = (b3[:, 2] * 64 + b3[:, 1]) * 64 + b3[:, 0]
            seen["a brick's cells use owners in all seven bricks that can own"] += any(len(set(code[brick == b].tolist())) == 7 for b in np.unique(brick))
            assert 7 not in set(code.tolist())              # corner 111 is never the lower end of an edge
            ci, cj, ck = st["tri_cell"] % nx, (st["tri_cell"] // nx) % ny, st["tri_cell"] // (nx * ny)
            missing = np.zeros(len(ci), bool)
            for dz in (0, 1):
                for dy in (0, 1):
                    for dx in (0, 1):
                        missing |= ~exists[ck + dz, cj + dy, ci + dx]
            seen["an emitting cell with a corner in a brick that does not exist"] += bool(missing.any())
        assert len(st["tri"]) == len(sparse["tri"]) and len(sparse["tri"]) <= len(dense["tri"])
        seen["sparse mesh smaller than the dense one"] += len(sparse["tri"]) < len(dense["tri"])
        seen["empty mesh"] += len(sparse["tri"]) == 0
        seen["more than 256 scan tiles"] += nx * ny * nz > 65536
        seen["more than 128 bricks"] += int(c.bricks.sum()) > 128 and int(c.bricks.sum()) * 512 > 65536
    print(f"(tetrahedron, case) pairs of 84: emitting {len(emitting)}, suppressed by an invalid corner {len(by_invalid)}, by a missing brick {len(by_brick)}")
    print("cases with a vertex on an edge that ends at a planted sum:", special_on_vertex)
    print("cases that reach:", seen, "brick modes:", modes)
    assert emitting == every and by_invalid == every and by_brick == every
    assert all(v >= 5 for v in special_on_vertex.values()), special_on_vertex
    assert all(v >= 2 for v in seen.values()), seen
    assert set(modes) == {"all", "none", "mask"}


def test_color_byte_is_the_contracts_and_leaves_the_old_range_alone():
    val = np.array([-np.inf, -1e9, -0.6, -0.5, -0.4, 0.0, 0.49, 0.5, 127.5, 254.4, 254.5, 255.0, 300.0, 1e9, 4e9, 3e38, np.inf, np.nan], F)
    assert tc.color_byte(val).tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 128, 254, 255, 255, 255, 255, 255, 255, 255, 0]
    old = np.linspace(0, 255, 100001).astype(F)
    assert np.array_equal(tc.color_byte(old), (old + F(0.5)).astype(np.int32).astype(np.uint8))       # what the statement did before


def test_same_bits_ignores_the_payload_of_a_nan_only():
    want = np.array([1.0, np.nan, -0.0, np.inf], F)
    other = want.copy()
    other.view(np.uint32)[1] = 0x7fc00001
    assert tc.same_bits(other, want) and tc.same_bits(want, want)
    assert not tc.same_bits(np.array([1.0, np.nan, 0.0, np.inf], F), want)       # the sign of a zero is compared
    assert not tc.same_bits(np.array([1.0, 2.0, -0.0, np.inf], F), want) and not tc.same_bits(np.array([np.nan, np.nan, -0.0, np.inf], F), want)
    assert not tc.same_bits(want[:3], want) and tc.same_bits(np.arange(3), np.arange(3)) and not tc.same_bits(np.arange(3), np.arange(1, 4))


# ---- sweep C ------------------------------------------------------------------------------------------------------------------------
def test_sweep_c_covers_every_operation_moves_refusals_and_empty_starts(pm):
    lives = [fz.life_case(pm, k) for k in range(N_C)]
    kinds = {kind: sum(1 for c in lives for op in c.ops if op[0] == kind) for kind in fz.OPS}
    moves, refusals = sum(c.moves for c in lives), sum(c.refusals for c in lives)
    zero = sum(1 for c in lives if c.zero_start)
    mid_set = sum(1 for c in lives if any(op[0] == "set_bricks" for op in c.ops[1:-1]))
    print("operations", kinds, "lengths", sorted(len(c.ops) for c in lives), "moves of old bricks", moves, "refusals", refusals,
          "lives that begin with an integrate into zero bricks", zero, "lives with a set_bricks in the middle", mid_set)
    assert all(v >= 20 for v in kinds.values()) and moves >= 10 and refusals >= 10 and zero >= 5 and mid_set >= 10
    assert all(c.ops[0][0] == "integrate" and c.ops[1][0] == "allocate" for c in lives if c.zero_start)
    assert all(6 <= len(c.ops) - c.forced <= 12 for c in lives)         # the refused allocates put in on purpose come on top
    assert sum(1 for c in lives if c.with_color) >= 10 and sum(1 for c in lives if not c.with_color) >= 10


def test_the_model_agrees_with_the_one_shot_statements(pm):
    """the model of sweep C against the statements it is built from: allocate, allocate, integrate is mask_dense of the dense statement
    on the union of the brick sets; a refused allocate and a read change nothing; a brick allocated after an integrate starts at zero"""
    checked = 0
    for k in range(6):
        c = fz.life_case(pm, k)
        n = len(c.cams)
        first, second, every = list(range(0, n, 2)), list(range(1, n, 2)), list(range(n))
        m = fz.Model(c)
        m.apply(("allocate", first))
        m.apply(("allocate", second))
        m.apply(("integrate", every))
        bricks = sc.allocate_statement(c.origin, c.voxel, c.dims, c.trunc, c.pad, c.cams, c.depths)
        assert np.array_equal(m.bricks, bricks)
        cols = c.cols if c.with_color else None
        want = sc.mask_dense(c.dims, bricks, *tc.integrate_statement(c.origin, c.voxel, c.dims, c.trunc, c.cams, c.depths, cols))
        assert tc.same_bits(m.total, want[0]) and np.array_equal(m.weight, want[1]) and (cols is None or np.array_equal(m.color4, want[2]))
        before = (m.bricks.copy(), m.total.copy(), m.weight.copy())
        m.apply(("refused", every))
        m.apply(("read",))
        assert np.array_equal(m.bricks, before[0]) and tc.same_bits(m.total, before[1]) and np.array_equal(m.weight, before[2])
        late = fz.Model(c)
        late.apply(("allocate", first[:1]))
        late.apply(("integrate", every))
        old = late.bricks.copy()
        late.apply(("allocate", every))
        fresh = sc.voxel_exists(c.dims, late.bricks & ~old)
        assert not late.weight[fresh].any() and not late.total[fresh].any()
        checked += bool((late.bricks & ~old).any())
    assert checked >= 3


# ---- named cases --------------------------------------------------------------------------------------------------------------------
def test_named_cases_are_what_they_say(pm):
    c = fz.cull_bound_case(pm)
    pos = tc.positions(c.origin, c.voxel, c.dims)
    assert len(c.cams) <= fz.CHUNK and [fz.cull_allowed(cam, pos) for cam in c.cams] == [True, False, True, False, False]
    assert c.cams[c.far].t[2] == 2.0 ** 41 and (c.depths[c.far] == F(2.0 ** 41)).all() and np.isnan(c.cams[c.nan_k].K[2]) and np.isnan(c.cams[c.nan_r].R[4])
    alone = [tc.integrate_statement(c.origin, c.voxel, c.dims, c.trunc, [cam], [d]) for cam, d in zip(c.cams, c.depths)]
    assert (alone[c.far][1] == 1).all() and not alone[c.far][0].any()          # z == 2^41 == d: s == 0 at every voxel
    assert not alone[c.nan_k][1].any() and not alone[c.nan_r][1].any()
    assert alone[0][1].any() and alone[2][1].any()                             # the ordinary views beside them contribute too
    for n in fz.FORCED_VIEWS:
        k = fz.chunk_case(pm, n)
        want = tc.integrate_statement(k.origin, k.voxel, k.dims, k.trunc, k.cams, k.depths, k.images)
        last = tc.integrate_statement(k.origin, k.voxel, k.dims, k.trunc, k.cams[-1:], k.depths[-1:], k.images[-1:])
        assert len(k.cams) == n and want[1].max() >= 2 and last[1].any()        # the view behind the boundary is seen
