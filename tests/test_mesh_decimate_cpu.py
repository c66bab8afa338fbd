"""vkv_mesh_decimate without a device: the numpy restatement of tests/mesh_decimate_ref.py against a second, sort-based one;
the cell rule at its edge values; closedness, exactly, on a ball and per label on the split-ball and junction label meshes, with faces kept
AND collapsed at every cell size used; the host helpers cluster_grid and drop_duplicate_faces; the entry points declared, exported and bound;
the scratch formula held to the header's text and to the library; the kernels' listing.  tests/test_gpu_mesh_decimate.py holds the kernels to
the restatement bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers as T
from tests import mesh_decimate_ref as D
from tests import mesh_smooth_ref as R
from vkvolume_amd import abi, lib, mesh as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- a second statement: sort the vertices by cell, sum each segment, number the named cells by a cumulative sum over the dense grid -----------
def decimate_sorted(vertices, faces, origin, cell, grid, counts=None, face_labels=None):
    p = np.asarray(vertices, np.float32).reshape(-1, 3)
    f_all = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    nv, nt = R.bounds(len(p), len(f_all), counts)
    origin, cell, grid = D.grid_of(origin, cell, grid)
    ids = np.zeros(nv, np.int64)
    for v in range(nv):        # the rule, one vertex and one axis at a time, on Python floats of float32 values
        c = []
        for a in range(3):
            u = np.float32(np.float32(p[v, a] - origin[a]) / cell[a])
            c.append((int(u) if u < np.float32(np.uint64(grid[a])) else grid[a] - 1) if u >= 0 else 0)
        ids[v] = c[0] + grid[0] * (c[1] + grid[1] * c[2])
    kept, out_faces = [], []
    mark = np.zeros(grid[0] * grid[1] * grid[2], bool)
    for t in range(nt):
        i = f_all[t]
        if (i >= nv).any():
            continue
        a, b, c = ids[i]
        if a != b and b != c and a != c:
            kept.append(t)
            out_faces.append((a, b, c))
            mark[[a, b, c]] = True
    number = np.cumsum(mark) - 1
    order = np.argsort(ids, kind="stable")
    q = (np.rint(p[:nv].astype(np.float64) * 16777216.0)).astype(np.int64)[order]
    starts = np.flatnonzero(np.r_[True, ids[order][1:] != ids[order][:-1]]) if nv else np.zeros(0, np.int64)
    sums = np.add.reduceat(q, starts, axis=0) if nv else np.zeros((0, 3), np.int64)        # int64: these meshes are far below 2^63
    sizes = np.diff(np.r_[starts, nv])
    seg_cell = ids[order][starts] if nv else np.zeros(0, np.int64)
    named = mark[seg_cell]
    out_vertices = np.array([[np.float32(float(int(s)) / float(k) * 2.0 ** -24) for s in row] for row, k in zip(sums[named], sizes[named])],
                            np.float32).reshape(-1, 3)
    return {
        "vertices": out_vertices,
        "faces": number[np.array(out_faces, np.int64).reshape(-1, 3)],
        "labels": None if face_labels is None else np.asarray(face_labels)[kept].astype(np.uint32),
        "vertex_map": np.where(mark[ids], number[ids], D.NONE).astype(np.uint32),
        "kept": np.array(kept, np.int64),
    }


def same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
            continue
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape, x.dtype, y.dtype)
        assert x.tobytes() == y.tobytes(), (what, k)


@pytest.mark.parametrize("name", sorted(R.small_meshes()))
def test_the_two_statements_agree_on_the_small_meshes(name):
    vertices, faces = R.small_meshes()[name]
    labels = (1 + np.arange(len(faces)) % 2).astype(np.uint32)
    for cell in (0.5, 1.0, 2.0, (0.5, 1.0, 3.0)):
        origin, size, grid = D.grid_for(vertices, cell)
        same(D.decimate_np(vertices, faces, origin, size, grid, face_labels=labels), decimate_sorted(vertices, faces, origin, size, grid, face_labels=labels),
             "%s, cell %s" % (name, cell))
    # a truncated input: faces past nt and faces that name vertices at or past nv are not used, and vertices past nv count in no mean
    counts = [99, max(len(faces) - 1, 0), 99, len(vertices) - 1]
    origin, size, grid = D.grid_for(vertices, 1.0)
    same(D.decimate_np(vertices, faces, origin, size, grid, counts=counts), decimate_sorted(vertices, faces, origin, size, grid, counts=counts), name + ", truncated")


@pytest.mark.parametrize("cell", D.CELLS, ids=str)
def test_the_two_statements_agree_on_the_junction(cell):
    vertices, _, faces, face_labels, _ = R.extracted("junction")
    origin, size, grid = M.cluster_grid((14, 14, 14), cell)
    want = D.decimate_np(vertices, faces, origin, size, grid, face_labels=face_labels)
    same(want, decimate_sorted(vertices, faces, origin, size, grid, face_labels=face_labels), "junction, cell %s" % (cell,))
    assert len(want["vertices"]) == want["faces"].max() + 1 and (np.bincount(want["faces"].reshape(-1)) > 0).all()        # no orphan
    assert np.array_equal(want["vertex_map"][faces[want["kept"]]], want["faces"])


def test_the_cell_rule_at_its_edges():
    origin, cell, grid = (-0.25, 1.0, 0.0), (2.0, 0.5, 3.0), (4, 5, 1)
    cases = [
        ((-0.25, 1.0, 0.0), (0, 0, 0)),        # on the origin
        ((1.75, 1.5, 2.9999), (1, 1, 0)),        # exactly on a boundary: the upper cell
        (np.nextafter(np.float32([1.75, 1.5, 3.0]), np.float32(-9)), (0, 0, 0)),        # one ulp below it
        ((-0.26, 0.0, -1e30), (0, 0, 0)),        # below the origin
        ((7.74, 3.49, 0.0), (3, 4, 0)),        # the last cell
        ((7.75, 3.5, 3.0), (3, 4, 0)),        # at its far side, which is the grid's: clamped
        ((1e30, np.inf, 5.0), (3, 4, 0)),        # past it
        ((-np.inf, np.nan, np.nan), (0, 0, 0)),        # NaN fails u >= 0
        ((np.nan, -0.0, 0.0), (0, 0, 0)),
    ]
    for p, (cx, cy, cz) in cases:
        got = D.cells_np(np.array([p], np.float32), origin, cell, grid)
        assert got.tolist() == [cx + 4 * (cy + 5 * cz)], (p, got)
    # (float) n rounds: 2^24 + 1 cells on an axis, and the last one is reached only by the clamp
    n = (1 << 24) + 1
    got = D.cells_np(np.array([[16777215.0, 0, 0], [16777216.0, 0, 0], [16777218.0, 0, 0], [3e9, 0, 0]], np.float32), (0, 0, 0), 1.0, (n, 1, 1))
    assert got.tolist() == [16777215, n - 1, n - 1, n - 1]
    # the division is the float32 one: 0.5 / 0.1f rounds to 5 in float32 and stays below it in double
    assert D.cells_np(np.array([[0.5, 0, 0]], np.float32), (0, 0, 0), (np.float32(0.1), 1, 1), (9, 1, 1)).tolist() == [5]
    assert int(0.5 / float(np.float32(0.1))) == 4


# ---- closedness -----------------------------------------------------------------------------------------------------------------------------
def closed_cases():
    vertices, faces, face_labels = D.ball()
    yield "ball", vertices, faces, face_labels, (24, 24, 24)
    for name, n in (("split ball", 24), ("junction", 14)):
        vertices, _, faces, face_labels, _ = R.extracted(name)
        yield name, vertices, faces, face_labels, (n, n, n)


@pytest.mark.parametrize("cell", D.CELLS, ids=str)
def test_closed_bodies_stay_closed_exactly(cell):
    for name, vertices, faces, face_labels, extent in closed_cases():
        origin, size, grid = M.cluster_grid(extent, cell)
        want = D.decimate_np(vertices, faces, origin, size, grid, face_labels=face_labels)
        # not vacuous: some faces are kept and some collapse, and the input is closed per label to begin with
        assert 0 < len(want["faces"]) < len(faces), (name, cell, len(want["faces"]), len(faces))
        assert len(want["vertices"]) < len(vertices)
        for label in np.unique(face_labels):
            assert not D.directed_edge_balance(faces[face_labels == label]), (name, label)
            assert not D.directed_edge_balance(want["faces"][want["labels"] == label]), (name, cell, label)
        assert not D.directed_edge_balance(want["faces"])
        # the test can fail: one face less leaves three edges open
        assert len(D.directed_edge_balance(want["faces"][1:])) == 3


def test_the_mean_takes_every_vertex_of_the_cell_and_moves_a_single_one_only_by_quantisation():
    vertices, faces = R.small_meshes()["isolated vertex"]        # vertex 4 belongs to no face
    vertices = vertices.copy()
    vertices[4] = vertices[3] + np.float32(0.01)
    origin, size, grid = (0, 0, 0), (0.5, 0.5, 0.5), (4, 4, 4)
    want = D.decimate_np(vertices, faces, origin, size, grid)
    assert len(want["faces"]) == 4 and want["vertex_map"][3] == want["vertex_map"][4] != D.NONE
    both = (R.q(vertices[3]).astype(object) + R.q(vertices[4]).astype(object))
    assert np.array_equal(want["vertices"][want["vertex_map"][3]], D.mean_np(both, 2))
    alone = want["vertices"][want["vertex_map"][0]]
    assert np.array_equal(alone, (R.q(vertices[0]).astype(np.float64) / R.FIX).astype(np.float32)) and np.abs(alone - vertices[0]).max() <= 2.0 ** -25


# ---- the host helpers -----------------------------------------------------------------------------------------------------------------------
def test_cluster_grid():
    origin, cell, grid = M.cluster_grid((24, 10, 7), 2)
    assert origin.dtype == np.float32 and cell.dtype == np.float32 and origin.tolist() == [-0.25] * 3 and cell.tolist() == [2.0] * 3
    assert grid == (12, 5, 4)        # ceil(23.25 / 2), ceil(9.25 / 2), ceil(6.25 / 2)
    assert M.cluster_grid(abi.Extent3D(24, 10, 7), 2)[2] == grid
    origin, cell, grid = M.cluster_grid(abi.Box(3, 4, 5, 8, 9, 1), (2, 3, 5))
    assert origin.tolist() == [2.75, 3.75, 4.75] and cell.tolist() == [2.0, 3.0, 5.0] and grid == (4, 3, 1)
    for extent, size in (((24, 24, 24), 2), ((14, 14, 14), 3), ((9, 40, 2), (2, 3, 5))):
        origin, cell, grid = M.cluster_grid(extent, size)
        # every voxel centre and every midpoint between two lies strictly inside a cell, none on a boundary, and the last one inside the grid
        for a in range(3):
            at = (np.arange(0, 2 * extent[a] - 1) * 0.5 - origin[a]) / cell[a]
            assert (at != np.floor(at)).all() and at.min() > 0
            assert at.max() < grid[a] and int(at.max()) == grid[a] - 1        # and no cell more than is needed
    for bad in (0, -1, float("nan"), float("inf"), (1, 0, 1)):
        with pytest.raises(ValueError):
            M.cluster_grid((4, 4, 4), bad)


def test_drop_duplicate_faces():
    faces = np.array([[0, 1, 2], [1, 2, 0], [2, 1, 0], [0, 1, 2], [3, 4, 5], [0, 2, 1], [5, 3, 4], [2, 0, 1]])
    assert M.drop_duplicate_faces(faces).tolist() == [[0, 1, 2], [2, 1, 0], [3, 4, 5]]        # a reversed face is another face; the first stays
    labels = np.array([1, 2, 1, 1, 7, 1, 7, 2], np.uint32)
    kept, kept_labels = M.drop_duplicate_faces(faces, labels)
    assert kept.tolist() == [[0, 1, 2], [1, 2, 0], [2, 1, 0], [3, 4, 5]] and kept_labels.tolist() == [1, 2, 1, 7] and kept_labels.dtype == np.uint32
    assert M.drop_duplicate_faces(np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 1, 1]])).tolist() == [[0, 0, 1], [0, 1, 1]]        # ties in the least number
    assert M.drop_duplicate_faces(np.zeros((0, 3), np.int64)).shape == (0, 3)
    with pytest.raises(ValueError):
        M.drop_duplicate_faces(faces, labels[:-1])
    # on a decimated mesh that does hold duplicates: two plates one voxel thick, two voxels apart, in cells that span both along z.  The
    # upper sides of both plates become the same faces, the lower sides their reverses
    from tests.test_label_mesh_indexed_cpu import label_indexed_np
    labels = np.zeros((12, 16, 16), np.uint32)
    labels[4, 3:13, 3:13] = labels[6, 3:13, 3:13] = 1
    vertices, _, _, f, face_labels = label_indexed_np(labels)
    want = D.decimate_np(vertices, f, *M.cluster_grid((16, 16, 12), (2, 2, 8)), face_labels=face_labels)
    f = want["faces"]
    kept, kept_labels = M.drop_duplicate_faces(f, want["labels"])
    # an independent count: a face up to rotation is its sorted triple and its parity
    even = ((f[:, 0] < f[:, 1]).astype(int) + (f[:, 1] < f[:, 2]).astype(int) + (f[:, 2] < f[:, 0]).astype(int)) == 2
    distinct = np.unique(np.concatenate([np.sort(f, axis=1), even[:, None].astype(np.int64)], axis=1), axis=0)
    assert len(f) == 200 and len(kept) == len(distinct) == 100 and (kept_labels == 1).all()        # every face came twice, one of each stays
    assert np.array_equal(kept[0], f[0])
    # each face and its reverse were doubled alike, so the body is closed before and after, exactly
    assert not D.directed_edge_balance(f) and not D.directed_edge_balance(kept)
    assert len(D.directed_edge_balance(kept[1:])) == 3


# ---- entry points ---------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    assert re.search(r"\bsize_t\s+vkv_mesh_decimate_scratch_bytes\s*\(\s*uint64_t capacity_vertices,\s*uint64_t capacity_triangles,\s*VkvExtent3D grid_extent\)",
                     header)
    assert re.search(r"\bint\s+vkv_mesh_decimate\s*\(\s*vkv_ctx\s*\*ctx,\s*const float\s*\*d_vertices,\s*const uint32_t\s*\*d_indices,\s*"
                     r"const uint32_t\s*\*d_triangle_labels,\s*uint64_t capacity_vertices,\s*uint64_t capacity_triangles,\s*const uint64_t\s*\*d_counts,\s*"
                     r"const float\s*\*grid_origin,\s*const float\s*\*grid_cell,\s*VkvExtent3D grid_extent,\s*void\s*\*d_scratch,\s*float\s*\*d_out_vertices,\s*"
                     r"uint64_t out_capacity_vertices,\s*uint32_t\s*\*d_out_indices,\s*uint32_t\s*\*d_out_triangle_labels,\s*uint64_t out_capacity_triangles,\s*"
                     r"uint32_t\s*\*d_vertex_map,\s*uint64_t\s*\*d_out_counts,\s*void\s*\*stream\)", header)
    assert "Not here: nothing is decimated" not in header and "Not here: decimation" not in header and header.count("vkv_mesh_decimate (DESIGN.md §5.25)") >= 1
    for word in ("quadric error metrics", "edge collapse", "removal of duplicate faces on the device", "feature preservation"):
        assert word in header[header.index("decimated by vertex clustering"):], word
    names = ["vkv_mesh_decimate_scratch_bytes", "vkv_mesh_decimate"]
    L = lib.load()
    assert set(names) <= set(lib.EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    for name in names:
        assert re.search(r"\b%s$" % name, out, flags=re.M), name
    assert L.vkv_mesh_decimate_scratch_bytes.restype is C.c_size_t and L.vkv_mesh_decimate_scratch_bytes.argtypes == [C.c_uint64, C.c_uint64, abi.Extent3D]
    at = L.vkv_mesh_decimate.argtypes
    assert len(at) == 19 and at[4] is C.c_uint64 and at[7] is C.POINTER(C.c_float) and at[8] is C.POINTER(C.c_float) and at[9] is abi.Extent3D
    assert at[12] is C.c_uint64 and at[15] is C.c_uint64
    assert callable(lib.Context.mesh_decimate_rc)
    for name in ("decimate", "cluster_grid", "drop_duplicate_faces", "decimate_scratch_bytes"):
        assert callable(getattr(M, name))


def test_the_binding_passes_the_grid_as_two_float_arrays():
    from tests.test_binding_cpu import HANDLE, context
    ctx, rec = context()
    e = abi.Extent3D(4, 5, 6)
    assert ctx.mesh_decimate_rc(10, 11, 12, 100, 200, 13, (0.25, -1, 2), (2, 3, 5), e, 14, 15, 50, 16, 17, 60, 18, 19, 99) == 0
    got = rec.last("vkv_mesh_decimate")
    assert got[:7] == (HANDLE, 10, 11, 12, 100, 200, 13) and got[7] == [0.25, -1.0, 2.0] and got[8] == [2.0, 3.0, 5.0]
    assert got[10:] == (14, 15, 50, 16, 17, 60, 18, 19, 99)
    ctx.mesh_decimate_rc(10, 11, None, 100, 200, 13, None, None, e, 14, None, 0, None, None, 0, None, 19)
    got = rec.last("vkv_mesh_decimate")
    assert got[3] is None and got[7] is None and got[8] is None and got[10:] == (14, None, 0, None, None, 0, None, 19, 0)


def test_scratch_bytes_against_the_headers_text_and_the_null_context_without_a_device():
    header = " ".join(open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read().replace("\n *", " ").split())
    formula = "32 * C + 8 * ceil(C / 4096) + 8 * B + 8 * ceil(B / 4096) + roundup8(4 * capacity_vertices)"
    assert formula in header and "C = n_x n_y n_z cells and B = ceil(capacity_triangles / 256)" in header
    ceil = lambda a, b: (a + b - 1) // b  # noqa: E731
    L = lib.load()
    size = L.vkv_mesh_decimate_scratch_bytes
    for cv, ct, grid in ((0, 0, (1, 1, 1)), (1, 1, (1, 1, 1)), (3, 5, (2, 3, 5)), (4097, 257, (17, 16, 16)), (5573, 13064, (16, 16, 16)), (7, 256 * 4096 + 1, (4096, 1, 1)),
                         (55_000_000, 110_000_001, (512, 512, 398)), (0xffffffff, 0xffffffff, (0xffffffff, 1, 1)), (1, 1, (65535, 65537, 1))):
        cells, blocks = grid[0] * grid[1] * grid[2], ceil(ct, 256)
        want = 32 * cells + 8 * ceil(cells, 4096) + 8 * blocks + 8 * ceil(blocks, 4096) + ((4 * cv + 7) & ~7)
        assert size(cv, ct, abi.Extent3D(*grid)) == want == M.decimate_scratch_bytes(cv, ct, grid) == M.decimate_scratch_bytes(cv, ct, abi.Extent3D(*grid)), (cv, ct, grid)
        assert want % 8 == 0 and want >= 40
    for cv, ct, grid in ((1 << 32, 1, (1, 1, 1)), (1, 1 << 32, (1, 1, 1)), (1, 1, (0, 1, 1)), (1, 1, (1, 0, 1)), (1, 1, (1, 1, 0)), (1, 1, (65536, 65536, 1)),
                         (1, 1, (0xffffffff, 0xffffffff, 0xffffffff)), (1, 1, (1 << 16, 1 << 8, 1 << 8))):
        if max(grid) <= 0xffffffff:
            assert size(cv, ct, abi.Extent3D(*grid)) == 0, (cv, ct, grid)
        assert M.decimate_scratch_bytes(cv, ct, grid) == 0, (cv, ct, grid)
    buf = (C.c_uint64 * 64)()
    a = C.addressof(buf)
    three = (C.c_float * 3)(1, 1, 1)
    assert L.vkv_mesh_decimate(None, a, a + 64, None, 3, 1, a + 128, three, three, abi.Extent3D(1, 1, 1), a + 192, a + 256, 3, a + 320, None, 1, None, a + 384,
                               None) == abi.VKV_E_INVALID_ARGUMENT
    assert not any(buf)


def test_kernels_use_no_scratch_memory(tmp_path):
    kernels = T.kernel_listing("mesh_decimate.hip", tmp_path / "mesh_decimate.s")
    for name in ("k_mdec_clear", "k_mdec_accumulate", "k_mdec_classify", "k_mdec_scan_cells", "k_mdec_scan_faces", "k_mdec_scan_totals", "k_mdec_emit_vertices",
                 "k_mdec_vertex_map", "k_mdec_emit_faces"):
        assert len([k for k in kernels if name in k]) == 1, (name, sorted(kernels))
    assert len(kernels) == 9
    for k, v in kernels.items():
        print(k, v)
        assert v.get("ScratchSize") == 0, (k, v)
        assert v.get("NumVgprs") <= 64, (k, v)        # gathers and atomics hide their latency behind other waves: full occupancy
    text = open(tmp_path / "mesh_decimate.s").read()
    assert not re.search(r"atomic\w*_f(32|64)|atomic_pk_add", text)        # integer atomics only
    assert re.search(r"global_atomic_add_x2\b", text) and not re.search(r"global_atomic_add_x2\b.*\bsc0\b", text)        # 64-bit, and none waits for its result
