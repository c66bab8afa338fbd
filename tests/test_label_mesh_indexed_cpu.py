"""The definition of vkv_label_mesh_indexed (include/vkvolume_amd.h) restated in numpy, label_indexed_np(), and what can be shown
of it without a GPU: de-indexed it is label_mesh_np() of tests/test_label_mesh_cpu.py bit for bit with the same face labels, on the labels of
the 14-components it is indexed_np() of tests/test_mesh_indexed_cpu.py in all three arrays, every listed vertex is used, a vertex's two labels
differ and at most one is 0, a face's label stands in the pair of each of its vertices, two half balls share every interface vertex, hiding a
label removes exactly the vertices whose pair becomes (0, 0), the entry points are declared, exported and bound, the kernels of
label_mesh_indexed.hip use no scratch memory, and vkvolume_amd.mesh cuts bodies out, orients normals and sums contact areas.
tests/test_gpu_label_mesh_indexed.py holds the kernels to label_indexed_np() bit for bit.

No context exists without a device, so of the rejections only the null context and the scratch sizes can be asked here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers as T
from tests.test_components_cpu import components_np
from tests.test_label_mesh_cpu import SHAPES, bordered, distinct_labels, half_balls, label_mesh_np, random_labels, shown_np
from tests.test_mesh_cpu import KINV255, TETS, ball, case_table, mesh_contents, same_bits, torus
from tests.test_mesh_indexed_cpu import indexed_np, same_u32
from vkvolume_amd import abi, labels as LB, lib, mesh as M, volume as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF = np.float32(0.5)


def label_indexed_np(labels, colors=None, vol=None, iso=None, box=None):
    """(vertices [v, 3] float32, normals [v, 3] float32 or None without a volume, vertex_labels [v, 2] uint32, faces [n, 3] int64, face_labels
    [n] uint32) of the header's sentences.  labels has the box's shape (d, h, w); vol (None: midpoints, no normals) the volume's; box = (x0,
    y0, z0, w, h, d)"""
    E = shown_np(labels, colors)
    d, h, w = E.shape
    x0, y0, z0 = (0, 0, 0) if box is None else tuple(int(v) for v in box[:3])
    assert box is None or tuple(box[3:]) == (w, h, d)
    empty = (np.zeros((0, 3), np.float32), None if vol is None else np.zeros((0, 3), np.float32), np.zeros((0, 2), np.uint32), np.zeros((0, 3), np.int64),
             np.zeros((0,), np.uint32))
    if min(d, h, w) < 2:
        return empty
    # the crossing edges: [z, y, x, d], d = dx + 2 dy + 4 dz; both ends in the box; the shown labels differ
    crossing = np.zeros((d, h, w, 8), bool)
    for dd in range(1, 8):
        dx, dy, dz = dd & 1, dd >> 1 & 1, dd >> 2
        crossing[:d - dz, :h - dy, :w - dx, dd] = E[:d - dz, :h - dy, :w - dx] != E[dz:, dy:, dx:]
    number = (np.cumsum(crossing.reshape(-1), dtype=np.int64) - 1).reshape(crossing.shape)        # the list's order: z, y, x, d rising
    z, y, x, dd = np.nonzero(crossing)
    if len(z) == 0:
        return empty
    dx, dy, dz = dd & 1, dd >> 1 & 1, dd >> 2
    t = np.full(len(z), HALF, np.float32)
    normals = None
    if vol is not None:
        whole = np.ascontiguousarray(vol, np.uint8)
        iso = np.float32(iso)
        f = whole[z0:z0 + d, y0:y0 + h, x0:x0 + w].astype(np.float32) * KINV255
        fa, fb = f[z, y, x], f[z + dz, y + dy, x + dx]
        with np.errstate(all="ignore"):
            t = np.where((fa >= iso) != (fb >= iso), (iso - fa) / (fb - fa), HALF)
        assert t.dtype == np.float32
        # central differences of the WHOLE volume's bytes, neighbours clamped to the volume
        padded = np.pad(whole.astype(np.int32), 1, mode="edge")
        grad = np.stack([padded[1:-1, 1:-1, 2:] - padded[1:-1, 1:-1, :-2], padded[1:-1, 2:, 1:-1] - padded[1:-1, :-2, 1:-1],
                         padded[2:, 1:-1, 1:-1] - padded[:-2, 1:-1, 1:-1]], axis=-1)
        ga, gb = grad[z + z0, y + y0, x + x0], grad[z + dz + z0, y + dy + y0, x + dx + x0]
        normals = -(ga.astype(np.float32) + t[:, None] * (gb - ga).astype(np.float32))
        assert normals.dtype == np.float32
    vertices = np.empty((len(z), 3), np.float32)
    for c, (p, o, has) in enumerate(((x, x0, dx), (y, y0, dy), (z, z0, dz))):
        ac = (p + o).astype(np.float32)
        vertices[:, c] = np.where(has == 1, ac + t, ac)
    pairs = np.stack([E[z, y, x], E[z + dz, y + dy, x + dx]], axis=1).astype(np.uint32)
    # faces: per cube, tetrahedron, group (by the first local vertex that carries the label) and triangle; the edge (a, b) of the cube at o
    # is the edge (o + a, a ^ b)
    corner = lambda j: E[(j >> 2):d - 1 + (j >> 2), (j >> 1 & 1):h - 1 + (j >> 1 & 1), (j & 1):w - 1 + (j & 1)]  # noqa: E731
    table = case_table()
    keys, faces, labs = [], [], []
    for tt in range(6):
        l = [corner(TETS[tt][i]) for i in range(4)]
        for g in range(4):
            starts = l[g] != 0
            for k in range(g):
                starts = starts & (l[k] != l[g])
            sub = sum((l[i] == l[g]).astype(np.int64) << i for i in range(4))
            for m in range(1, 15):
                _, edges = table[tt, m]
                cz, cy, cx = np.nonzero(starts & (sub == m))
                if len(cz) == 0:
                    continue
                cube = (cz * (h - 1) + cy) * (w - 1) + cx
                for k in range(len(edges) // 3):
                    out = np.empty((len(cz), 3), np.int64)
                    for v in range(3):
                        a, b = edges[3 * k + v]
                        assert a & b == a and a != b
                        at = (cz + (a >> 2), cy + (a >> 1 & 1), cx + (a & 1), a ^ b)
                        assert crossing[at].all()        # every triangle vertex lies on a crossing edge
                        out[:, v] = number[at]
                    keys.append((((cube * 6 + tt) * 4 + g) * 2) + k)
                    faces.append(out)
                    labs.append(l[g][cz, cy, cx].astype(np.uint32))
    keys, faces, labs = np.concatenate(keys), np.concatenate(faces), np.concatenate(labs)
    assert len(np.unique(keys)) == len(keys)
    order = np.argsort(keys, kind="stable")
    return vertices, normals, pairs, np.ascontiguousarray(faces[order]), np.ascontiguousarray(labs[order])


def check_properties(got, what=""):
    vertices, normals, pairs, faces, face_labels = got
    assert len(pairs) == len(vertices) and len(face_labels) == len(faces) and (normals is None or normals.shape == vertices.shape), what
    if len(vertices) == 0:
        assert len(faces) == 0, what
        return
    assert np.array_equal(np.unique(faces), np.arange(len(vertices))), "%s: a listed vertex is not referenced" % what
    assert (pairs[:, 0] != pairs[:, 1]).all() and ((pairs != 0).sum(axis=1) >= 1).all(), what
    assert (pairs[faces] == face_labels[:, None, None]).any(axis=2).all(), "%s: a face's label is missing from a vertex's pair" % what


# ---- against the triangle list -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_deindexed_it_is_the_triangle_list_bit_for_bit(shape):
    vol = np.random.default_rng(40).integers(0, 256, size=shape, dtype=np.uint8)
    for seed, colors in ((0, None), (1, LB.color_table(3, hidden=(2,))), (2, LB.color_table(2)), (3, LB.color_table(3, hidden=(1, 3)))):
        labels = random_labels(shape, seed)
        for v, iso in ((None, None), (vol, 0.5)):
            got = label_indexed_np(labels, colors, v, iso)
            want = label_mesh_np(labels, colors, v, iso)
            what = "%s seed %d" % (shape, seed)
            same_bits(got[0][got[3]].reshape(-1, 3, 3), want[0], what)
            assert np.array_equal(got[4], want[1]), what
            assert (got[1] is None) == (v is None)
            check_properties(got, what)
    if min(shape[1:]) > 1:
        box = (1, 1, 0, shape[2] - 1, shape[1] - 1, shape[0])
        big = np.random.default_rng(41).integers(0, 256, size=shape, dtype=np.uint8)
        labels = random_labels((box[5], box[4], box[3]), 5)
        got, want = label_indexed_np(labels, None, big, 0.4, box), label_mesh_np(labels, None, big, 0.4, box)
        same_bits(got[0][got[3]].reshape(-1, 3, 3), want[0], "%s box" % (shape,))
        assert np.array_equal(got[4], want[1])
        check_properties(got, "%s box" % (shape,))


def test_distinct_labels_use_every_edge_of_every_cube():
    labels = distinct_labels((3, 4, 5))
    got = label_indexed_np(labels)
    d, h, w = labels.shape
    edges = sum((d - (dd >> 2)) * (h - (dd >> 1 & 1)) * (w - (dd & 1)) for dd in range(1, 8))
    assert len(got[0]) == edges and len(got[3]) == 24 * (d - 1) * (h - 1) * (w - 1)
    check_properties(got, "distinct")
    same_bits(got[0][got[3]].reshape(-1, 3, 3), label_mesh_np(labels)[0], "distinct")


# ---- against the indexed isosurface ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", ["random", "ball", "torus"])
def test_the_labels_of_the_14_components_give_the_indexed_isosurface_bit_for_bit(content):
    vol = {"random": lambda: mesh_contents("random", (6, 7, 9), 17), "ball": ball, "torus": torus}[content]()
    d, h, w = vol.shape
    cases = [(0.5, None), (0.3, None), (0.5, (1, 2, 1, w - 2, h - 3, d - 1))] + ([(0.85, None)] if content == "random" else [])
    for iso, box in cases:
        labels = components_np(vol, iso, 14, box)[0]
        got = label_indexed_np(labels, None, vol, iso, box)
        wv, wn, wf = indexed_np(vol, iso, box)
        what = "%s iso %g box %s" % (content, iso, box)
        assert len(wv) > 0 and len(wf) > 0
        same_u32(got[0], wv, what + ": vertices")
        same_u32(got[1], wn, what + ": normals")
        assert np.array_equal(got[3], wf), what + ": faces"
        assert got[4].min() >= 1 and (got[2].min(axis=1) == 0).all()        # every vertex lies between a body and nothing
        check_properties(got, what)


# ---- shared interface vertices -------------------------------------------------------------------------------------------------------------
def test_two_half_balls_share_every_interface_vertex():
    labels = half_balls()
    vertices, _, pairs, faces, face_labels = got = label_indexed_np(labels)
    check_properties(got, "half balls")
    used = [np.unique(faces[face_labels == L]) for L in (1, 2)]
    interface = np.flatnonzero((pairs != 0).all(axis=1))
    assert len(interface) > 50 and set(map(tuple, pairs[interface].tolist())) <= {(1, 2), (2, 1)}
    assert set(interface.tolist()) == set(used[0].tolist()) & set(used[1].tolist())        # exactly the interface is shared, and all of it
    own = [len(label_indexed_np(np.where(labels == L, L, 0).astype(np.uint32))[0]) for L in (1, 2)]
    assert len(vertices) == own[0] + own[1] - len(interface) < own[0] + own[1]
    assert len(np.unique(vertices.view(np.uint32), axis=0)) == len(vertices)        # at midpoints no two edges give one position: a weld finds nothing


def test_hiding_a_label_removes_exactly_the_vertices_whose_pair_becomes_zero():
    labels = bordered(random_labels((4, 5, 6), 23))
    vol = np.random.default_rng(24).integers(0, 256, size=labels.shape, dtype=np.uint8)
    full = label_indexed_np(labels, LB.color_table(3), vol, 0.5)
    for hidden in (1, 2, 3):
        got = label_indexed_np(labels, LB.color_table(3, hidden=(hidden,)), vol, 0.5)
        pairs = np.where(full[2] == hidden, 0, full[2]).astype(np.uint32)
        keep = (pairs != 0).any(axis=1)
        assert 0 < keep.sum() < len(keep)
        same_u32(got[0], full[0][keep], "label %d hidden: vertices" % hidden)
        same_u32(got[1], full[1][keep], "label %d hidden: normals" % hidden)
        assert np.array_equal(got[2], pairs[keep])
        renumber = np.cumsum(keep) - 1
        stay = full[4] != hidden
        assert np.array_equal(got[3], renumber[full[3][stay]]) and np.array_equal(got[4], full[4][stay])
        check_properties(got, "label %d hidden" % hidden)
    # two hidden labels next to each other do not cross, and neither does a hidden label against 0
    assert len(label_indexed_np(labels, LB.color_table(3, hidden=(1, 2, 3)))[0]) == 0


# ---- entry points --------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    assert re.search(r"\bsize_t\s+vkv_label_mesh_indexed_scratch_bytes\s*\(\s*VkvExtent3D extent,\s*const VkvBox\s*\*box\)", header)
    assert re.search(r"\bint\s+vkv_label_mesh_indexed\s*\(\s*vkv_ctx\s*\*ctx,\s*const uint32_t\s*\*d_labels,\s*VkvExtent3D extent,\s*const VkvBox\s*\*box,\s*"
                     r"const uint32_t\s*\*d_colors,\s*uint64_t table_entries,\s*const uint8_t\s*\*d_volume,\s*float iso,\s*"
                     r"const uint8_t\s*\*d_visibility_map,\s*VkvExtent3D map_extent,\s*void\s*\*d_scratch,\s*float\s*\*d_vertices,\s*float\s*\*d_normals,\s*"
                     r"uint32_t\s*\*d_vertex_labels,\s*uint64_t capacity_vertices,\s*uint32_t\s*\*d_indices,\s*uint32_t\s*\*d_triangle_labels,\s*"
                     r"uint64_t capacity_triangles,\s*uint64_t\s*\*d_counts,\s*void\s*\*stream\)", header)
    L = lib.load()
    assert {"vkv_label_mesh_indexed", "vkv_label_mesh_indexed_scratch_bytes"} <= set(lib.EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    assert re.search(r"\bvkv_label_mesh_indexed$", out, flags=re.M) and re.search(r"\bvkv_label_mesh_indexed_scratch_bytes$", out, flags=re.M)
    at = L.vkv_label_mesh_indexed.argtypes
    assert len(at) == 20 and at[2] is abi.Extent3D and at[3] is C.POINTER(abi.Box) and at[5] is C.c_uint64 and at[7] is C.c_float
    assert at[9] is abi.Extent3D and at[14] is C.c_uint64 and at[17] is C.c_uint64 and at[13] is C.c_void_p and at[16] is C.c_void_p
    assert L.vkv_label_mesh_indexed_scratch_bytes.restype is C.c_size_t
    assert callable(lib.Context.label_mesh_indexed_rc) and callable(V.Volume.extract_label_mesh_indexed) and callable(LB.mesh_indexed_scratch_bytes)
    assert callable(M.body_submesh) and callable(M.oriented_corner_normals) and callable(M.contact_areas)


def test_scratch_bytes_and_the_null_context_without_a_device():
    L = lib.load()
    e = abi.Extent3D(258, 5, 19)
    size = LB.mesh_indexed_scratch_bytes
    assert size(e) >= 16 and size(e) % 8 == 0
    assert size(e) >= lib.mesh_indexed_scratch_bytes(e)        # the indexed mesh's block, and whatever the labels add
    assert size(abi.Extent3D(1, 5, 19)) >= 16 and size(abi.Extent3D(1, 1, 1)) >= 16        # no cubes, still a buffer
    for ext in ((3, 2, 66), (2, 66, 65), (300, 9, 20), (5, 3, 3), (7, 3, 3)):
        assert size(abi.Extent3D(*ext)) % 8 == 0
    assert size(e, abi.Box(1, 1, 1, 2, 2, 2)) <= size(e)
    assert size(abi.Extent3D(0, 5, 19)) == 0
    assert size(e, abi.Box(257, 0, 0, 2, 1, 1)) == 0 and size(e, abi.Box(0, 0, 0, 0, 1, 1)) == 0
    assert size(abi.Extent3D(0x80000000, 2, 2)) == 0
    assert size(abi.Extent3D(2048, 2048, 1024)) == 0        # 2^32 voxels: one more than the labels' calls take
    assert size(abi.Extent3D(2048, 2048, 1024), abi.Box(0, 0, 0, 2048, 2048, 1023)) > 0
    buf = (C.c_uint64 * 64)()
    a = C.addressof(buf)
    none = abi.Extent3D(0, 0, 0)
    assert L.vkv_label_mesh_indexed(None, a, abi.Extent3D(4, 4, 4), None, None, 0, None, 0.5, None, none, a + 64, None, None, None, 0, None, None, 0, a + 256,
                                    None) == abi.VKV_E_INVALID_ARGUMENT


def test_kernels_use_no_scratch_memory(tmp_path):
    kernels = T.kernel_listing("label_mesh_indexed.hip", tmp_path / "label_mesh_indexed.s")
    for name in ("k_lmeshi_count", "k_lmeshi_emit_vertices", "k_lmeshi_emit_indices"):
        assert len([k for k in kernels if name in k]) == 2, sorted(kernels)  # WIDE, narrow
    assert len([k for k in kernels if "k_lmeshi_scan" in k]) == 2, sorted(kernels)
    for k, v in kernels.items():
        print(k, v)
        assert v.get("ScratchSize") == 0, (k, v)
        assert v.get("NumVgprs") <= 128, (k, v)        # two waves per SIMD at the least


# ---- vkvolume_amd.mesh -------------------------------------------------------------------------------------------------------------------
def face_cross(vertices, faces):
    tri = vertices[faces].astype(np.float64)
    return np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])


def test_helpers_on_a_cube():
    labels = np.zeros((8, 9, 10), np.uint32)
    labels[2:6, 2:7, 2:5] = 1
    vol = np.where(labels != 0, 255, 0).astype(np.uint8)
    vertices, normals, pairs, faces, face_labels = label_indexed_np(labels, None, vol, 0.5)
    sv, sf, sn = M.body_submesh(vertices, faces, face_labels, 1, normals)
    same_u32(sv, vertices, "the only body is the whole mesh")
    same_u32(sn, normals, "normals")
    assert np.array_equal(sf, faces) and sf.dtype == np.int64
    assert M.body_submesh(vertices, faces, face_labels, 1)[2] is None
    ev, ef, _ = M.body_submesh(vertices, faces, face_labels, 2)
    assert ev.shape == (0, 3) and ef.shape == (0, 3)
    # the volume's normals point out of the cube, as its faces do: nothing is turned
    corner = M.oriented_corner_normals(vertices, faces, normals)
    assert corner.shape == (len(faces), 3, 3) and corner.dtype == np.float32
    same_u32(corner, normals[faces], "outward normals stay")
    same_u32(M.oriented_corner_normals(vertices, faces, -normals), normals[faces], "inward normals are turned")
    across, areas = M.contact_areas(vertices, faces, face_labels, pairs)
    assert across.dtype == np.uint32 and (across == 0).all() and list(areas) == [(1, 0)]
    area, _ = M.body_measures(vertices[faces], face_labels, 1)
    assert abs(areas[1, 0] - area[0]) < 1e-9
    with pytest.raises(ValueError):
        M.contact_areas(vertices, faces, face_labels, pairs[:-1])
    with pytest.raises(ValueError):
        M.body_submesh(vertices, faces, face_labels[:-1], 1)
    with pytest.raises(ValueError):
        M.oriented_corner_normals(vertices, faces, normals[:-1])


def test_helpers_on_two_half_balls():
    labels = half_balls()
    vertices, _, pairs, faces, face_labels = label_indexed_np(labels)
    tri, lab = label_mesh_np(labels)
    for L in (1, 2):
        sv, sf, _ = M.body_submesh(vertices, faces, face_labels, L)
        same_bits(sv[sf], tri[lab == L], "body %d" % L)        # the body's own triangles, in order
        assert np.array_equal(np.unique(sf), np.arange(len(sv))) and len(sv) < len(vertices)
        assert np.array_equal(sv, vertices[np.unique(faces[face_labels == L])])        # compacted in the list's order
    across, areas = M.contact_areas(vertices, faces, face_labels, pairs)
    assert set(across.tolist()) == {0, 1, 2, M.MIXED}        # the rim's faces have vertices on the interface and on the free surface
    assert areas[1, 2] > 20 and abs(areas[1, 2] - areas[2, 1]) < 1e-9 * areas[1, 2]
    area, _ = M.body_measures(tri, lab, 2)
    for L in (1, 2):
        assert abs(sum(a for (label, _), a in areas.items() if label == L) - area[L - 1]) < 1e-9 * area[L - 1]
        assert areas[L, 0] > areas[L, 3 - L] > areas[L, M.MIXED] > 0
    # normals along +x everywhere: body 1 (x below the cut) keeps them on the interface, body 2 gets them turned
    normals = np.tile(np.array([1, 0, 0], np.float32), (len(vertices), 1))
    corner = M.oriented_corner_normals(vertices, faces, normals)
    cross = face_cross(vertices, faces)
    assert (np.einsum("nkc,nc->nk", corner.astype(np.float64), cross) >= 0).all()
    assert np.array_equal(np.abs(corner), np.abs(normals[faces]))
    on_interface = (across == 1) | (across == 2)
    assert (corner[on_interface & (face_labels == 1), :, 0] == 1).all() and (corner[on_interface & (face_labels == 2), :, 0] == -1).all()


def test_helpers_on_a_three_label_junction():
    # three sectors around the line x = y = centre, in a zero border
    n = 9
    z, y, x = np.indices((n, n, n))
    labels = np.where(x < 4, 1, np.where(y < 4, 2, 3)).astype(np.uint32)
    labels[[0, -1]] = 0
    labels[:, [0, -1]] = 0
    labels[:, :, [0, -1]] = 0
    got = vertices, _, pairs, faces, face_labels = label_indexed_np(labels)
    check_properties(got, "junction")
    across, areas = M.contact_areas(vertices, faces, face_labels, pairs)
    assert {(1, 2), (2, 1), (1, 3), (3, 1), (2, 3), (3, 2), (1, 0), (2, 0), (3, 0)} <= set(areas)
    assert any(k[1] == M.MIXED for k in areas)        # the faces along the junction line
    for a, b in ((1, 2), (1, 3), (2, 3)):
        assert abs(areas[a, b] - areas[b, a]) < 1e-9 * areas[a, b]
    tri, lab = label_mesh_np(labels)
    area, _ = M.body_measures(tri, lab, 3)
    for L in (1, 2, 3):
        assert abs(sum(v for (label, _), v in areas.items() if label == L) - area[L - 1]) < 1e-9 * area[L - 1]
        sv, sf, _ = M.body_submesh(vertices, faces, face_labels, L)
        same_bits(sv[sf], tri[lab == L], "body %d" % L)
    # a vertex on the junction line itself lies between two of the three: no vertex has three labels, the faces around it disagree instead
    assert len(np.unique(pairs, axis=0)) >= 9
