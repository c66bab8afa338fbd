"""The definition of vkv_isosurface_mesh_indexed (include/vkvolume_amd.h) restated in numpy, indexed_np(), and what can be shown
of it without a GPU: de-indexed it is mesh_np() of tests/test_mesh_cpu.py bit for bit, every listed vertex is used, the vertices lie in
(z, y, x, d) order, there are exactly as many as a bitwise weld finds unless iso sits on a voxel's value, the surfaces of a ball and a torus
have the Euler characteristics of a sphere and a torus straight from the faces, the gradient normals of the ball point outwards and agree with
the adjacent faces, a box's vertices and normals are the whole volume's, the entry points are declared, exported and bound, the kernels of
mesh_indexed.hip use no scratch memory, and vkvolume_amd.mesh unindexes and writes PLY.  tests/test_gpu_mesh_indexed.py holds the kernels to
indexed_np() bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers as T
from tests.test_mesh_cpu import KINV255, SHAPES, TETS, ball, bordered_random, case_table, mesh_contents, mesh_np, same_bits, torus
from vkvolume_amd import abi, lib, mesh as M, volume as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def indexed_np(vol_dhw, iso, box=None, origin=(0, 0, 0)):
    """(vertices [v, 3] float32, normals [v, 3] float32, faces [n, 3] int64) of the header's sentences.  box = (x0, y0, z0, w, h, d);
    origin: where voxel (0, 0, 0) of vol_dhw lies in the volume whose coordinates the vertices carry (vol_dhw is a window cut from it)"""
    whole = np.ascontiguousarray(vol_dhw, np.uint8)
    x0, y0, z0, w, h, d = (0, 0, 0) + whole.shape[::-1] if box is None else box
    vol = whole[z0:z0 + d, y0:y0 + h, x0:x0 + w]
    empty = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)
    if min(d, h, w) < 2:
        return empty
    iso = np.float32(iso)
    f = vol.astype(np.float32) * KINV255
    inside = f >= iso
    # the crossing edges: [z, y, x, d], d = dx + 2 dy + 4 dz; both ends in the box
    crossing = np.zeros((d, h, w, 8), bool)
    for dd in range(1, 8):
        dx, dy, dz = dd & 1, dd >> 1 & 1, dd >> 2
        crossing[:d - dz, :h - dy, :w - dx, dd] = inside[:d - dz, :h - dy, :w - dx] != inside[dz:, dy:, dx:]
    number = (np.cumsum(crossing.reshape(-1), dtype=np.int64) - 1).reshape(crossing.shape)        # the list's order: z, y, x, d rising
    z, y, x, dd = np.nonzero(crossing)
    if len(z) == 0:
        return empty
    dx, dy, dz = dd & 1, dd >> 1 & 1, dd >> 2
    fa, fb = f[z, y, x], f[z + dz, y + dy, x + dx]
    t = (iso - fa) / (fb - fa)
    assert t.dtype == np.float32
    vertices = np.empty((len(z), 3), np.float32)
    for c, (p, o, has) in enumerate(((x, x0 + int(origin[0]), dx), (y, y0 + int(origin[1]), dy), (z, z0 + int(origin[2]), dz))):
        ac = (p + o).astype(np.float32)
        vertices[:, c] = np.where(has == 1, ac + t, ac)
    # normals: central differences of the WHOLE volume's bytes, neighbours clamped to the volume
    padded = np.pad(whole.astype(np.int32), 1, mode="edge")
    D, H, W = whole.shape
    grad = np.stack([padded[1:-1, 1:-1, 2:] - padded[1:-1, 1:-1, :-2], padded[1:-1, 2:, 1:-1] - padded[1:-1, :-2, 1:-1],
                     padded[2:, 1:-1, 1:-1] - padded[:-2, 1:-1, 1:-1]], axis=-1)
    assert grad.shape == (D, H, W, 3)
    ga, gb = grad[z + z0, y + y0, x + x0], grad[z + dz + z0, y + dy + y0, x + dx + x0]
    normals = -(ga.astype(np.float32) + t[:, None] * (gb - ga).astype(np.float32))
    assert normals.dtype == np.float32
    # faces: the triangles of mesh_np in its order, each edge (a, b) of the cube with origin o named (o + a, a ^ b)
    corner = lambda a, j: a[(j >> 2):d - 1 + (j >> 2), (j >> 1 & 1):h - 1 + (j >> 1 & 1), (j & 1):w - 1 + (j & 1)]  # noqa: E731
    table = case_table()
    keys, faces = [], []
    for tt in range(6):
        sub = sum(corner(inside, TETS[tt][i]).astype(np.int64) << i for i in range(4))
        for m in range(1, 15):
            _, edges = table[tt, m]
            cz, cy, cx = np.nonzero(sub == m)
            if len(cz) == 0:
                continue
            cube = (cz * (h - 1) + cy) * (w - 1) + cx
            for k in range(len(edges) // 3):
                out = np.empty((len(cz), 3), np.int64)
                for v in range(3):
                    a, b = edges[3 * k + v]
                    assert a & b == a and a != b
                    out[:, v] = number[cz + (a >> 2), cy + (a >> 1 & 1), cx + (a & 1), a ^ b]
                    assert crossing[cz + (a >> 2), cy + (a >> 1 & 1), cx + (a & 1), a ^ b].all()
                keys.append((cube * 6 + tt) * 2 + k)
                faces.append(out)
    keys, faces = np.concatenate(keys), np.concatenate(faces)
    return vertices, normals, np.ascontiguousarray(faces[np.argsort(keys, kind="stable")])


def vertex_keys(vol_dhw, iso, box=None):
    """(z, y, x, d) of every vertex of indexed_np in its order, in VOLUME coordinates"""
    whole = np.ascontiguousarray(vol_dhw, np.uint8)
    x0, y0, z0, w, h, d = (0, 0, 0) + whole.shape[::-1] if box is None else box
    inside = whole[z0:z0 + d, y0:y0 + h, x0:x0 + w].astype(np.float32) * KINV255 >= np.float32(iso)
    out = []
    if min(d, h, w) >= 2:
        for z in range(d):
            for y in range(h):
                for x in range(w):
                    for dd in range(1, 8):
                        bx, by, bz = x + (dd & 1), y + (dd >> 1 & 1), z + (dd >> 2)
                        if bx < w and by < h and bz < d and inside[z, y, x] != inside[bz, by, bx]:
                            out.append((z + z0, y + y0, x + x0, dd))
    return out


def same_u32(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    g, w = got.view(np.uint32), want.view(np.uint32)
    assert np.array_equal(g, w), "%s: %d words differ, first at %s: got %s want %s" % (
        what, int((g != w).sum()), np.argwhere(g != w)[:4].tolist(), got[g != w][:4].tolist(), want[g != w][:4].tolist())


def inner_box(shape_dhw):
    d, h, w = shape_dhw
    x0, y0, z0 = (1 if w > 2 else 0), (1 if h > 2 else 0), (1 if d > 2 else 0)
    return (x0, y0, z0, max(w - x0 - (1 if w > 3 else 0), 1), max(h - y0 - (1 if h > 3 else 0), 1), max(d - z0 - (1 if d > 3 else 0), 1))


def euler(faces):
    e = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    return len(np.unique(faces)), len(np.unique(e, axis=0)), len(faces)


# ---- entry points ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    assert re.search(r"\bsize_t\s+vkv_isosurface_mesh_indexed_scratch_bytes\s*\(\s*VkvExtent3D extent,\s*const VkvBox\s*\*box\)", header)
    assert re.search(r"\bint\s+vkv_isosurface_mesh_indexed\s*\(\s*vkv_ctx\s*\*ctx,\s*const uint8_t\s*\*d_volume,\s*VkvExtent3D extent,\s*const VkvBox\s*\*box,\s*"
                     r"float iso,\s*const uint8_t\s*\*d_max_map,\s*VkvExtent3D map_extent,\s*void\s*\*d_scratch,\s*float\s*\*d_vertices,\s*"
                     r"float\s*\*d_normals,\s*uint64_t capacity_vertices,\s*uint32_t\s*\*d_indices,\s*uint64_t capacity_triangles,\s*"
                     r"uint64_t\s*\*d_counts,\s*void\s*\*stream\)", header)
    L = lib.load()
    assert {"vkv_isosurface_mesh_indexed", "vkv_isosurface_mesh_indexed_scratch_bytes"} <= set(lib.EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    assert re.search(r"\bvkv_isosurface_mesh_indexed$", out, flags=re.M) and re.search(r"\bvkv_isosurface_mesh_indexed_scratch_bytes$", out, flags=re.M)
    at = L.vkv_isosurface_mesh_indexed.argtypes
    assert len(at) == 15 and at[2] is abi.Extent3D and at[3] is C.POINTER(abi.Box) and at[4] is C.c_float and at[6] is abi.Extent3D
    assert at[10] is C.c_uint64 and at[12] is C.c_uint64 and at[9] is C.c_void_p and at[11] is C.c_void_p
    assert L.vkv_isosurface_mesh_indexed_scratch_bytes.restype is C.c_size_t
    assert callable(lib.Context.isosurface_mesh_indexed) and callable(lib.Context.isosurface_mesh_indexed_rc)
    assert callable(lib.mesh_indexed_scratch_bytes) and callable(V.Volume.extract_isosurface_indexed)
    assert callable(M.unindex) and callable(M.write_ply)


def test_scratch_bytes_and_bad_arguments_without_a_device():
    L = lib.load()
    e = abi.Extent3D(258, 5, 19)
    for extent in (e, abi.Extent3D(1, 5, 19), abi.Extent3D(1, 1, 1), abi.Extent3D(257, 2, 2), abi.Extent3D(2, 1026, 1026)):
        n = lib.mesh_indexed_scratch_bytes(extent)
        assert n >= 16 and n % 8 == 0, (extent.width, n)
    assert lib.mesh_indexed_scratch_bytes(abi.Extent3D(1, 5, 19)) == 16        # no cubes, no edges: only the totals are written
    assert 16 <= lib.mesh_indexed_scratch_bytes(e, abi.Box(1, 1, 1, 2, 2, 2)) <= lib.mesh_indexed_scratch_bytes(e)
    # 16 bytes per entry of 256 voxels of a row: 257 voxels are two entries where 256 cubes are one
    assert lib.mesh_indexed_scratch_bytes(abi.Extent3D(257, 2, 2)) > lib.mesh_indexed_scratch_bytes(abi.Extent3D(256, 2, 2))
    assert lib.mesh_indexed_scratch_bytes(abi.Extent3D(0, 5, 19)) == 0
    assert lib.mesh_indexed_scratch_bytes(e, abi.Box(257, 0, 0, 2, 1, 1)) == 0 and lib.mesh_indexed_scratch_bytes(e, abi.Box(0, 0, 0, 0, 1, 1)) == 0
    assert lib.mesh_indexed_scratch_bytes(abi.Extent3D(0x80000000, 2, 2)) == 0
    buf = (C.c_uint64 * 128)()
    a = C.addressof(buf)
    none = abi.Extent3D(0, 0, 0)
    bad = abi.VKV_E_INVALID_ARGUMENT
    assert L.vkv_isosurface_mesh_indexed(None, a, abi.Extent3D(4, 4, 4), None, 0.5, None, none, a + 64, None, None, 0, None, 0, a + 512, None) == bad
    assert L.vkv_isosurface_mesh_indexed(None, a, abi.Extent3D(4, 4, 4), None, 0.5, None, none, a + 64, a + 600, None, 1 << 32, None, 0, a + 512, None) == bad
    assert not any(buf)


# ---- the statement against the triangle list ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_deindexed_it_is_the_triangle_list_and_every_vertex_is_used(shape):
    for k, content in enumerate(("random", "ball", "below", "above", "voxel")):
        vol = mesh_contents(content, shape, seed=40 + k)
        for box in (None, inner_box(shape)):
            for iso in (0.5, 0.25):
                what = "%s %s box %s iso %g" % (content, shape, box, iso)
                vertices, normals, faces = indexed_np(vol, iso, box)
                want = mesh_np(vol, iso, box)
                same_bits(vertices[faces] if len(faces) else np.zeros((0, 3, 3), np.float32), want, what)
                assert normals.shape == vertices.shape
                if len(vertices):
                    assert np.array_equal(np.unique(faces), np.arange(len(vertices))), what        # every vertex is referenced
                keys = vertex_keys(vol, iso, box)
                assert len(keys) == len(vertices) and keys == sorted(keys), what
                b = (0, 0, 0) + shape[::-1] if box is None else box
                if min(b[3:]) < 2:
                    assert len(vertices) == 0 and len(faces) == 0, what
                # the position names its edge: the integer part is the owner, the moving axes are those of d
                for (z, y, x, dd), p in zip(keys, vertices):
                    assert [int(np.floor(p[0])), int(np.floor(p[1])), int(np.floor(p[2]))] in ([x, y, z], [x + (dd & 1), y + (dd >> 1 & 1), z + (dd >> 2)]), what


def test_one_vertex_per_welded_vertex_unless_iso_sits_on_a_voxel_value():
    vol = np.random.default_rng(5).integers(0, 256, size=(5, 6, 7), dtype=np.uint8)
    for iso in (0.5, 0.3):        # no byte / 255 equals either
        assert not (vol.astype(np.float32) * KINV255 == np.float32(iso)).any()
        vertices, _, faces = indexed_np(vol, iso)
        welded, welded_faces = M.weld(mesh_np(vol, iso))
        assert len(vertices) == len(welded) > 0
        assert len(np.unique(vertices.view(np.uint32), axis=0)) == len(vertices)
    iso = 100 / 255        # next to byte 100's value: t rounds away in a_c + t, and the edges that meet in such a voxel share its position
    assert (vol == 100).any()
    vertices, _, faces = indexed_np(vol, iso)
    welded, _ = M.weld(mesh_np(vol, iso))
    assert (len(vertices), len(welded)) == (537, 534)        # they stay separate vertices
    same_bits(vertices[faces], mesh_np(vol, iso), "iso on a voxel's value")


def test_ball_is_a_sphere_with_outward_normals_that_agree_with_its_faces():
    vol = ball()
    vertices, normals, faces = indexed_np(vol, 0.5)
    v, e, f = euler(faces)
    assert (v, e, f) == (914, 2736, 1824) and v - e + f == 2 and len(vertices) == 914
    length = np.linalg.norm(normals.astype(np.float64), axis=1)
    assert (length > 0).all()
    assert (np.einsum("ij,ij->i", normals.astype(np.float64), vertices.astype(np.float64) - 5.5) > 0).all()
    unit = normals.astype(np.float64) / length[:, None]
    tri = vertices[faces]
    face = M.face_normals(tri).astype(np.float64)
    assert (np.linalg.norm(face, axis=1) > 0.99).all()
    dots = np.einsum("ijk,ik->ij", unit[faces], face)        # every vertex of every face against that face
    print("ball: %d vertices, minimum dot(unit vertex normal, adjacent face normal) %.4f" % (len(vertices), dots.min()))
    assert dots.min() > 0.9


def test_torus_has_euler_characteristic_zero():
    vertices, _, faces = indexed_np(torus(), 0.5)
    v, e, f = euler(faces)
    assert f == 2272 and v == len(vertices) and v - e + f == 0
    vertices, _, faces = indexed_np(bordered_random(), 0.5)
    v, e, f = euler(faces)
    assert v == len(vertices) and (v - e + f) % 2 == 0        # closed: a sum of 2 - 2 g over its components


def test_a_box_holds_the_whole_volumes_vertices_and_normals_for_its_edges():
    vol = np.random.default_rng(5).integers(0, 256, size=(5, 6, 7), dtype=np.uint8)
    box = (2, 1, 1, 4, 3, 3)
    whole = dict(zip(vertex_keys(vol, 0.5), range(10 ** 6)))
    wv, wn, _ = indexed_np(vol, 0.5)
    bv, bn, bf = indexed_np(vol, 0.5, box)
    keys = vertex_keys(vol, 0.5, box)
    assert len(keys) == len(bv) > 0
    rows = [whole[k] for k in keys]
    same_u32(bv, wv[rows], "box vertices")
    same_u32(bn, wn[rows], "box normals")
    assert len(bv) < len(wv)
    same_bits(bv[bf], mesh_np(vol, 0.5, box), "box")


# ---- vkvolume_amd.mesh -------------------------------------------------------------------------------------------------------------------
def read_ply(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = nf = None
    props, element = [], None
    for line in lines[2:]:
        w = line.split()
        if w[:1] == ["element"]:
            element = w[1]
            if element == "vertex":
                nv = int(w[2])
            else:
                assert element == "face"
                nf = int(w[2])
        elif w[:1] == ["property"] and element == "vertex":
            assert w[1] == "float"
            props.append(w[2])
        elif w[:1] == ["property"]:
            assert w[1:] == ["list", "uchar", "uint", "vertex_indices"]
    body = data[end:]
    assert len(body) == 4 * len(props) * nv + 13 * nf
    table = np.frombuffer(body, "<f4", count=len(props) * nv).reshape(nv, len(props))
    rec = np.frombuffer(body, np.dtype([("n", "u1"), ("v", "<u4", 3)]), offset=4 * len(props) * nv)
    assert (rec["n"] == 3).all()
    return props, table, rec["v"]


def test_write_ply_round_trips(tmp_path):
    vertices, normals, faces = indexed_np(ball(), 0.5)
    path = str(tmp_path / "ball.ply")
    M.write_ply(path, vertices, faces.astype(np.uint32), normals)
    props, table, back = read_ply(path)
    assert props == ["x", "y", "z", "nx", "ny", "nz"]
    same_u32(table[:, :3], vertices, "ply vertices")
    same_u32(table[:, 3:], normals, "ply normals")
    assert back.dtype == np.uint32 and np.array_equal(back, faces)
    M.write_ply(path, vertices, faces)
    props, table, back = read_ply(path)
    assert props == ["x", "y", "z"] and np.array_equal(back, faces)
    same_u32(table, vertices, "ply vertices, no normals")
    M.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))
    assert len(read_ply(path)[1]) == 0 and len(read_ply(path)[2]) == 0
    with pytest.raises(ValueError):
        M.write_ply(path, vertices, faces, normals[:-1])
    with pytest.raises(ValueError):
        M.write_ply(path, vertices.reshape(-1), faces)


def test_unindex_and_the_coordinate_maps_on_vertex_arrays():
    tri = mesh_np(ball(), 0.5)
    same_bits(M.unindex(*M.weld(tri)), tri, "unindex(weld(tri))")
    vertices, _, faces = indexed_np(ball(), 0.5)
    same_bits(M.unindex(vertices, faces.astype(np.uint32)), tri, "unindex")
    with pytest.raises(ValueError):
        M.unindex(vertices.reshape(-1), faces)
    # triangles: the results of before, bit for bit; vertices: the same map
    tex = M.to_texture(tri, (12, 12, 12))
    assert tex.dtype == np.float32 and np.array_equal(tex, (tri + np.float32(0.5)) / np.float32(12))
    vtex = M.to_texture(vertices, (12, 12, 12))
    assert vtex.shape == vertices.shape and vtex.dtype == np.float32
    same_bits(vtex[faces], tex, "to_texture of vertices")
    from vkvolume_amd import camera
    xf = camera.image_transform((1.0, 2.0, 0.5), (12, 12, 12))
    model = M.to_model(tri, (12, 12, 12), xf)
    local = tex.astype(np.float64) - 0.5
    m = np.asarray(xf, np.float64).reshape(4, 4)
    same_bits(model, (local @ m[:3, :3] + m[3, :3]).astype(np.float32), "to_model of triangles, as before")
    assert np.allclose(M.to_model(vertices, (12, 12, 12), xf)[faces], model, rtol=0, atol=1e-5)        # another matmul shape: not pinned to the bit
    with pytest.raises(ValueError):
        M.to_texture(np.zeros((4, 2), np.float32), (12, 12, 12))


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch_memory(tmp_path):
    kernels = T.kernel_listing("mesh_indexed.hip", tmp_path / "mesh_indexed.s")
    for name in ("k_meshi_count", "k_meshi_emit_vertices", "k_meshi_emit_indices"):
        assert len([k for k in kernels if name in k]) == 2, sorted(kernels)        # WIDE, narrow
    assert len([k for k in kernels if "k_meshi_scan" in k]) == 2, sorted(kernels)
    assert len(kernels) == 8
    for k, v in kernels.items():
        assert v.get("ScratchSize") == 0, (k, v)
