"""The definition of vkv_label_mesh (include/vkvolume_amd.h, DESIGN.md §5.22: marching tetrahedra on the Kuhn decomposition, every tetrahedron
cut once per visible label it touches) restated twice in numpy, and what can be shown of it without a GPU: the two statements agree to the
bit, the labels of the 14-components give the isosurface mesh's own triangles, every label's subset of a zero-bordered array is a closed,
oriented surface of positive volume, hiding one label leaves the others' triangles alone, a cube gives at most 24 triangles, the entry points
are declared, exported and bound, the kernels of label_mesh.hip use no scratch memory, and vkvolume_amd.mesh splits, measures and colours
what it is given.  tests/test_gpu_label_mesh.py holds the kernels to label_mesh_np() bit for bit.

No context exists without a device, so of the rejections only the null context and the scratch sizes can be asked here; the GPU file asks
every rejection of the header with a live context and pre-filled buffers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers as T
from tests.test_components_cpu import components_np
from tests.test_labels_render_cpu import visibility_map_np, visible_np
from tests.test_mesh_cpu import (KINV255, TETS, _crop, ball, case_table, closed_and_oriented, mesh_contents, mesh_np, same_bits, signed_volume,
                                 tet_triangles, torus)
from vkvolume_amd import abi, labels as LB, lib, mesh as M, volume as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF = np.float32(0.5)


def shown_np(labels, colors):
    """the labels with the hidden ones replaced by 0; colors None: every label is visible"""
    labels = np.ascontiguousarray(labels, np.uint32)
    if colors is None:
        return labels.astype(np.int64)
    return np.where(visible_np(colors, labels.astype(np.int64)), labels, 0).astype(np.int64)


def label_mesh_np(labels_dhw, colors=None, vol_dhw=None, iso=None, box=None, origin=(0, 0, 0)):
    """vectorised statement: (triangles [n, 3, 3] float32, labels [n] uint32), all cubes at once, then sorted into the defined order.
    labels_dhw has the box's shape; vol_dhw (None: midpoints) the volume's; box = (x0, y0, z0, w, h, d); origin: where voxel (0, 0, 0) of
    vol_dhw lies in the volume whose coordinates the vertices carry (vol_dhw is a window cut from it)"""
    E = shown_np(labels_dhw, colors)
    d, h, w = E.shape
    origin = tuple(int(a) + int(b) for a, b in zip((0, 0, 0) if box is None else box[:3], origin))
    f = None
    if vol_dhw is not None:
        vol, _ = _crop(vol_dhw, box)
        assert vol.shape == E.shape
        iso = np.float32(iso)
        f = vol.astype(np.float32) * KINV255
    if min(d, h, w) < 2:
        return np.zeros((0, 3, 3), np.float32), np.zeros((0,), np.uint32)
    corner = lambda a, j: a[(j >> 2):d - 1 + (j >> 2), (j >> 1 & 1):h - 1 + (j >> 1 & 1), (j & 1):w - 1 + (j & 1)]  # noqa: E731
    table = case_table()
    keys, tris, labs = [], [], []
    for t in range(6):
        l = [corner(E, TETS[t][i]) for i in range(4)]
        for g in range(4):
            starts = l[g] != 0
            for k in range(g):
                starts = starts & (l[k] != l[g])
            sub = sum((l[i] == l[g]).astype(np.int64) << i for i in range(4))
            for m in range(1, 15):
                _, edges = table[t, m]
                z, y, x = np.nonzero(starts & (sub == m))
                if len(z) == 0:
                    continue
                cube = (z * (h - 1) + y) * (w - 1) + x
                for k in range(len(edges) // 3):
                    out = np.empty((len(z), 3, 3), np.float32)
                    for v in range(3):
                        a, b = edges[3 * k + v]
                        pa = [x + (a & 1), y + (a >> 1 & 1), z + (a >> 2)]
                        pb = [x + (b & 1), y + (b >> 1 & 1), z + (b >> 2)]
                        tt = np.full(len(z), HALF, np.float32)
                        if f is not None:
                            fa, fb = f[pa[2], pa[1], pa[0]], f[pb[2], pb[1], pb[0]]
                            with np.errstate(all="ignore"):
                                tt = np.where((fa >= iso) != (fb >= iso), (iso - fa) / (fb - fa), HALF)
                        assert tt.dtype == np.float32
                        for c in range(3):
                            ac = (pa[c] + origin[c]).astype(np.float32)
                            out[:, v, c] = ac + tt if (a ^ b) >> c & 1 else ac
                    keys.append((((cube * 6 + t) * 4 + g) * 2) + k)
                    tris.append(out)
                    labs.append(l[g][z, y, x].astype(np.uint32))
    if not keys:
        return np.zeros((0, 3, 3), np.float32), np.zeros((0,), np.uint32)
    keys, tris, labs = np.concatenate(keys), np.concatenate(tris), np.concatenate(labs)
    order = np.argsort(keys, kind="stable")
    assert len(np.unique(keys)) == len(keys)
    return np.ascontiguousarray(tris[order]), np.ascontiguousarray(labs[order])


def label_mesh_loop(labels_dhw, colors=None, vol_dhw=None, iso=None, box=None):
    """plain statement: cube by cube, tetrahedron by tetrahedron, group by group, straight from the definition's sentences (no table)"""
    labels = np.ascontiguousarray(labels_dhw, np.uint32)
    colors = None if colors is None else np.asarray(colors, np.uint32)
    d, h, w = labels.shape
    origin = (0, 0, 0) if box is None else tuple(box[:3])
    vol = None
    if vol_dhw is not None:
        vol, _ = _crop(vol_dhw, box)
        iso = np.float32(iso)
    value = lambda p: np.float32(vol[p[2], p[1], p[0]]) * KINV255  # noqa: E731

    def visible(L):
        if colors is None:
            return L != 0
        return 1 <= L <= len(colors) and (int(colors[L - 1]) >> 24) != 0

    tris, labs = [], []
    for z in range(d - 1):
        for y in range(h - 1):
            for x in range(w - 1):
                for t in range(6):
                    pos = [(x + (j & 1), y + (j >> 1 & 1), z + (j >> 2)) for j in TETS[t]]
                    carried = [int(labels[p[2], p[1], p[0]]) for p in pos]
                    for g in range(4):
                        L = carried[g]
                        if not visible(L) or L in carried[:g]:
                            continue
                        m = sum(1 << i for i in range(4) if carried[i] == L)
                        for tri in tet_triangles(t, m):
                            verts = []
                            for i, j in tri:
                                a, b = pos[min(i, j)], pos[max(i, j)]
                                tt = HALF
                                if vol is not None:
                                    fa, fb = value(a), value(b)
                                    if (fa >= iso) != (fb >= iso):
                                        tt = (iso - fa) / (fb - fa)
                                verts.append([np.float32(a[c] + origin[c]) + tt if b[c] != a[c] else np.float32(a[c] + origin[c]) for c in range(3)])
                            tris.append(verts)
                            labs.append(L)
    return np.array(tris, np.float32).reshape(-1, 3, 3), np.array(labs, np.uint32)


def same_mesh(got, want, what=""):
    same_bits(got[0], want[0], what)
    assert np.array_equal(np.asarray(got[1], np.uint32), np.asarray(want[1], np.uint32)), "%s: the triangle labels differ" % what


# ---- the contents of both test files ---------------------------------------------------------------------------------------------------
def random_labels(shape_dhw, seed, top=3):
    return np.random.default_rng(seed).integers(0, top + 1, size=shape_dhw, dtype=np.uint32)


def distinct_labels(shape_dhw):
    """every voxel its own label: 1 + its linear index"""
    return (np.arange(int(np.prod(shape_dhw)), dtype=np.uint32) + 1).reshape(shape_dhw)


def bordered(labels):
    out = np.zeros(tuple(s + 2 for s in labels.shape), np.uint32)
    out[1:-1, 1:-1, 1:-1] = labels
    return out


def half_balls(n=14, radius=5.0):
    """a ball cut by the plane x = centre into the bodies 1 and 2, inside a zero border"""
    z, y, x = np.indices((n, n, n)).astype(np.float64)
    c = (n - 1) / 2
    inside = (x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2 <= radius ** 2
    return np.where(inside, np.where(x < c, 1, 2), 0).astype(np.uint32)


# the skipping scene of tests/test_gpu_label_mesh.py: 300 x 9 x 20 voxels, bodies only where x < 90, so the second x segment of tiles is empty
SKIP_SHAPE = (20, 9, 300)        # (depth, height, width)
SKIP_COLORS = LB.color_table(5, seed=3, hidden=(2,))


def skip_labels():
    labels = np.zeros(SKIP_SHAPE, np.uint32)
    labels[2:18, 1:8, 3:90] = np.random.default_rng(31).integers(0, 7, size=(16, 7, 87), dtype=np.uint32)        # 6: past the table
    labels[:, :, 200:300][np.random.default_rng(32).random((20, 9, 100)) < 0.05] = 2        # hidden salt in the second segment
    return labels


ROUNDS_ROWS = ((0, 0), (3, 1000), (512, 513), (1023, 0), (1025, 1025))        # (z, y), rising in the output's order


def rounds_labels():
    """2 x 1026 x 1026, the case of tests/test_gpu_label_mesh.py whose 1025 x 1025 entries are 257 scan chunks: five labelled rows far
    apart, three labels"""
    w, h, d = 2, 1026, 1026
    labels = np.zeros((d, h, w), np.uint32)
    for k, (z, y) in enumerate(ROUNDS_ROWS):
        labels[z, y, :] = 1 + k % 3
    return labels


def test_the_statement_on_the_sparse_rounds_case_is_the_rows_own_meshes_in_order():
    """label_mesh_np takes a few seconds on the million cubes of rounds_labels(); its list is, row by row, the mesh of the 3 x 3 rows around
    each labelled row as a box of its own"""
    labels = rounds_labels()
    tri, lab = label_mesh_np(labels)
    parts = []
    for z, y in ROUNDS_ROWS:
        z0, y0 = max(z - 1, 0), max(y - 1, 0)
        z1, y1 = min(z + 2, labels.shape[0]), min(y + 2, labels.shape[1])
        parts.append(label_mesh_np(labels[z0:z1, y0:y1, :], box=(0, y0, z0, 2, y1 - y0, z1 - z0)))
        assert len(parts[-1][0]) > 0
    same_mesh((tri, lab), (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])), "rounds case")


def empty_tiles(vis_map, shape_dhw, box, map_extent):
    """the tiles of 256 x 4 x 16 cubes of the box all of whose cube origins lie in cells that hold 0 (the kernels' test), of how many"""
    D, H, W = shape_dhw
    x0, y0, z0, bw, bh, bd = (0, 0, 0, W, H, D) if box is None else box
    mw, mh, md = map_extent
    bx, by, bz = -(-W // mw), -(-H // mh), -(-D // md)
    nx, ny, nz = bw - 1, bh - 1, bd - 1
    empty = total = 0
    for zt in range(0, nz, 16):
        for yt in range(0, ny, 4):
            for xt in range(0, nx, 256):
                cells = vis_map[(z0 + zt) // bz:(z0 + min(zt + 16, nz) - 1) // bz + 1, (y0 + yt) // by:(y0 + min(yt + 4, ny) - 1) // by + 1,
                                (x0 + xt) // bx:(x0 + min(xt + 256, nx) - 1) // bx + 1]
                total += 1
                empty += int(not cells.any())
    return empty, total


# ---- the two statements ------------------------------------------------------------------------------------------------------------------
SHAPES = [(4, 5, 6), (1, 5, 6), (5, 1, 6), (5, 6, 1), (2, 2, 2), (3, 2, 5), (1, 1, 1)]  # (depth, height, width)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_the_two_statements_agree_to_the_bit(shape):
    vol = np.random.default_rng(40).integers(0, 256, size=shape, dtype=np.uint8)
    for seed, colors in ((0, None), (1, LB.color_table(3, hidden=(2,))), (2, LB.color_table(2)), (3, LB.color_table(3, hidden=(1, 3)))):
        labels = random_labels(shape, seed)
        assert colors is None or len(colors) < 3 or (labels == 2).any() or labels.size < 8
        for v, iso in ((None, None), (vol, 0.5)):
            a, b = label_mesh_np(labels, colors, v, iso), label_mesh_loop(labels, colors, v, iso)
            same_mesh(a, b, "%s seed %d" % (shape, seed))
            if min(shape) < 2:
                assert len(a[0]) == 0
            shown = set(np.unique(shown_np(labels, colors))) - {0}
            assert set(a[1].tolist()) <= shown
    box = (1, 1, 0, shape[2] - 1, shape[1] - 1, shape[0]) if min(shape[1:]) > 1 else None
    if box is not None:
        big = np.random.default_rng(41).integers(0, 256, size=shape, dtype=np.uint8)
        labels = random_labels((box[5], box[4], box[3]), 5)
        same_mesh(label_mesh_np(labels, None, big, 0.4, box), label_mesh_loop(labels, None, big, 0.4, box), "%s box" % (shape,))


def test_labels_above_the_table_and_hidden_labels_are_outside():
    labels = random_labels((4, 5, 6), 9, top=5)
    colors = LB.color_table(3, hidden=(2,))        # 4 and 5 are past the table, 2 is switched off
    a = label_mesh_np(labels, colors)
    same_mesh(a, label_mesh_loop(labels, colors), "table of 3")
    assert set(a[1].tolist()) == {1, 3}
    zeroed = np.where(np.isin(labels, (1, 3)), labels, 0).astype(np.uint32)
    same_mesh(a, label_mesh_np(zeroed, None), "hidden labels are label 0")


# ---- 14-components: the isosurface mesh itself -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", ["random", "ball", "torus"])
def test_the_labels_of_the_14_components_give_the_isosurface_mesh_bit_for_bit(content):
    vol = {"random": lambda: mesh_contents("random", (6, 7, 9), 17), "ball": ball, "torus": torus}[content]()
    d, h, w = vol.shape
    cases = [(0.5, None), (0.3, None), (0.5, (1, 2, 1, w - 2, h - 3, d - 1))] + ([(0.85, None)] if content == "random" else [])        # 0.85: random bytes fall apart
    for iso, box in cases:
        labels = components_np(vol, iso, 14, box)[0]
        tri, lab = label_mesh_np(labels, None, vol, iso, box)
        same_bits(tri, mesh_np(vol, iso, box), "%s iso %g box %s" % (content, iso, box))
        assert len(tri) > 0 and lab.min() >= 1 and lab.max() <= labels.max()
    if content == "random":
        assert labels.max() > 3 and len(np.unique(lab)) > 3        # the labels split the mesh by body


# ---- watertight per label ----------------------------------------------------------------------------------------------------------------
def each_label_is_closed(tri, lab):
    names, starts, parts = M.split_by_label(tri, lab)
    for k, L in enumerate(names):
        part = parts[starts[k]:starts[k + 1]]
        closed_and_oriented(part)
        assert signed_volume(part) > 0, L
    return names


def test_two_half_balls_are_each_closed_and_share_their_interface():
    labels = half_balls()
    tri, lab = label_mesh_np(labels)
    assert each_label_is_closed(tri, lab).tolist() == [1, 2]
    # the interface: the vertices both bodies use are bit-equal, and there are many of them
    key = lambda part: set(map(bytes, np.ascontiguousarray(part.reshape(-1, 3)).view(np.uint8).reshape(-1, 12)))  # noqa: E731
    shared = key(tri[lab == 1]) & key(tri[lab == 2])
    assert len(shared) > 50
    # each body is the midpoint surface of its own indicator: it encloses what the tetrahedra hold of it, counted without any triangle.  (The
    # bodies do not tile the ball: a tetrahedron with the labels 1, 2, 0, 0 gives each body a corner of 1 / 8 and the ball as one body a half.)
    for L in (1, 2):
        assert abs(signed_volume(tri[lab == L]) - tet_volume_np(labels == L)) < 1e-9
    one = label_mesh_np((labels != 0).astype(np.uint32))[0]
    assert 0 <= signed_volume(one) - signed_volume(tri) < 0.02 * signed_volume(one)
    # with the volume, where label != 0 is exactly "inside", the outer surface has the isosurface's own vertices
    vol = np.where(labels != 0, 200, 30).astype(np.uint8)
    tri_v, lab_v = label_mesh_np(labels, None, vol, 0.5)
    each_label_is_closed(tri_v, lab_v)
    assert key(mesh_np(vol, 0.5)) <= key(tri_v)


def test_random_labels_inside_a_zero_border_are_closed_per_label():
    labels = bordered(random_labels((4, 5, 6), 21))
    tri, lab = label_mesh_np(labels)
    assert each_label_is_closed(tri, lab).tolist() == [1, 2, 3]
    vol = np.random.default_rng(22).integers(0, 256, size=labels.shape, dtype=np.uint8)
    tri, lab = label_mesh_np(labels, None, vol, 0.5)        # interpolated where the volume happens to cross: still shared, still closed
    each_label_is_closed(tri, lab)


def test_hiding_a_label_leaves_the_others_triangles_unchanged():
    labels = bordered(random_labels((4, 5, 6), 23))
    tri, lab = label_mesh_np(labels, LB.color_table(3))
    for hidden in (1, 2, 3):
        tri_h, lab_h = label_mesh_np(labels, LB.color_table(3, hidden=(hidden,)))
        same_mesh((tri_h, lab_h), (tri[lab != hidden], lab[lab != hidden]), "label %d hidden" % hidden)


def test_distinct_labels_reach_24_triangles_in_a_cube_and_never_more():
    for shape in ((2, 2, 2), (3, 4, 5)):
        labels = distinct_labels(shape)
        tri, lab = label_mesh_np(labels)
        cubes = (shape[0] - 1) * (shape[1] - 1) * (shape[2] - 1)
        assert len(tri) == 24 * cubes
        same_mesh((tri, lab), label_mesh_loop(labels), "distinct")
    for seed in range(4):
        labels = random_labels((3, 3, 3), 50 + seed, top=8)
        tri, _ = label_mesh_np(labels)
        per_cube = [len(label_mesh_np(labels[z:z + 2, y:y + 2, x:x + 2])[0]) for z in range(2) for y in range(2) for x in range(2)]
        assert max(per_cube) <= 24 and sum(per_cube) == len(tri)


def test_the_skipping_scene_empties_whole_tiles():
    labels = skip_labels()
    d, h, w = SKIP_SHAPE
    for block in (1, 4):
        me = ((w + block - 1) // block, (h + block - 1) // block, (d + block - 1) // block)
        vis = visibility_map_np(labels, None, SKIP_SHAPE, SKIP_COLORS, me)
        empty, total = empty_tiles(vis, SKIP_SHAPE, None, me)
        assert total == 2 * 2 * 2 and empty >= 4, (block, empty, total)        # the second x segment holds hidden salt only
    tri, lab = label_mesh_np(labels, SKIP_COLORS)
    assert len(tri) > 1000 and set(lab.tolist()) == {1, 3, 4, 5}
    assert tri[:, :, 0].max() < 100


# ---- entry points --------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    assert re.search(r"\bsize_t\s+vkv_label_mesh_scratch_bytes\s*\(\s*VkvExtent3D extent,\s*const VkvBox\s*\*box\)", header)
    assert re.search(r"\bint\s+vkv_label_mesh\s*\(\s*vkv_ctx\s*\*ctx,\s*const uint32_t\s*\*d_labels,\s*VkvExtent3D extent,\s*const VkvBox\s*\*box,\s*"
                     r"const uint32_t\s*\*d_colors,\s*uint64_t table_entries,\s*const uint8_t\s*\*d_volume,\s*float iso,\s*"
                     r"const uint8_t\s*\*d_visibility_map,\s*VkvExtent3D map_extent,\s*void\s*\*d_scratch,\s*float\s*\*d_triangles,\s*"
                     r"uint32_t\s*\*d_triangle_labels,\s*uint64_t capacity_triangles,\s*uint64_t\s*\*d_counts,\s*void\s*\*stream\)", header)
    assert "every non-zero label is visible" in header
    L = lib.load()
    assert {"vkv_label_mesh", "vkv_label_mesh_scratch_bytes"} <= set(lib.EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    assert re.search(r"\bvkv_label_mesh$", out, flags=re.M) and re.search(r"\bvkv_label_mesh_scratch_bytes$", out, flags=re.M)
    at = L.vkv_label_mesh.argtypes
    assert len(at) == 16 and at[2] is abi.Extent3D and at[3] is C.POINTER(abi.Box) and at[5] is C.c_uint64 and at[7] is C.c_float
    assert at[9] is abi.Extent3D and at[13] is C.c_uint64
    assert callable(lib.Context.label_mesh_rc) and callable(V.Volume.extract_label_mesh) and callable(LB.mesh_scratch_bytes)


def test_scratch_bytes_and_the_null_context_without_a_device():
    L = lib.load()
    e = abi.Extent3D(258, 5, 19)
    assert LB.mesh_scratch_bytes(e) >= 16 and LB.mesh_scratch_bytes(e) % 8 == 0
    assert LB.mesh_scratch_bytes(e) == lib.mesh_scratch_bytes(e)        # the mesh's plan and layout
    assert LB.mesh_scratch_bytes(abi.Extent3D(1, 5, 19)) >= 16 and LB.mesh_scratch_bytes(abi.Extent3D(1, 1, 1)) >= 16        # no cubes, still a buffer
    for ext in ((3, 2, 66), (2, 66, 65), (300, 9, 20)):
        assert LB.mesh_scratch_bytes(abi.Extent3D(*ext)) % 8 == 0
    assert LB.mesh_scratch_bytes(e, abi.Box(1, 1, 1, 2, 2, 2)) <= LB.mesh_scratch_bytes(e)
    assert LB.mesh_scratch_bytes(abi.Extent3D(0, 5, 19)) == 0
    assert LB.mesh_scratch_bytes(e, abi.Box(257, 0, 0, 2, 1, 1)) == 0 and LB.mesh_scratch_bytes(e, abi.Box(0, 0, 0, 0, 1, 1)) == 0
    assert LB.mesh_scratch_bytes(abi.Extent3D(0x80000000, 2, 2)) == 0
    assert LB.mesh_scratch_bytes(abi.Extent3D(2048, 2048, 1024)) == 0        # 2^32 voxels: one more than the labels' calls take
    assert LB.mesh_scratch_bytes(abi.Extent3D(2048, 2048, 1024), abi.Box(0, 0, 0, 2048, 2048, 1023)) > 0
    buf = (C.c_uint64 * 64)()
    a = C.addressof(buf)
    none = abi.Extent3D(0, 0, 0)
    assert L.vkv_label_mesh(None, a, abi.Extent3D(4, 4, 4), None, None, 0, None, 0.5, None, none, a + 64, None, None, 0, a + 256, None) == abi.VKV_E_INVALID_ARGUMENT


def test_kernels_use_no_scratch_memory(tmp_path):
    kernels = T.kernel_listing("label_mesh.hip", tmp_path / "label_mesh.s")
    assert len([k for k in kernels if "k_lmesh_count" in k]) == 2 and len([k for k in kernels if "k_lmesh_emit" in k]) == 2, sorted(kernels)  # WIDE, narrow
    assert len([k for k in kernels if "k_lmesh_scan" in k]) == 2, sorted(kernels)
    for k, v in kernels.items():
        print(k, v)
        assert v.get("ScratchSize") == 0, (k, v)
        assert v.get("NumVgprs") <= 128, (k, v)        # two waves per SIMD at the least


# ---- vkvolume_amd.mesh -------------------------------------------------------------------------------------------------------------------
def test_split_by_label_is_a_stable_sort_into_slices():
    labels = bordered(random_labels((4, 5, 6), 21))
    tri, lab = label_mesh_np(labels)
    names, starts, parts = M.split_by_label(tri, lab)
    assert names.tolist() == [1, 2, 3] and starts[0] == 0 and starts[-1] == len(tri) and len(starts) == 4
    for k, L in enumerate(names):
        same_bits(parts[starts[k]:starts[k + 1]], tri[lab == L], "label %d" % L)        # the extraction's order within a body
    names, starts, parts = M.split_by_label(np.zeros((0, 3, 3), np.float32), np.zeros((0,), np.uint32))
    assert len(names) == 0 and starts.tolist() == [0] and parts.shape == (0, 3, 3)
    with pytest.raises(ValueError):
        M.split_by_label(tri, lab[:-1])


def tet_volume_np(inside):
    """the volume the midpoint surface of an indicator encloses, counted tetrahedron by tetrahedron and not from any triangle: a
    tetrahedron (volume 1/6) with 4, 3, 2, 1 inside vertices holds 1, 7/8, 1/2, 1/8 of itself (the corner cut off at the midpoints of
    three edges is 1/8 of the tetrahedron; two and two split it in halves by symmetry)"""
    d, h, w = inside.shape
    corner = lambda j: inside[(j >> 2):d - 1 + (j >> 2), (j >> 1 & 1):h - 1 + (j >> 1 & 1), (j & 1):w - 1 + (j & 1)].astype(np.int64)  # noqa: E731
    share = np.array([0, 1 / 8, 1 / 2, 7 / 8, 1], np.float64)
    return float(sum(share[sum(corner(TETS[t][i]) for i in range(4))].sum() for t in range(6)) / 6.0)


def test_body_measures_of_a_cube_and_a_ball():
    # a 0/255 cube: two boxes of voxels, labels 1 and 3, in a zero border; label 2 has no voxel
    labels = np.zeros((9, 10, 12), np.uint32)
    labels[2:6, 2:7, 2:5] = 1
    labels[2:7, 3:6, 7:10] = 3
    vol = np.where(labels != 0, 255, 0).astype(np.uint8)
    for v, iso in ((None, None), (vol, 0.5)):        # 0/255 at iso 0.5 gives t = 0.5 too, by interpolation
        tri, lab = label_mesh_np(labels, None, v, iso)
        area, volume = M.body_measures(tri, lab, 3)
        assert area.dtype == np.float64 and volume.dtype == np.float64 and area.shape == (3,) and volume.shape == (3,)
        assert abs(volume[0] - tet_volume_np(labels == 1)) < 1e-9 and abs(volume[2] - tet_volume_np(labels == 3)) < 1e-9
        assert volume[1] == 0 and area[1] == 0
        # between the boxes of voxel centres and of voxels grown by half a voxel
        assert 3 * 4 * 2 < volume[0] < 4 * 5 * 3 and 2 * (3 * 4 + 3 * 2 + 4 * 2) < area[0] < 2 * (4 * 5 + 4 * 3 + 5 * 3)
    assert np.array_equal(M.body_measures(tri, lab, 1)[1], volume[:1])        # labels above n_labels are ignored
    # a ball of radius r = 8 in a smooth volume, (r - dist) * 60 + 128 clipped, cut at iso 0.5 (byte 127.5: r + 0.5 / 60).  On every crossing
    # edge (length h <= sqrt 3) the field is not clipped (128 / 60 > sqrt 3) and is linear in the distance, which along a chord of a sphere
    # sags by at most h^2 / (8 r) = 0.047 voxels = 0.6 % of r: at most 1.8 % of the volume and 1.2 % of the area; a facet tilted against
    # the sphere by h / (2 r) shrinks the area by another 0.6 %.  The bound asked is 3 % for both.
    r = 8.0
    vol = ball(n=20, centre=9.5, radius=r)
    labels = components_np(vol, 0.5, 14)[0]
    assert labels.max() == 1
    tri, lab = label_mesh_np(labels, None, vol, 0.5)
    area, volume = M.body_measures(tri, lab, 1)
    rr = r + 0.5 / 60
    assert abs(volume[0] - 4 / 3 * np.pi * rr ** 3) < 0.03 * 4 / 3 * np.pi * rr ** 3, volume
    assert abs(area[0] - 4 * np.pi * rr ** 2) < 0.03 * 4 * np.pi * rr ** 2, area
    assert abs(volume[0] - signed_volume(tri)) < 1e-9


def read_ply(path):
    data = open(path, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in lines if l.startswith("element face")][0].split()[-1])
    coloured = "property uchar red" in lines
    vertices = np.frombuffer(body, "<f4", nv * 3).reshape(nv, 3)
    fields = [("n", "u1"), ("v", "<u4", 3)] + ([("c", "u1", 3)] if coloured else [])
    rec = np.frombuffer(body, np.dtype(fields), nf, offset=nv * 12)
    assert len(body) == nv * 12 + nf * np.dtype(fields).itemsize and (rec["n"] == 3).all()
    return lines, vertices, rec["v"], rec["c"] if coloured else None


def test_coloured_ply_round_trips_and_the_plain_file_keeps_its_bytes(tmp_path):
    labels = bordered(random_labels((4, 5, 6), 21))
    tri, lab = label_mesh_np(labels)
    vertices, faces = M.weld(tri)
    table = LB.color_table(2, seed=5)        # label 3 is past the table: black
    colors = M.label_face_colors(lab, table)
    assert colors.dtype == np.uint8 and colors.shape == (len(tri), 3)
    assert (colors[lab == 3] == 0).all() and (colors[lab == 1] == [table[0] & 255, table[0] >> 8 & 255, table[0] >> 16 & 255]).all()
    assert (colors[lab != 3] >= 64).all()
    path = tmp_path / "bodies.ply"
    M.write_ply(str(path), vertices, faces, face_colors=colors)
    lines, v, f, c = read_ply(str(path))
    assert lines[-4:-1] == ["property uchar red", "property uchar green", "property uchar blue"]
    same_bits(v[f.astype(np.int64)], tri, "ply")
    assert np.array_equal(c, colors)
    # without face_colors: the file of before, byte for byte
    plain = tmp_path / "plain.ply"
    M.write_ply(str(plain), vertices, faces)
    want = ("ply\nformat binary_little_endian 1.0\ncomment vkvolume_amd isosurface\nelement vertex %d\nproperty float x\nproperty float y\n"
            "property float z\nelement face %d\nproperty list uchar uint vertex_indices\nend_header\n" % (len(vertices), len(faces))).encode("ascii")
    rec = np.zeros(len(faces), np.dtype([("n", "u1"), ("v", "<u4", 3)]))
    rec["n"], rec["v"] = 3, faces
    assert open(str(plain), "rb").read() == want + vertices.astype("<f4").tobytes() + rec.tobytes()
    with pytest.raises(ValueError):
        M.write_ply(str(path), vertices, faces, face_colors=colors[:-1])
