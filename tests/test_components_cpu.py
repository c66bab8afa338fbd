"""The definitions of vkv_label_components and vkv_select_components (include/vkvolume_amd.h) restated in numpy,
components_np() and select_np(), and what can be shown of them without a GPU: components_np() is scipy.ndimage.label with the matching
structure on random small volumes for all three neighbourhoods (partition AND numbering), contents on which the three neighbourhoods must
differ do differ, the 14 offsets are exactly the tetrahedron edges of mtet_table.hpp, the entry points are declared, exported and bound,
the scratch formula is the header's, and the kernels of components.hip use no scratch memory.  tests/test_gpu_components.py holds the kernels
to components_np() and select_np() bit for bit."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers as T
from tests.test_mesh_cpu import KINV255
from vkvolume_amd import abi, lib, volume as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the header's three neighbourhoods as (dx, dy, dz)
_ALL = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]
OFFSETS = {
    6: [o for o in _ALL if sum(map(abs, o)) == 1],
    14: [o for o in _ALL if all(c >= 0 for c in o) or all(c <= 0 for c in o)],
    26: _ALL,
}
TETS = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))        # T0 .. T5 of the header, corner j = dx + 2 dy + 4 dz


def inside_np(vol_dhw, iso, box=None):
    """the inside voxels of the box (x0, y0, z0, w, h, d): (float) byte * kInv255 >= iso in fp32"""
    whole = np.ascontiguousarray(vol_dhw, np.uint8)
    x0, y0, z0, w, h, d = (0, 0, 0) + whole.shape[::-1] if box is None else box
    return whole[z0:z0 + d, y0:y0 + h, x0:x0 + w].astype(np.float32) * KINV255 >= np.float32(iso)


def components_np(vol_dhw, iso, connectivity=6, box=None, capacity=None):
    """(labels [d, h, w] uint32, sizes [min(K, capacity)] uint32, counts [3] uint64) of the header's sentences: every inside voxel starts with
    its own box-linear index as its label; a voxel, and the voxel that its label names, take the minimum over the labels of its inside
    neighbours (the stated offsets, inside the box only), and every voxel its label's label, until nothing changes: a component ends with
    the index of its first voxel; components are then ranked by that index."""
    inside = inside_np(vol_dhw, iso, box)
    d, h, w = inside.shape
    n = inside.size
    index = np.arange(n, dtype=np.int64).reshape(inside.shape)
    flat = np.append(np.where(inside, index, n).reshape(-1), n)        # flat[n]: the outside's label
    while True:
        before = flat.copy()
        lab = before[:n].reshape(inside.shape)
        for dx, dy, dz in OFFSETS[connectivity]:
            dst = (slice(max(-dz, 0), d - max(dz, 0)), slice(max(-dy, 0), h - max(dy, 0)), slice(max(-dx, 0), w - max(dx, 0)))
            src = (slice(max(dz, 0), d - max(-dz, 0)), slice(max(dy, 0), h - max(-dy, 0)), slice(max(dx, 0), w - max(-dx, 0)))
            pair = inside[dst] & inside[src]
            mine, theirs = lab[dst][pair], lab[src][pair]
            # a voxel takes its neighbour's label, and so does the voxel whose index its own label is (a voxel of the same component)
            np.minimum.at(flat, mine, theirs)
            np.minimum.at(flat, index[dst][pair], theirs)
        while True:        # a label is a voxel of the same component: take that voxel's label where it is smaller
            jumped = np.minimum(flat, flat[flat])
            if np.array_equal(jumped, flat):
                break
            flat = jumped
        if np.array_equal(flat, before):
            break
    lab = flat[:n].reshape(inside.shape)
    firsts = np.unique(lab[inside])
    assert np.array_equal(lab.reshape(-1)[firsts], firsts)        # every component carries the index of a voxel of its own: the first
    labels = np.zeros(inside.shape, np.uint32)
    labels[inside] = np.searchsorted(firsts, lab[inside]) + 1
    k = len(firsts)
    sizes = np.bincount(labels[inside], minlength=k + 1)[1:].astype(np.uint32)
    written = k if capacity is None else min(k, capacity)
    return labels, sizes[:written], np.array([k, written, int(inside.sum())], np.uint64)


def select_np(src_dhw, labels, sizes, written, min_voxels, max_voxels, fill, box=None, dst=None):
    """vkv_select_components: `dst` (None: a copy of src) with the box's voxels written"""
    src = np.ascontiguousarray(src_dhw, np.uint8)
    out = src.copy() if dst is None else dst.copy()
    x0, y0, z0, w, h, d = (0, 0, 0) + src.shape[::-1] if box is None else box
    assert labels.shape == (d, h, w)
    sub = src[z0:z0 + d, y0:y0 + h, x0:x0 + w].copy()
    known = (labels != 0) & (labels <= written)
    size = np.zeros(labels.shape, np.uint64)
    size[known] = np.asarray(sizes, np.uint64)[labels[known].astype(np.int64) - 1]
    sub[known & ((size < min_voxels) | (size > max_voxels))] = fill
    out[z0:z0 + d, y0:y0 + h, x0:x0 + w] = sub
    return out


def structure_of(connectivity):
    s = np.zeros((3, 3, 3), bool)
    s[1, 1, 1] = True
    for dx, dy, dz in OFFSETS[connectivity]:
        s[dz + 1, dy + 1, dx + 1] = True
    return s


# ---- the statement ----------------------------------------------------------------------------------------------------------------------
def test_the_neighbourhoods_have_6_14_and_26_symmetric_offsets():
    for c, offsets in OFFSETS.items():
        assert len(offsets) == c == len(set(offsets)) and all((-dx, -dy, -dz) in offsets for dx, dy, dz in offsets)
    assert set(OFFSETS[6]) < set(OFFSETS[14]) < set(OFFSETS[26])


def test_the_14_offsets_are_the_tetrahedron_edges():
    text = open(os.path.join(ROOT, "vkvolume_amd", "csrc", "mtet_table.hpp")).read()
    m = re.search(r"kMtetCorners\[6\]\[4\]\s*=\s*\{(.*?)\};", text)
    assert tuple(tuple(int(c) for c in t.split(",")) for t in re.findall(r"\{([^{}]*)\}", m.group(1))) == TETS
    corner = lambda j: np.array([j & 1, j >> 1 & 1, j >> 2])  # noqa: E731
    edges = set()
    for t in TETS:
        for a, b in itertools.combinations(t, 2):
            assert a & b == a        # from a corner to one that only adds axes
            diff = corner(b) - corner(a)
            edges |= {tuple(diff), tuple(-diff)}
    assert edges == set(OFFSETS[14])


@pytest.mark.parametrize("connectivity", [6, 14, 26])
def test_components_np_is_scipy_label(connectivity):
    from scipy import ndimage
    rng = np.random.default_rng(connectivity)
    for k in range(40):
        shape = tuple(rng.integers(1, 9, size=3))
        density = (0.1, 0.31, 0.6, 0.9)[k % 4]
        vol = np.where(rng.random(shape) < density, 200, 17).astype(np.uint8)
        want, count = ndimage.label(vol >= 128, structure=structure_of(connectivity))
        labels, sizes, counts = components_np(vol, 0.5, connectivity)
        assert np.array_equal(labels, want.astype(np.uint32)), (shape, density)        # the partition and the numbering
        assert counts.tolist() == [count, count, int((vol >= 128).sum())]
        assert np.array_equal(sizes, np.bincount(want.reshape(-1), minlength=count + 1)[1:])


def test_a_box_is_labelled_as_the_cropped_array():
    from scipy import ndimage
    vol = np.where(np.random.default_rng(5).random((7, 8, 9)) < 0.4, 255, 0).astype(np.uint8)
    box = (2, 1, 3, 5, 6, 3)
    labels, sizes, counts = components_np(vol, 0.5, 26, box)
    want, count = ndimage.label(vol[3:6, 1:7, 2:7] > 0, structure=structure_of(26))
    assert labels.shape == (3, 6, 5) and np.array_equal(labels, want) and counts[0] == count
    assert components_np(vol, 0.5, 26, box, capacity=2)[1].tolist() == sizes[:2].tolist()


def test_the_inside_rule_is_the_meshes():
    vol = np.arange(256, dtype=np.uint8).reshape(1, 1, 256)
    for iso in (0.0, 0.2, 0.5, 128 * float(KINV255), 1.0, 1.5, -1.0):
        thr = next((b for b in range(256) if np.float32(b) * KINV255 >= np.float32(iso)), 256)
        labels, sizes, counts = components_np(vol, iso, 6)
        assert counts.tolist() == [1 if thr < 256 else 0] * 2 + [256 - thr]
        assert np.array_equal(labels[0, 0] != 0, np.arange(256) >= thr)


def test_contents_on_which_the_neighbourhoods_differ():
    z, y, x = np.indices((4, 5, 6))
    board = np.where((x + y + z) % 2 == 0, 255, 0).astype(np.uint8)
    assert components_np(board, 0.5, 6)[2].tolist() == [60, 60, 60] and (components_np(board, 0.5, 6)[1] == 1).all()
    assert components_np(board, 0.5, 14)[2].tolist() == [1, 1, 60]        # (1, 1, 0) joins the even voxels
    assert components_np(board, 0.5, 26)[2].tolist() == [1, 1, 60]
    anti = np.zeros((3, 3, 3), np.uint8)
    anti[1, 2, 0] = anti[1, 1, 1] = 255        # offset (1, -1, 0)
    assert [int(components_np(anti, 0.5, c)[2][0]) for c in (6, 14, 26)] == [2, 2, 1]
    diag = np.zeros((3, 3, 3), np.uint8)
    diag[0, 0, 0] = diag[1, 1, 1] = 255        # offset (1, 1, 1)
    assert [int(components_np(diag, 0.5, c)[2][0]) for c in (6, 14, 26)] == [2, 1, 1]


def test_select_np_keeps_what_it_does_not_know():
    vol = np.zeros((1, 1, 12), np.uint8)
    vol[0, 0, [0, 2, 3, 5, 6, 7, 10]] = 200        # sizes 1, 2, 3, 1
    labels, sizes, counts = components_np(vol, 0.5, 6)
    assert sizes.tolist() == [1, 2, 3, 1]
    assert select_np(vol, labels, sizes, 4, 2, 2 ** 64 - 1, 0)[0, 0].tolist() == [0, 0, 200, 200, 0, 200, 200, 200, 0, 0, 0, 0]
    assert select_np(vol, labels, sizes, 4, 0, 2, 9)[0, 0].tolist() == [200, 0, 200, 200, 0, 9, 9, 9, 0, 0, 200, 0]
    assert select_np(vol, labels, sizes[:2], 2, 2, 2 ** 64 - 1, 0)[0, 0].tolist() == [0, 0, 200, 200, 0, 200, 200, 200, 0, 0, 200, 0]        # 3 and 4 unknown
    assert np.array_equal(select_np(vol, labels, sizes[:0], 0, 5, 5, 0), vol)


# ---- entry points ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    for name, value in (("VKV_CONNECT_6", 6), ("VKV_CONNECT_14", 14), ("VKV_CONNECT_26", 26)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header)
    assert (abi.CONNECT_6, abi.CONNECT_14, abi.CONNECT_26) == (6, 14, 26)
    assert re.search(r"\bsize_t\s+vkv_label_components_scratch_bytes\s*\(\s*VkvExtent3D extent,\s*const VkvBox\s*\*box\)", header)
    assert re.search(r"\bint\s+vkv_label_components\s*\(\s*vkv_ctx\s*\*ctx,\s*const uint8_t\s*\*d_volume,\s*VkvExtent3D extent,\s*const VkvBox\s*\*box,\s*float iso,\s*"
                     r"int32_t connectivity,\s*const uint8_t\s*\*d_max_map,\s*VkvExtent3D map_extent,\s*void\s*\*d_scratch,\s*uint32_t\s*\*d_labels,\s*"
                     r"uint32_t\s*\*d_sizes,\s*uint64_t capacity_components,\s*uint64_t\s*\*d_counts,\s*void\s*\*stream\)", header)
    assert re.search(r"\bint\s+vkv_select_components\s*\(\s*vkv_ctx\s*\*ctx,\s*const uint8_t\s*\*d_src,\s*uint8_t\s*\*d_dst,\s*VkvExtent3D extent,\s*const VkvBox\s*\*box,\s*"
                     r"const uint32_t\s*\*d_labels,\s*const uint32_t\s*\*d_sizes,\s*const uint64_t\s*\*d_counts,\s*uint64_t min_voxels,\s*uint64_t max_voxels,\s*"
                     r"uint32_t fill,\s*void\s*\*stream\)", header)
    L = lib.load()
    names = {"vkv_label_components", "vkv_label_components_scratch_bytes", "vkv_select_components"}
    assert names <= set(lib.EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    assert all(re.search(r"\b%s$" % n, out, flags=re.M) for n in names)
    at = L.vkv_label_components.argtypes
    assert len(at) == 14 and at[2] is abi.Extent3D and at[3] is C.POINTER(abi.Box) and at[4] is C.c_float and at[5] is C.c_int32 and at[7] is abi.Extent3D
    assert at[11] is C.c_uint64
    at = L.vkv_select_components.argtypes
    assert len(at) == 12 and at[3] is abi.Extent3D and at[8] is C.c_uint64 and at[9] is C.c_uint64 and at[10] is C.c_uint32
    assert L.vkv_label_components_scratch_bytes.restype is C.c_size_t
    assert callable(lib.Context.label_components) and callable(lib.Context.label_components_rc)
    assert callable(lib.Context.select_components) and callable(lib.Context.select_components_rc)
    assert callable(lib.components_scratch_bytes) and callable(V.Volume.label_components) and callable(V.Volume.remove_islands)


def test_scratch_bytes_and_bad_arguments_without_a_device():
    L = lib.load()
    for extent in ((1, 1, 1), (64, 1, 1), (65, 1, 1), (258, 5, 19), (2, 66, 65), (1024, 1024, 795)):
        w, h, d = extent
        n = w * h * d
        entries = (n + 63) // 64
        want = 24 * entries + 16 * ((entries + 4095) // 4096)        # the header's formula
        assert lib.components_scratch_bytes(abi.Extent3D(w, h, d)) == want and want % 8 == 0 and want <= n + 64, extent
    e = abi.Extent3D(258, 5, 19)
    assert 40 == lib.components_scratch_bytes(e, abi.Box(1, 1, 1, 2, 2, 2)) < lib.components_scratch_bytes(e)
    assert lib.components_scratch_bytes(abi.Extent3D(0, 5, 19)) == 0
    assert lib.components_scratch_bytes(e, abi.Box(257, 0, 0, 2, 1, 1)) == 0 and lib.components_scratch_bytes(e, abi.Box(0, 0, 0, 0, 1, 1)) == 0
    big = abi.Extent3D(0x10000, 0x10000, 2)        # 2^33 voxels
    assert lib.components_scratch_bytes(big) == 0 and lib.components_scratch_bytes(abi.Extent3D(0xffffffff, 1, 1)) > 0
    assert lib.components_scratch_bytes(abi.Extent3D(0x10000, 0x10000, 1)) == 0        # 2^32: one voxel too many
    assert lib.components_scratch_bytes(big, abi.Box(5, 5, 0, 3, 3, 2)) == 40
    buf = (C.c_uint64 * 128)()
    a = C.addressof(buf)
    none = abi.Extent3D(0, 0, 0)
    bad = abi.VKV_E_INVALID_ARGUMENT
    assert L.vkv_label_components(None, a, abi.Extent3D(4, 4, 4), None, 0.5, 6, None, none, a + 64, a + 512, None, 0, a + 128, None) == bad
    assert L.vkv_select_components(None, a, a, abi.Extent3D(4, 4, 4), None, a + 512, a + 800, a + 128, 0, 10, 0, None) == bad
    assert not any(buf)


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch_memory(tmp_path):
    kernels = T.kernel_listing("components.hip", tmp_path / "components.s")
    assert len([k for k in kernels if "k_cc_merge" in k]) == 3, sorted(kernels)        # one per neighbourhood
    for name in ("k_cc_init", "k_cc_flatten", "k_cc_scan_chunks", "k_cc_scan_total", "k_cc_rank_roots", "k_cc_relabel", "k_cc_select"):
        assert len([k for k in kernels if name in k]) == 1, sorted(kernels)
    assert len(kernels) == 10
    for k, v in kernels.items():
        assert v.get("ScratchSize") == 0, (k, v)
