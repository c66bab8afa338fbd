"""The definitions of vkv_component_stats and vkv_select_components_by_table (include/vkvolume_amd.h) restated in numpy,
component_stats_np() and select_by_table_np(), and what can be shown of them without a GPU: the restatement is scipy.ndimage's find_objects,
sum_labels, minimum, maximum and center_of_mass x count on labels of components_np() for all three neighbourhoods, with and without a box
off the origin; the ctypes mirror and the numpy dtype have the C layout; the entry points are declared, exported and bound; bad arguments
are rejected without a device; Volume.clear_border's rule is skimage.segmentation.clear_border's, restated; the kernels of
component_stats.hip use no scratch memory; and the shapes of tests/test_gpu_component_stats.py reach what they are there for.
tests/test_gpu_component_stats.py holds the kernels to component_stats_np() and select_by_table_np() bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import helpers as T
from tests.test_components_cpu import components_np
from tests.test_gpu_components import CONTENTS, EXTENTS, contents
from vkvolume_amd import abi, lib, volume as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISO = 0.5
DTYPE = abi.component_stats_dtype()
U32_FIELDS = ("min_x", "min_y", "min_z", "max_x", "max_y", "max_z", "min_value", "max_value")
U64_FIELDS = ("voxels", "sum_x", "sum_y", "sum_z", "sum_value", "sum_value2")
SPAN_VOXELS = 2048        # kCsSpan entries of 64 voxels: what one wave walks


def box_of(shape_dhw, box):
    """(x0, y0, z0, w, h, d) of `box`, or of the whole volume"""
    return (0, 0, 0) + tuple(shape_dhw)[::-1] if box is None else tuple(box)


def component_stats_np(vol, labels, n_labels, capacity, box=None):
    """the records [0, written) of the header's sentences as a structured array, written = min(n_labels, capacity): per label k <= written
    the inclusive bounding box of its voxels in VOLUME coordinates, their number, the sums of their coordinates and, with a volume, the
    smallest and largest byte and the sums of bytes and squared bytes; labels 0 and above `written` are ignored; a label without a voxel
    keeps mins 0xffffffff, maxes 0, sums 0; vol None: the four value fields are 0.  Exact integer arithmetic throughout."""
    x0, y0, z0, w, h, d = box_of(labels.shape if vol is None else vol.shape, box)
    assert labels.shape == (d, h, w)
    written = min(int(n_labels), int(capacity))
    rec = np.zeros(written, DTYPE)
    for f in ("min_x", "min_y", "min_z"):
        rec[f] = 0xffffffff
    if vol is not None:
        rec["min_value"] = 0xffffffff
    flat = labels.reshape(-1).astype(np.int64)
    counted = np.flatnonzero((flat != 0) & (flat <= written))
    if not len(counted):
        return rec
    order = counted[np.argsort(flat[counted], kind="stable")]
    present, starts = np.unique(flat[order], return_index=True)
    k = present - 1
    i = order.astype(np.uint64)
    x, y, z = i % np.uint64(w) + np.uint64(x0), i // np.uint64(w) % np.uint64(h) + np.uint64(y0), i // np.uint64(w * h) + np.uint64(z0)
    rec["voxels"][k] = np.add.reduceat(np.ones(len(i), np.uint64), starts)
    for axis, c in (("x", x), ("y", y), ("z", z)):
        rec["min_" + axis][k] = np.minimum.reduceat(c, starts)
        rec["max_" + axis][k] = np.maximum.reduceat(c, starts)
        rec["sum_" + axis][k] = np.add.reduceat(c, starts)
    if vol is not None:
        b = np.ascontiguousarray(vol, np.uint8)[z0:z0 + d, y0:y0 + h, x0:x0 + w].reshape(-1)[order].astype(np.uint64)
        rec["min_value"][k] = np.minimum.reduceat(b, starts)
        rec["max_value"][k] = np.maximum.reduceat(b, starts)
        rec["sum_value"][k] = np.add.reduceat(b, starts)
        rec["sum_value2"][k] = np.add.reduceat(b * b, starts)
    return rec


def select_by_table_np(src_dhw, labels, keep, fill, box=None, dst=None):
    """vkv_select_components_by_table: `dst` (None: a copy of src) with the box's voxels written: `fill` where the voxel's label L is in
    1 .. len(keep) and keep[L - 1] == 0, else the source's byte"""
    src = np.ascontiguousarray(src_dhw, np.uint8)
    out = src.copy() if dst is None else dst.copy()
    x0, y0, z0, w, h, d = box_of(src.shape, box)
    assert labels.shape == (d, h, w)
    keep = np.asarray(keep).astype(np.uint8)
    sub = src[z0:z0 + d, y0:y0 + h, x0:x0 + w].copy()
    named = (labels != 0) & (labels <= len(keep))
    reject = np.zeros(labels.shape, bool)
    reject[named] = keep[labels[named].astype(np.int64) - 1] == 0
    sub[reject] = fill
    out[z0:z0 + d, y0:y0 + h, x0:x0 + w] = sub
    return out


def touches_no_face_np(rec, shape_dhw, box=None):
    """Volume.clear_border's keep table from the records: the bounding box touches no face of the box"""
    x0, y0, z0, w, h, d = box_of(shape_dhw, box)
    r = {f: rec[f].astype(np.int64) for f in U32_FIELDS}
    return ((r["min_x"] > x0) & (r["min_y"] > y0) & (r["min_z"] > z0) & (r["max_x"] < x0 + w - 1) & (r["max_y"] < y0 + h - 1) & (r["max_z"] < z0 + d - 1))


def clear_border_np(vol, iso, connectivity, fill, box=None):
    """skimage.segmentation.clear_border(labels, buffer_size=0) restated: the labels that occur on the outermost voxels of any axis of the
    label array (the box) are removed; here removing a label fills its voxels of the volume"""
    labels = components_np(vol, iso, connectivity, box)[0]
    borders = np.zeros(labels.shape, bool)
    for axis in range(3):
        for end in (0, -1):
            index = [slice(None)] * 3
            index[axis] = end
            borders[tuple(index)] = True
    remove = np.unique(labels[borders])
    x0, y0, z0, w, h, d = box_of(vol.shape, box)
    out = vol.copy()
    sub = out[z0:z0 + d, y0:y0 + h, x0:x0 + w]
    sub[np.isin(labels, remove[remove != 0])] = fill
    return out


BORDER_SHAPE = (12, 14, 70)        # depth, height, width
BORDER_BOX = (4, 2, 2, 60, 10, 8)        # x 4 .. 63, y 2 .. 11, z 2 .. 9
#               name: (x range, y range, z range), value
BORDER_BODIES = {
    "face x0": ((0, 3), (6, 8), (5, 7), 200), "face x1": ((67, 70), (6, 8), (5, 7), 201), "face y0": ((30, 33), (0, 2), (5, 7), 202),
    "face y1": ((30, 33), (12, 14), (5, 7), 203), "face z0": ((40, 43), (6, 8), (0, 2), 204), "face z1": ((40, 43), (6, 8), (10, 12), 205),
    "interior": ((20, 26), (5, 8), (4, 7), 206),
    "box face only": ((4, 7), (5, 7), (4, 6), 207),        # touches x = 4, the box's face, and no face of the volume
    "cut by the box": ((60, 66), (8, 10), (4, 6), 208),        # runs through x = 63, the box's far face
}


def border_volume():
    """the hand-made volume of the clear_border tests: a dim background and nine bright cuboids, apart from one another"""
    vol = np.full(BORDER_SHAPE, 10, np.uint8)
    for (xa, xb), (ya, yb), (za, zb), value in BORDER_BODIES.values():
        vol[za:zb, ya:yb, xa:xb] = value
    return vol


def survivors(vol):
    return {name for name, (_, _, _, value) in BORDER_BODIES.items() if (vol == value).any()}


# ---- the statement -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 14, 26])
@pytest.mark.parametrize("box", [None, (3, 2, 1, 6, 5, 4)], ids=["whole", "box"])
def test_component_stats_np_is_scipy(connectivity, box):
    from scipy import ndimage
    shape = (6, 8, 10)
    for k, content in enumerate(CONTENTS):
        vol = contents(content, shape, seed=300 + k)
        bright = vol >= 128
        vol = np.where(bright, np.random.default_rng(k).integers(128, 256, size=shape, dtype=np.uint8), vol).astype(np.uint8)        # not one value
        labels, sizes, counts = components_np(vol, ISO, connectivity, box)
        n = int(counts[0])
        rec = component_stats_np(vol, labels, n, n + 3, box)
        assert len(rec) == n and rec.dtype == DTYPE
        x0, y0, z0, w, h, d = box_of(shape, box)
        crop = vol[z0:z0 + d, y0:y0 + h, x0:x0 + w].astype(np.int64)
        index = np.arange(1, n + 1)
        assert np.array_equal(rec["voxels"], sizes)
        if not n:
            continue
        for r, sl in zip(rec, ndimage.find_objects(labels.astype(np.int32), max_label=n)):
            assert (r["min_z"], r["min_y"], r["min_x"]) == (sl[0].start + z0, sl[1].start + y0, sl[2].start + x0), (content, box)        # volume coordinates
            assert (r["max_z"], r["max_y"], r["max_x"]) == (sl[0].stop - 1 + z0, sl[1].stop - 1 + y0, sl[2].stop - 1 + x0)
        assert np.array_equal(rec["sum_value"], ndimage.sum_labels(crop, labels, index).astype(np.uint64))
        assert np.array_equal(rec["sum_value2"], ndimage.sum_labels(crop * crop, labels, index).astype(np.uint64))
        assert np.array_equal(rec["min_value"], ndimage.minimum(crop, labels, index).astype(np.uint32))
        assert np.array_equal(rec["max_value"], ndimage.maximum(crop, labels, index).astype(np.uint32))
        com = np.array(ndimage.center_of_mass(np.ones(labels.shape), labels, index)) + (z0, y0, x0)        # (z, y, x) per label
        sums = np.stack([rec["sum_z"], rec["sum_y"], rec["sum_x"]], axis=1)
        assert np.array_equal(np.rint(com * rec["voxels"][:, None]).astype(np.uint64), sums), (content, box)
        assert np.abs(com * rec["voxels"][:, None] - sums).max() < 1e-6


def test_capacity_empty_labels_and_no_volume():
    vol = np.array([[[9, 200, 0, 130, 131, 0, 255]]], np.uint8)
    labels = np.array([[[0, 1, 0, 4, 4, 0, 2]]], np.uint32)        # label 3 is empty, n_labels = 6 names two more that no voxel carries
    rec = component_stats_np(vol, labels, 6, 10)
    assert len(rec) == 6
    assert rec[0].tolist() == (1, 0, 0, 1, 0, 0, 200, 200, 1, 1, 0, 0, 200, 40000)
    assert rec[3].tolist() == (3, 0, 0, 4, 0, 0, 130, 131, 2, 7, 0, 0, 261, 130 * 130 + 131 * 131)
    empty = (0xffffffff,) * 3 + (0,) * 3 + (0xffffffff, 0) + (0,) * 6
    assert rec[2].tolist() == rec[4].tolist() == rec[5].tolist() == empty
    short = component_stats_np(vol, labels, 6, 2)        # labels above the capacity are ignored
    assert len(short) == 2 and short.tobytes() == rec[:2].tobytes()
    assert len(component_stats_np(vol, labels, 6, 0)) == 0 and len(component_stats_np(vol, labels, 0, 5)) == 0
    bare = component_stats_np(None, labels, 6, 6)
    for f in ("min_value", "max_value", "sum_value", "sum_value2"):
        assert not bare[f].any()
    for f in DTYPE.names:
        if "value" not in f:
            assert np.array_equal(bare[f], rec[f]), f
    boxed = component_stats_np(np.zeros((3, 4, 9), np.uint8), labels, 6, 6, box=(2, 3, 1, 7, 1, 1))
    assert (boxed[3]["min_x"], boxed[3]["max_x"], boxed[3]["min_y"], boxed[3]["min_z"], boxed[3]["sum_x"], boxed[3]["sum_y"]) == (5, 6, 3, 1, 11, 6)


def test_select_by_table_np_keeps_what_the_table_does_not_name():
    vol = np.array([[[9, 200, 0, 130, 131, 0, 255]]], np.uint8)
    labels = np.array([[[0, 1, 0, 4, 4, 0, 2]]], np.uint32)
    assert select_by_table_np(vol, labels, [0, 1, 1, 0], 7)[0, 0].tolist() == [9, 7, 0, 7, 7, 0, 255]
    assert select_by_table_np(vol, labels, [0, 0], 7)[0, 0].tolist() == [9, 7, 0, 130, 131, 0, 7]        # label 4 is beyond the table
    assert np.array_equal(select_by_table_np(vol, labels, [], 7), vol)
    assert select_by_table_np(vol, labels, np.array([True, False, True, True]), 0)[0, 0].tolist() == [9, 200, 0, 130, 131, 0, 0]


# ---- layout and entry points -----------------------------------------------------------------------------------------------------------------
def test_the_mirrors_match_the_c_layout(tmp_path):
    fields = [f for f, _ in abi.ComponentStats._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vkvolume_amd.h"\nint main(void) {\n'
                   '  printf("sizeof %zu\\n", sizeof(VkvComponentStats));\n'
                   '  printf("alignof %zu\\n", (size_t) _Alignof(VkvComponentStats));\n' +
                   "".join('  printf("%s %%zu\\n", offsetof(VkvComponentStats, %s));\n' % (f, f) for f in fields) +
                   "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)]).decode().split("\n") if line.strip())
    assert int(out.pop("sizeof")) == 80 == C.sizeof(abi.ComponentStats) == DTYPE.itemsize == abi.COMPONENT_STATS_BYTES
    assert int(out.pop("alignof")) == 8 == C.alignment(abi.ComponentStats) == DTYPE.alignment
    assert fields == list(U32_FIELDS + U64_FIELDS) == list(DTYPE.names)
    assert [int(out[f]) for f in fields] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64, 72]
    for f in fields:
        assert int(out[f]) == getattr(abi.ComponentStats, f).offset == DTYPE.fields[f][1], f
        assert DTYPE.fields[f][0] == np.dtype("<u4" if f in U32_FIELDS else "<u8") and getattr(abi.ComponentStats, f).size == DTYPE.fields[f][0].itemsize


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "vkvolume_amd.h")).read()
    assert re.search(r"\bint\s+vkv_component_stats\s*\(\s*vkv_ctx\s*\*ctx,\s*const uint8_t\s*\*d_volume,\s*VkvExtent3D extent,\s*const VkvBox\s*\*box,\s*"
                     r"const uint32_t\s*\*d_labels,\s*const uint64_t\s*\*d_counts,\s*VkvComponentStats\s*\*d_stats,\s*uint64_t capacity_components,\s*"
                     r"void\s*\*stream\)", header)
    assert re.search(r"\bint\s+vkv_select_components_by_table\s*\(\s*vkv_ctx\s*\*ctx,\s*const uint8_t\s*\*d_src,\s*uint8_t\s*\*d_dst,\s*VkvExtent3D extent,\s*"
                     r"const VkvBox\s*\*box,\s*const uint32_t\s*\*d_labels,\s*const uint8_t\s*\*d_keep,\s*uint64_t table_entries,\s*uint32_t fill,\s*"
                     r"void\s*\*stream\)", header)
    L = lib.load()
    names = {"vkv_component_stats", "vkv_select_components_by_table"}
    assert names <= set(lib.EXPORTS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    assert all(re.search(r"\b%s$" % n, out, flags=re.M) for n in names)
    vp = C.c_void_p
    assert L.vkv_component_stats.argtypes == [vp, vp, abi.Extent3D, C.POINTER(abi.Box), vp, vp, vp, C.c_uint64, vp]
    assert L.vkv_select_components_by_table.argtypes == [vp, vp, vp, abi.Extent3D, C.POINTER(abi.Box), vp, vp, C.c_uint64, C.c_uint32, vp]
    for name in ("component_stats", "component_stats_rc", "select_components_by_table", "select_components_by_table_rc"):
        assert callable(getattr(lib.Context, name)), name
    for name in ("component_stats", "select_components", "clear_border", "remove_islands"):
        assert callable(getattr(V.Volume, name)), name
    for name in ("voxels", "bbox_min", "bbox_max", "centroid", "mean", "variance", "min_value", "max_value", "numpy"):
        assert hasattr(V.ComponentStats, name), name
    makefile = open(os.path.join(ROOT, "vkvolume_amd", "csrc", "Makefile")).read().replace("\\\n", " ")
    assert re.search(r"^SRCS\s*:=.*\bcomponent_stats\.hip\b", makefile, flags=re.M)


def test_bad_arguments_without_a_device():
    L = lib.load()
    buf = (C.c_uint64 * 256)()
    a = C.addressof(buf)
    e, bad = abi.Extent3D(4, 4, 4), abi.VKV_E_INVALID_ARGUMENT
    # a null context: nothing else is looked at, nothing is written
    assert L.vkv_component_stats(None, a, e, None, a + 512, a + 128, a + 1024, 4, None) == bad
    assert L.vkv_select_components_by_table(None, a, a, e, None, a + 512, a + 128, 4, 0, None) == bad
    assert not any(buf)


# ---- Volume.clear_border's rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
def test_clear_border_rule_is_skimages_on_the_hand_made_volume(connectivity):
    vol = border_volume()
    assert components_np(vol, ISO, connectivity)[2][0] == len(BORDER_BODIES) == 9
    for box, kept in ((None, {"interior", "box face only", "cut by the box"}), (BORDER_BOX, {"interior"})):
        labels, _, counts = components_np(vol, ISO, connectivity, box)
        rec = component_stats_np(None, labels, int(counts[0]), int(counts[0]), box)
        got = select_by_table_np(vol, labels, touches_no_face_np(rec, vol.shape, box), 3, box)
        want = clear_border_np(vol, ISO, connectivity, 3, box)
        assert np.array_equal(got, want), box
        x0, y0, z0, w, h, d = box_of(vol.shape, box)
        inside_box = np.zeros(vol.shape, bool)
        inside_box[z0:z0 + d, y0:y0 + h, x0:x0 + w] = True
        assert np.array_equal(got[~inside_box], vol[~inside_box])
        assert survivors(np.where(inside_box, got, 0)) == kept, box
    # the bodies outside the box are not its business, and the body the box cuts is removed only inside it
    assert (got[5, 8, 64:66] == 208).all() and (got[5, 8, 60:64] == 3).all() and int(counts[0]) == 3


def test_clear_border_rule_on_random_volumes():
    rng = np.random.default_rng(12)
    for k in range(12):
        shape = tuple(rng.integers(1, 8, size=3))
        vol = np.where(rng.random(shape) < 0.25, 200, 17).astype(np.uint8)
        for connectivity in (6, 14, 26):
            labels, _, counts = components_np(vol, ISO, connectivity)
            rec = component_stats_np(None, labels, int(counts[0]), int(counts[0]))
            got = select_by_table_np(vol, labels, touches_no_face_np(rec, shape), 0)
            assert np.array_equal(got, clear_border_np(vol, ISO, connectivity, 0)), (shape, connectivity)        # an axis of length 1: everything goes


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch_memory(tmp_path):
    kernels = T.kernel_listing("component_stats.hip", tmp_path / "component_stats.s")
    for name in ("k_cs_init", "k_cs_accumulate", "k_cs_select_table"):
        assert len([k for k in kernels if name in k]) == 1, sorted(kernels)
    assert len(kernels) == 3
    for k, v in kernels.items():
        assert v.get("ScratchSize") == 0, (k, v)


# ---- what the GPU shapes reach -----------------------------------------------------------------------------------------------------------------
SLAB_EXTENT = (4096, 600, 1)        # (width, height, depth): one component, every byte 255
X_NEEDLE = (1 << 22) + 5
NARROW = [(7, 3, 3), (5, 7, 67), (9, 33, 5), (3, 1, 4), (1, 4, 3), (2, 2, 2), (4, 5, 1)]
STATS_EXTENTS = EXTENTS + [(7, 3, 3), (131, 3, 2), (130, 17, 5), (130, 17, 17)]
WORKGROUP_ENTRIES = 16 * 32        # sixteen waves of one span each


def own_labels(shape_dhw):
    """every voxel its own component, numbered in memory order: 64 distinct labels in every full entry"""
    return np.arange(1, int(np.prod(shape_dhw)) + 1, dtype=np.uint32).reshape(shape_dhw)


def test_the_slab_needs_64_bit_sums():
    w, h, d = SLAB_EXTENT
    rec = component_stats_np(np.full((d, h, w), 255, np.uint8), np.ones((d, h, w), np.uint32), 1, 1)[0]
    assert rec["sum_x"] == h * (w * (w - 1) // 2) > 2 ** 32 and rec["sum_value2"] == w * h * 255 * 255 > 2 ** 32
    assert rec["voxels"] == w * h and rec["sum_y"] == w * (h * (h - 1) // 2) and (rec["max_x"], rec["max_y"], rec["max_z"]) == (w - 1, h - 1, 0)


def test_the_x_needles_last_full_span_alone_passes_32_bits():
    assert (X_NEEDLE - 5) % SPAN_VOXELS == 0        # the last span of all holds the five voxels behind 2^22; the one before it is full
    x = np.arange(X_NEEDLE - 5 - SPAN_VOXELS, X_NEEDLE - 5, dtype=np.uint64)
    assert len(x) == SPAN_VOXELS and int(x.sum()) > 2 ** 32        # 8.6e9: one wave's pending partial sum
    assert int(x.sum()) // 64 < 2 ** 32        # while one lane's share still fits: the 64-bit need arises where the lanes meet
    rec = component_stats_np(None, np.ones((1, 1, X_NEEDLE), np.uint32), 1, 1)[0]
    assert rec["sum_x"] == X_NEEDLE * (X_NEEDLE - 1) // 2 and rec["max_x"] == X_NEEDLE - 1 and rec["voxels"] == X_NEEDLE


def test_the_worst_cases_of_the_reduction_loop():
    """the 3-D checkerboard's inside voxels are half of all voxels, so under 6 a full entry of its labels holds 32 distinct labels, each on one
    lane; the array that gives every voxel a label of its own holds 64, the most an entry can"""
    shape = (2, 3, 128)
    labels = components_np(contents("checkerboard", shape), ISO, 6)[0].reshape(-1)
    assert [len(np.unique(labels[e * 64:(e + 1) * 64][labels[e * 64:(e + 1) * 64] != 0])) for e in range(len(labels) // 64)] == [32] * 12
    own = own_labels(shape).reshape(-1)
    assert all(len(np.unique(own[e * 64:(e + 1) * 64])) == 64 for e in range(len(own) // 64))


def test_a_label_continues_across_a_span_boundary_beside_a_second_label():
    shape = (5, 17, 130)        # 11050 voxels: five spans and a part
    found = []
    for content in CONTENTS:
        for connectivity in (6, 26):
            labels = components_np(contents(content, shape, seed=900 + CONTENTS.index(content)), ISO, connectivity)[0].reshape(-1)
            for s in range(SPAN_VOXELS, len(labels), SPAN_VOXELS):
                before, after = labels[s - SPAN_VOXELS:s], labels[s:s + SPAN_VOXELS]
                carried = np.intersect1d(before[before != 0], after[after != 0])
                if len(carried) and len(np.unique(after[after != 0])) >= 2:
                    found.append((content, connectivity, s))
    assert {c for c, _, _ in found} >= {"random 0.1", "random 0.31", "random 0.6"}, found        # (the serpentine and the slabs are one component)


def test_the_narrow_extents_wrap_three_or_more_rows_in_an_entry():
    assert set(NARROW) <= set(STATS_EXTENTS)
    for w, h, d in NARROW:
        n = w * h * d
        for first in range(0, n, 64):
            i = np.arange(first, min(first + 64, n))
            if len(i) == 64 or first == 0:
                assert len(np.unique(i // w)) >= 3, (w, h, d, first)
    w, h, d = STATS_EXTENTS[-2]
    assert (w * h * d + 63) // 64 > 4 * 32        # several waves of a workgroup walk a span each
    w, h, d = STATS_EXTENTS[-1]
    assert (w * h * d + 63) // 64 > WORKGROUP_ENTRIES        # more entries than one workgroup's sixteen spans
