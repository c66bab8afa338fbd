"""The contents, the scipy references and the arithmetic of tests/test_gpu_components_scale.py, and what can be shown of them without a GPU.

vkv_label_components merges through a lock-free union-find whose intermediate state depends on the schedule; only its
result is unique.  The extents of tests/test_gpu_components.py that merge at all hold at most 1040 workgroups, fewer than an MI355X keeps
resident at once (256 CUs x 32 waves / 4 waves = 2048 workgroups at the most: derived from the occupancy limits, not measured; register use
only lowers it).  SCALE, 251 x 127 x 131 = 4 175 887 voxels, is 16 313 workgroups, about eight times that bound: trees built by workgroups
that have finished are hooked, compressed and re-rooted by workgroups that start later, on other XCDs.  It is 16 scan chunks, the last one
partial, and its width is no multiple of 64, so entries start in the middle of rows and wrap at every phase.

The reference at this size is scipy.ndimage.label with structure_of(connectivity): its numbering is the call's by specification, and
components_np() is held to it on small shapes by tests/test_components_cpu.py and once here at size.  The contents:
  random        default_rng(7).random(shape) < p at each neighbourhood's percolation point, p = 0.31 (6), 0.18 (14), 0.10 (26): many
                components of all sizes, the largest tortuous and present in every scan chunk;
  serpentine    the generator of tests/test_gpu_components.py: ONE path of 1 064 447 voxels, the longest find chains;
  comb x, y, z  lines along the axis at every even position of the other two axes, plus the full LAST slice of that axis: thousands of
                trees, each rooted at its line's first voxel, joined only at the far end, so every union hooks a large finished tree;
  teeth x, y, z the combs without the joining slice: thousands of equal components, labelled in the order of their first voxels;
  checkerboard  under 14 and 26 every inside voxel starts its own x-run and unions with up to twelve neighbours, all converging on voxel
                0; under 6, 2 087 944 singletons.
Every number asserted below comes from scipy and the generators alone."""
import functools

import numpy as np
import pytest

from tests.test_components_cpu import components_np, inside_np, structure_of
from tests.test_gpu_components import serpentine

ISO = 0.5
CONNECTIVITIES = (6, 14, 26)
SCALE = (251, 127, 131)        # (width, height, depth)
SHAPE = SCALE[::-1]
VOXELS = 4175887
WORKGROUP_VOXELS, CHUNK_VOXELS = 256, 4096 * 64
RESIDENT_WORKGROUPS = 256 * 32 // 4        # an upper bound: 256 CUs x 32 waves per CU, four waves per workgroup
BOX_VOLUME_EXTENT = (256, 130, 133)        # the volume of the box case, and SCALE as a box inside it
BOX = (3, 2, 1) + SCALE

RANDOM_P = {6: 0.31, 14: 0.18, 26: 0.10}
#                  K, voxels of the largest component
RANDOM_TABLE = {6: (227965, 92953), 14: (95102, 241017), 26: (55048, 111508)}
AT_LEAST_1000_UNDER_14 = 24        # components of >= 1000 voxels in the p = 0.18 case under 14
SERPENTINE_VOXELS = 1064447
TEETH = {"x": (4224, 251), "y": (8316, 127), "z": (8064, 131)}        # lines, voxels per line
CHECKERBOARD_INSIDE = 2087944
CONTENTS = ("random", "serpentine", "comb x", "comb y", "comb z", "teeth x", "teeth y", "teeth z", "checkerboard")
_AXIS = {"x": 2, "y": 1, "z": 0}


# ---- contents ---------------------------------------------------------------------------------------------------------------------------
def random_volume(p, shape_dhw=SHAPE, seed=7):
    return np.where(np.random.default_rng(seed).random(shape_dhw) < p, 200, 17).astype(np.uint8)


def comb(axis, shape_dhw=SHAPE, joined=True):
    """lines along `axis` at every even position of the other two axes; joined: plus the full last slice of that axis"""
    vol = np.full(shape_dhw, 17, np.uint8)
    lines = [slice(None, None, 2)] * 3
    lines[_AXIS[axis]] = slice(None)
    vol[tuple(lines)] = 255
    if joined:
        last = [slice(None)] * 3
        last[_AXIS[axis]] = shape_dhw[_AXIS[axis]] - 1
        vol[tuple(last)] = 255
    return vol


def checkerboard(shape_dhw=SHAPE):
    z, y, x = np.indices(shape_dhw, dtype=np.int32)
    return np.where((x + y + z) % 2 == 0, 255, 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _volume(name):
    if name.startswith("random"):
        vol = random_volume(float(name.split()[1]))
    elif name == "serpentine":
        vol = serpentine(SHAPE)
    elif name == "checkerboard":
        vol = checkerboard()
    else:
        kind, axis = name.split()
        vol = comb(axis, joined=kind == "comb")
    vol.setflags(write=False)
    return vol


def volume_of(content, connectivity):
    """the SCALE volume of one of CONTENTS (read-only, shared); `random` is the connectivity's own density"""
    return _volume("random %g" % RANDOM_P[connectivity] if content == "random" else content)


@functools.lru_cache(maxsize=None)
def box_volume(connectivity):
    """BOX_VOLUME_EXTENT of the same density from another seed, with the connectivity's random SCALE volume as the voxels of BOX: inside
    voxels lie against every face of the box from outside, and the reference is the reference of the SCALE volume"""
    w, h, d = BOX_VOLUME_EXTENT
    vol = random_volume(RANDOM_P[connectivity], (d, h, w), seed=8)
    x0, y0, z0, bw, bh, bd = BOX
    vol[z0:z0 + bd, y0:y0 + bh, x0:x0 + bw] = volume_of("random", connectivity)
    vol.setflags(write=False)
    return vol


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def scipy_want(vol, connectivity):
    """(labels uint32, sizes uint32 [K], counts uint64 [K, K, inside]) from scipy.ndimage.label alone"""
    from scipy import ndimage
    inside = inside_np(vol, ISO)
    labels, k = ndimage.label(inside, structure=structure_of(connectivity))
    sizes = np.bincount(labels.reshape(-1))[1:].astype(np.uint32)
    assert len(sizes) == k
    want = labels.astype(np.uint32), sizes, np.array([k, k, int(inside.sum())], np.uint64)
    for a in want:
        a.setflags(write=False)
    return want


@functools.lru_cache(maxsize=6)        # 17 MB of labels each: the tests of one (content, connectivity) run next to each other
def want_of(content, connectivity):
    return scipy_want(volume_of(content, connectivity), connectivity)


def teeth_labels(axis, inside):
    """the closed form for lines along `axis`: a line's label is the running count of line starts (in memory order) at its first voxel"""
    a = _AXIS[axis]
    first = [slice(None)] * 3
    first[a] = slice(0, 1)
    starts = np.zeros(inside.shape, bool)
    starts[tuple(first)] = inside[tuple(first)]
    running = np.cumsum(starts.reshape(-1), dtype=np.uint32).reshape(inside.shape)
    return np.where(inside, running[tuple(first)], np.uint32(0))


# ---- the figures the argument rests on ----------------------------------------------------------------------------------------------------
def test_the_shape_is_several_generations_of_workgroups():
    w, h, d = SCALE
    assert w * h * d == VOXELS
    workgroups = -(-VOXELS // WORKGROUP_VOXELS)
    assert workgroups == 16313 and RESIDENT_WORKGROUPS == 2048 and workgroups >= 4 * RESIDENT_WORKGROUPS
    assert -(-VOXELS // CHUNK_VOXELS) == 16 and VOXELS % CHUNK_VOXELS != 0        # 16 scan chunks, the last one partial
    assert w % 64 != 0 and np.gcd(w, 64) == 1        # entries start at every phase of a row
    assert 64 * 65 * 64 // WORKGROUP_VOXELS == 1040 < RESIDENT_WORKGROUPS        # the largest merging extent of the small-shape suite
    x0, y0, z0, bw, bh, bd = BOX
    assert (bw, bh, bd) == SCALE and min(x0, y0, z0) > 0
    assert all(o + n < e for o, n, e in zip((x0, y0, z0), SCALE, BOX_VOLUME_EXTENT))        # the volume goes on behind every face


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_random_at_the_percolation_point(connectivity):
    labels, sizes, counts = want_of("random", connectivity)
    k, largest = RANDOM_TABLE[connectivity]
    assert counts.tolist() == [k, k, int(sizes.sum(dtype=np.uint64))] and int(sizes.max()) == largest
    where = np.flatnonzero(labels.reshape(-1) == int(sizes.argmax()) + 1)        # box-linear indices, ascending
    assert len(where) == largest
    z = where // (SCALE[0] * SCALE[1])
    assert (z.min(), z.max()) == (0, SCALE[2] - 1)
    assert where[0] // CHUNK_VOXELS == 0 and where[-1] // CHUNK_VOXELS == 15
    assert len(np.unique(where // CHUNK_VOXELS)) == 16        # and it has voxels in every chunk between
    if connectivity == 14:
        assert int((sizes >= 1000).sum()) == AT_LEAST_1000_UNDER_14


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_serpentine_and_combs_are_one_component(connectivity):
    for content in ("serpentine", "comb x", "comb y", "comb z"):
        vol = volume_of(content, connectivity)
        labels, sizes, counts = want_of(content, connectivity)
        inside = vol >= 128
        assert counts.tolist() == [1, 1, int(inside.sum())] and sizes.tolist() == [int(inside.sum())], content
        assert np.array_equal(labels, inside.astype(np.uint32)), content
    assert int((volume_of("serpentine", connectivity) >= 128).sum()) == SERPENTINE_VOXELS


def test_the_serpentine_is_a_path():
    inside = volume_of("serpentine", 6) >= 128
    padded = np.pad(inside, 1).astype(np.int8)
    degree = sum(np.roll(padded, o, a) for a in range(3) for o in (1, -1))[1:-1, 1:-1, 1:-1]        # inside 6-neighbours
    assert int(((degree == 1) & inside).sum()) == 2 and int(((degree > 2) & inside).sum()) == 0        # two ends, no branch


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("axis", sorted(TEETH))
def test_teeth_are_labelled_in_the_order_of_their_first_voxels(axis, connectivity):
    vol = volume_of("teeth " + axis, connectivity)
    labels, sizes, counts = want_of("teeth " + axis, connectivity)
    lines, length = TEETH[axis]
    assert counts.tolist() == [lines, lines, lines * length] and (sizes == length).all() and len(sizes) == lines
    assert length == SHAPE[_AXIS[axis]]
    assert np.array_equal(labels, teeth_labels(axis, vol >= 128))
    joined = volume_of("comb " + axis, connectivity)
    assert int((joined != vol).sum()) == (VOXELS // length - lines)        # the joining slice adds exactly the voxels between the lines' ends


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_checkerboard(connectivity):
    vol = volume_of("checkerboard", connectivity)
    labels, sizes, counts = want_of("checkerboard", connectivity)
    inside = vol >= 128
    assert int(inside.sum()) == CHECKERBOARD_INSIDE == (VOXELS + 1) // 2
    if connectivity == 6:
        assert counts.tolist() == [CHECKERBOARD_INSIDE] * 3 and (sizes == 1).all()
        assert np.array_equal(labels, np.where(inside, np.cumsum(inside.reshape(-1), dtype=np.uint32).reshape(inside.shape), np.uint32(0)))
    else:
        assert counts.tolist() == [1, 1, CHECKERBOARD_INSIDE]
        assert np.array_equal(labels, inside.astype(np.uint32))


@pytest.mark.parametrize("connectivity", [6, 26])
def test_the_box_volume_holds_the_scale_volume_and_goes_on_around_it(connectivity):
    vol = box_volume(connectivity)
    x0, y0, z0, w, h, d = BOX
    assert vol.shape == BOX_VOLUME_EXTENT[::-1]
    assert np.array_equal(vol[z0:z0 + d, y0:y0 + h, x0:x0 + w], volume_of("random", connectivity))
    inside = vol >= 128
    around = (inside[z0 - 1, y0:y0 + h, x0:x0 + w], inside[z0 + d, y0:y0 + h, x0:x0 + w], inside[z0:z0 + d, y0 - 1, x0:x0 + w],
              inside[z0:z0 + d, y0 + h, x0:x0 + w], inside[z0:z0 + d, y0:y0 + h, x0 - 1], inside[z0:z0 + d, y0:y0 + h, x0 + w])
    assert all(int(f.sum()) > 100 for f in around)        # inside voxels against every face: a component that leaked out would merge others
    from scipy import ndimage
    whole, _ = ndimage.label(inside, structure=structure_of(connectivity))
    crop = whole[z0:z0 + d, y0:y0 + h, x0:x0 + w]
    assert len(np.unique(crop[crop != 0])) < RANDOM_TABLE[connectivity][0]        # and labelling the whole volume does merge some


# ---- components_np at size ----------------------------------------------------------------------------------------------------------------
def test_components_np_is_scipy_label_at_size():
    """the statement of the header in numpy against scipy on the p = 0.31 case under 6: partition, numbering, sizes, counts"""
    labels, sizes, counts = components_np(volume_of("random", 6), ISO, 6)
    wl, ws, wc = want_of("random", 6)
    assert counts.tolist() == wc.tolist()
    assert np.array_equal(labels, wl) and labels.dtype == wl.dtype
    assert np.array_equal(sizes, ws) and sizes.dtype == ws.dtype
