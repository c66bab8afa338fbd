"""GPU: vkv_nearest_target and vkv_propagate_labels bit for bit against nearest_separable_np / propagate_labels_np of
tests/test_nearest_cpu.py, d_dist2 against vkv_distance_transform_weighted's bytes on the device, and Volume.nearest_target /
expand_labels / split_bodies against the numpy statements.

Pattern, helpers and shapes are those of tests/test_gpu_distance_weighted.py: axes of length 1 (their pass is not launched, so the x pass
starts in either buffer and the LAST launched pass writes the final format, whichever it is: 1 x 1 x n and n x 1 x 1 are added), widths
below a wave and around one and two words, 200-voxel needles, 70 x 66 x 65 (several workgroups per pass) and 32768 along each axis.
Contents: those of the weighted test plus the ones BUILT FOR TIES (two faces of an odd axis, all eight corners, a checkerboard, random
0.5): kernels built from the envelope without the tie rule fail on them.  The reference of a limited call is the unlimited one with NONE
where the distance is >= limit: the definition (tests/test_nearest_cpu.py holds the separable statement to it at every limit).  Every buffer
is a guarded allocation, pre-filled and compared as a whole; the scratch is exactly vkv_distance_transform_scratch_bytes."""
import numpy as np
import pytest
import torch

from tests import helpers as T
from tests.test_distance_cpu import NONE, TO_INSIDE, TO_OUTSIDE, inside_np
from tests.test_gpu_distance_weighted import (BOX_VOLUME, BOXES, EXTENTS, FILL, ISO, LONG_CONTENTS, LONGEST, TARGETS, WEIGHTED_CONTENTS, cap, contents, ext_of,
                                              guard_damage, long_weights, make_volume, run as run_weighted, same, st, upload)
from tests.test_nearest_cpu import (TIE_CONTENTS, bridge_scene, expand_labels_np, nearest_separable_np, propagate_labels_np, split_bodies_np, tie_contents)
from vkvolume_amd import abi, lib

pytestmark = pytest.mark.gpu

WEIGHTS = ((1, 1, 1), (2, 2, 5), (3, 7, 1), (1, 1, 255))
ALL_CONTENTS = TIE_CONTENTS + tuple(c for c in WEIGHTED_CONTENTS if c not in TIE_CONTENTS)
NEAR_EXTENTS = EXTENTS + [(1, 1, 9), (1, 9, 1), (9, 1, 1), (5, 5, 5), (7, 9, 5)]        # (width, height, depth)


def make(content, shape_dhw, seed=0):
    return tie_contents(content, shape_dhw, seed) if content in TIE_CONTENTS else contents(content, shape_dhw, seed)


def near_limits(weights):
    return (None, 1, min(weights) ** 2, 10, 100000)


def cap_nearest(nearest, dist2, limit):
    """the limited call's d_nearest from the unlimited call's outputs: NONE where the distance is >= limit"""
    return nearest if limit is None else np.where(dist2 < np.uint32(limit), nearest, np.uint32(NONE))


@pytest.fixture(scope="module")
def ctx():
    torch.cuda.set_device(0)
    c = lib.Context(0)
    yield c
    c.close()


# ---- one call ---------------------------------------------------------------------------------------------------------------------------
def run(ctx, vol, iso, target, weights, limit, box=None, device_volume=None, distance=True, what=""):
    """(d_nearest, d_dist2 or None), whole buffers of the box's shape, of ONE vkv_nearest_target call on guarded buffers, every output and the
    scratch pre-filled with FILL; the scratch is vkv_distance_transform's"""
    abox = None if box is None else abi.Box(*box)
    shape = vol.shape if box is None else (box[5], box[4], box[3])
    n = int(np.prod(shape))
    d_vol, h_vol = upload(vol) if device_volume is None else device_volume
    nbytes = lib.distance_transform_scratch_bytes(ext_of(vol), abox)
    assert nbytes == 4 * n + 8 * ((n + 63) // 64), (what, nbytes)
    d_scratch, h_scratch = T.guarded(((nbytes + 7) // 8,), 0, FILL, "cuda", dtype=np.int64)
    d_near, h_near = T.guarded(shape, 0, FILL, "cuda", dtype=np.int32)
    d_dist, h_dist = T.guarded(shape, 0, FILL, "cuda", dtype=np.int32)
    rc = ctx.nearest_target_rc(d_vol.data_ptr(), ext_of(vol), abox, iso, target, weights, limit, d_scratch.data_ptr(), d_near.data_ptr(),
                               d_dist.data_ptr() if distance else None, st())
    assert rc == abi.VKV_OK, (what, rc, ctx.last_error())
    torch.cuda.synchronize()
    for name, h in (("d_volume", h_vol), ("d_scratch", h_scratch), ("d_nearest", h_near), ("d_dist2", h_dist)):
        bad = guard_damage(h)
        assert not bad, "%s: %s: guard bytes %s changed (payload is bytes %d .. %d)" % (what, name, bad[:8], h.start, h.stop - 1)
    if nbytes % 8:        # the scratch block ends 4 bytes before the allocation's payload does: they are not the call's to write
        assert (d_scratch.view(torch.uint8)[nbytes:].cpu().numpy() == FILL).all(), "%s: bytes past the scratch block changed" % what
    assert np.array_equal(d_vol.cpu().numpy(), vol), "%s: the volume changed" % what
    dist = d_dist.cpu().numpy().view(np.uint32)
    if not distance:
        assert (d_dist.view(torch.uint8).cpu().numpy() == FILL).all(), "%s: d_dist2 was not given and was written" % what
    return d_near.cpu().numpy().view(np.uint32), dist if distance else None


def check_nearest(ctx, vol, weights, iso=ISO, limits=None, box=None, what="", against_weighted=False, **kw):
    device_volume = upload(vol, **kw)
    for target in TARGETS:
        want_n, want_d = nearest_separable_np(vol, iso, weights, target, None, box)
        for limit in near_limits(weights) if limits is None else limits:
            w = "%s, weights %s, to %s, limit %s" % (what, weights, ("inside", "outside")[target], limit)
            got_n, got_d = run(ctx, vol, iso, target, weights, limit, box=box, device_volume=device_volume, what=w)
            same(got_n, cap_nearest(want_n, want_d, limit), w + ": d_nearest")
            same(got_d, cap(want_d, limit), w + ": d_dist2")
            if against_weighted:
                same(got_d, run_weighted(ctx, vol, iso, target, weights, limit, box=box, device_volume=device_volume, what=w), w + ": the weighted call's bytes")
                same(run(ctx, vol, iso, target, weights, limit, box=box, device_volume=device_volume, distance=False, what=w)[0], got_n, w + ": without d_dist2")


# ---- every extent ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", NEAR_EXTENTS, ids=lambda e: "%dx%dx%d" % e)
def test_every_extent_content_target_weight_and_limit(ctx, extent):
    w, h, d = extent
    for j, weights in enumerate(WEIGHTS):
        for k, content in enumerate(ALL_CONTENTS):
            vol = make(content, (d, h, w), seed=900 + k)
            # d_dist2 against the other call, and the call without d_dist2: one weight triple per content, in turn
            check_nearest(ctx, vol, weights, what="%s %s" % (content, extent), against_weighted=(j + k) % 4 == 0)


@pytest.mark.parametrize("content", TIE_CONTENTS + ("corner 7", "ball", "random 0.001"), ids=lambda c: c.replace(" ", "_"))
@pytest.mark.parametrize("weights", WEIGHTS, ids=lambda w: "%d_%d_%d" % w)
def test_every_axis_longer_than_a_word(ctx, weights, content):
    w, h, d = 70, 66, 65
    vol = make(content, (d, h, w), seed=41)
    check_nearest(ctx, vol, weights, limits=(None, min(weights) ** 2, 100000), what="%s 70x66x65" % content, against_weighted=content == "random 0.5")


# ---- the longest axis -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", sorted(LONG_CONTENTS), ids=lambda c: c.replace(" ", "_"))
@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
def test_an_axis_of_32768_voxels(ctx, axis, content):
    """the reference is the definition in 64-bit integers over the targets (at the far corners) in box-linear order, a later one taking a
    voxel only where it is strictly nearer.  To the outside, the volume is the inverted one"""
    extent = [2, 2, 2]
    extent[axis] = LONGEST
    w, h, d = extent
    corners = sorted(((d - 1) * (k >> 2 & 1), (h - 1) * (k >> 1 & 1), (w - 1) * (k & 1)) for k in LONG_CONTENTS[content])
    z, y, x = (a.astype(np.uint64) for a in np.indices((d, h, w), sparse=True))
    for weights, farthest in long_weights(axis):
        sq = lambda a, c, wa: (np.uint64(wa) * np.where(a > c, a - np.uint64(c), np.uint64(c) - a)) ** 2  # noqa: E731
        exact = np.full((d, h, w), 2 ** 64 - 1, np.uint64)
        index = np.full((d, h, w), NONE, np.uint64)
        for cz, cy, cx in corners:
            dc = sq(z, cz, weights[2]) + sq(y, cy, weights[1]) + sq(x, cx, weights[0])
            index = np.where(dc < exact, np.uint64((cz * h + cy) * w + cx), index)
            exact = np.minimum(exact, dc)
        for target in TARGETS:
            vol = np.full((d, h, w), 17 if target == TO_INSIDE else 200, np.uint8)
            for c in corners:
                vol[c] = 200 if target == TO_INSIDE else 17
            device_volume = upload(vol)
            for limit in (None, farthest - 1, farthest, farthest + 1, 0xfffffffe):
                lim = np.uint64(NONE if limit is None else limit)
                what = "%s %s, weights %s, to %s, limit %s" % (content, tuple(extent), weights, ("inside", "outside")[target], limit)
                got_n, got_d = run(ctx, vol, ISO, target, weights, limit, device_volume=device_volume, what=what)
                same(got_d, np.minimum(exact, lim).astype(np.uint32), what + ": d_dist2")
                same(got_n, np.where(exact < lim, index, np.uint64(NONE)).astype(np.uint32), what + ": d_nearest")


# ---- boxes, alignment -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box_volume():
    w, h, d = BOX_VOLUME
    return contents("random 0.02", (d, h, w), seed=91)


@pytest.mark.parametrize("box", sorted(BOXES), ids=lambda b: b.replace(" ", "_").replace(",", ""))
def test_a_box_is_transformed_as_the_cropped_array(ctx, box_volume, box):
    b = BOXES[box]
    x0, y0, z0, w, h, d = b
    crop = np.ascontiguousarray(box_volume[z0:z0 + d, y0:y0 + h, x0:x0 + w])
    weights = (2, 2, 5)
    for target in TARGETS:
        want_n, want_d = nearest_separable_np(crop, ISO, weights, target)        # nothing beyond the box exists; indices are the box's
        for limit in (None, 30):
            got_n, got_d = run(ctx, box_volume, ISO, target, weights, limit, box=b, what="box %s" % box)
            assert got_n.shape == (d, h, w)
            same(got_n, cap_nearest(want_n, want_d, limit), "box %s, to %s, limit %s: d_nearest" % (box, target, limit))
            same(got_d, cap(want_d, limit), "box %s, to %s, limit %s: d_dist2" % (box, target, limit))


@pytest.mark.parametrize("extent", [(7, 3, 3), (131, 3, 2)], ids=lambda e: "%dx%dx%d" % e)
def test_every_volume_alignment_with_both_guard_fills(ctx, extent):
    """a result that consumed a guard byte as a voxel differs under one of the two fills"""
    w, h, d = extent
    vol = contents("random 0.1", (d, h, w), seed=77)
    for fill in (0x00, 0xFF):
        for offset in (0, 1, 2, 3):
            check_nearest(ctx, vol, (2, 2, 5), limits=(None, 8), offset=offset, fill=fill, what="%s, volume +%d fill %#x" % (extent, offset, fill))


# ---- determinism and capture ------------------------------------------------------------------------------------------------------------
def test_two_runs_on_the_same_buffers_give_identical_bytes(ctx):
    vol = contents("random 0.01", (19, 5, 258), seed=21)
    d_vol = torch.from_numpy(vol).cuda()
    n = lib.distance_transform_scratch_bytes(ext_of(vol))
    d_scratch = torch.full(((n + 7) // 8,), -1, dtype=torch.int64, device="cuda")
    for target in TARGETS:
        for limit in (None, 30):
            d_near = torch.full(vol.shape, -1, dtype=torch.int32, device="cuda")
            d_dist = torch.full(vol.shape, -1, dtype=torch.int32, device="cuda")
            results = []
            for _ in range(2):        # the second run starts from the first run's features and scratch: stale stack entries in both buffers
                ctx.check(ctx.nearest_target_rc(d_vol.data_ptr(), ext_of(vol), None, ISO, target, (3, 7, 1), limit, d_scratch.data_ptr(), d_near.data_ptr(),
                                                d_dist.data_ptr(), st()))
                torch.cuda.synchronize()
                results.append((d_near.cpu().numpy().view(np.uint32), d_dist.cpu().numpy().view(np.uint32)))
            assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
            want_n, want_d = nearest_separable_np(vol, ISO, (3, 7, 1), target)
            same(results[1][0], cap_nearest(want_n, want_d, limit), "second run: d_nearest")
            same(results[1][1], cap(want_d, limit), "second run: d_dist2")


def test_nearest_and_propagate_captured_into_a_graph_replay(ctx):
    shape = (17, 9, 131)
    weights, r2 = (2, 2, 5), 29
    vol = contents("random 0.05", shape, seed=13)
    labels = (np.arange(vol.size, dtype=np.uint32).reshape(shape) % 7 + 1)
    d_vol = torch.from_numpy(vol).cuda()
    d_labels = torch.from_numpy(labels.view(np.int32)).cuda()
    d_scratch = torch.empty(((lib.distance_transform_scratch_bytes(ext_of(vol)) + 7) // 8,), dtype=torch.int64, device="cuda")
    d_near = torch.empty(shape, dtype=torch.int32, device="cuda")
    d_out = torch.empty(shape, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()

    def call():        # labels grown by radius^2 29 in weighted units
        ctx.check(ctx.nearest_target_rc(d_vol.data_ptr(), ext_of(vol), None, ISO, TO_INSIDE, weights, r2 + 1, d_scratch.data_ptr(), d_near.data_ptr(), None,
                                        s.cuda_stream))
        ctx.check(ctx.propagate_labels_rc(d_near.data_ptr(), d_labels.data_ptr(), d_out.data_ptr(), ext_of(vol), None, None, 0.0, s.cuda_stream))

    torch.cuda.synchronize()
    with torch.cuda.stream(s):  # one direct call on the capture stream
        call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    torch.cuda.synchronize()
    for seed in (13, 14):  # the volume rewritten in place, the outputs fresh, then the graph replayed
        if seed != 13:
            vol = contents("random 0.05", shape, seed=seed)
            d_vol.copy_(torch.from_numpy(vol))
        d_near.view(torch.uint8).fill_(FILL)
        d_out.view(torch.uint8).fill_(FILL)
        d_scratch.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        want_n, _ = nearest_separable_np(vol, ISO, weights, TO_INSIDE, r2 + 1)
        same(d_near.cpu().numpy().view(np.uint32), want_n, "replay, seed %d: d_nearest" % seed)
        same(d_out.cpu().numpy().view(np.uint32), propagate_labels_np(want_n, labels), "replay, seed %d: the grown labels" % seed)


# ---- rejected calls ---------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_write_nothing(ctx):
    w, h, d = 12, 5, 4
    e = abi.Extent3D(w, h, d)
    vol = torch.full((d, h, w), 200, dtype=torch.uint8, device="cuda")
    out = torch.full((8192,), FILL, dtype=torch.uint8, device="cuda")        # [scratch 2048 | features 2048 | distances 2048 | spare]
    a = out.data_ptr()
    assert a % 8 == 0 and lib.distance_transform_scratch_bytes(e) <= 2048
    scratch, near, dist, v = a, a + 2048, a + 4096, vol.data_ptr()
    bad, unsupported, inf, nan = abi.VKV_E_INVALID_ARGUMENT, abi.VKV_E_UNSUPPORTED, float("inf"), float("nan")
    W = (2, 2, 5)
    rc = lambda *args: ctx.nearest_target_rc(*args, st())  # noqa: E731
    # the feature buffer and its partner
    assert rc(v, e, None, 0.5, 0, W, 5, scratch, None, dist) == bad and "d_nearest" in ctx.last_error()
    assert rc(v, e, None, 0.5, 0, W, 5, scratch, near + 2, dist) == bad and "d_nearest" in ctx.last_error()
    assert rc(v, e, None, 0.5, 0, W, 5, scratch, near, dist + 2) == bad and "aligned" in ctx.last_error()
    for other in (near, near + 4, near + 956, near - 956):        # 240 voxels: 960 bytes each
        assert rc(v, e, None, 0.5, 0, W, 5, scratch, near, other) == bad and "overlap" in ctx.last_error()
    # the weights
    assert rc(v, e, None, 0.5, 0, None, 5, scratch, near, dist) == bad and "weight" in ctx.last_error()
    for zero in ((0, 2, 5), (2, 0, 5), (2, 2, 0)):
        assert rc(v, e, None, 0.5, 0, zero, 5, scratch, near, dist) == bad and "weight" in ctx.last_error()
    assert rc(v, abi.Extent3D(12, 1, 4), None, 0.5, 0, (2, 0, 5), 5, scratch, near, dist) == bad        # on an axis of length 1 as well
    assert rc(v, e, None, 0.5, 0, (5958, 1, 1), 5, scratch, near, dist) == unsupported and "weights" in ctx.last_error()        # 5958 x 11 = 65538
    assert rc(v, e, None, 0.5, 0, (1, 16384, 1), 5, scratch, near, dist) == unsupported
    assert rc(v, e, None, 0.5, 0, (4000, 12000, 11000), 5, scratch, near, dist) == unsupported
    assert rc(v, abi.Extent3D(32768, 2, 2), None, 0.5, 0, (2, 363, 362), 5, scratch, near, dist) == unsupported
    assert rc(v, abi.Extent3D(32768, 1, 1), None, 0.5, 0, (3, 1, 1), 5, scratch, near, dist) == unsupported
    # each rejection of the weighted call, with and without d_dist2
    for dd in (dist, None):
        assert rc(None, e, None, 0.5, 0, W, 5, scratch, near, dd) == bad
        assert rc(v, e, None, 0.5, 0, W, 5, None, near, dd) == bad
        assert rc(v, abi.Extent3D(w, 0, d), None, 0.5, 0, W, 5, scratch, near, dd) == bad
        for iso in (inf, -inf, nan):
            assert rc(v, e, None, iso, 0, W, 5, scratch, near, dd) == bad and "iso" in ctx.last_error()
        for target in (-1, 2, 6):
            assert rc(v, e, None, 0.5, target, W, 5, scratch, near, dd) == bad and "target" in ctx.last_error()
        assert rc(v, e, None, 0.5, 0, W, 0, scratch, near, dd) == bad and "limit" in ctx.last_error()
        assert rc(v, e, abi.Box(0, 0, 0, 13, 2, 2), 0.5, 0, W, 5, scratch, near, dd) == bad and "box" in ctx.last_error()
        assert rc(v, e, abi.Box(11, 4, 3, 1, 2, 1), 0.5, 0, W, 5, scratch, near, dd) == bad
        assert rc(v, e, abi.Box(1, 1, 1, 2, 0, 2), 0.5, 0, W, 5, scratch, near, dd) == bad
        assert rc(v, e, None, 0.5, 0, W, 5, scratch + 4, near, dd) == bad and "aligned" in ctx.last_error()
        assert rc(v, abi.Extent3D(32768, 32768, 4), None, 0.5, 0, (1, 1, 1), 5, scratch, near, dd) == unsupported        # 2^32 voxels: one too many
        assert rc(v, abi.Extent3D(32769, 1, 1), None, 0.5, 0, (1, 1, 1), 5, scratch, near, dd) == unsupported        # an axis above 32768
        assert rc(v, abi.Extent3D(2, 2, 40000), None, 0.5, 0, (1, 1, 1), 5, scratch, near, dd) == unsupported
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((vol == 200).all())
    # the accepted neighbours write: d_dist2 right behind d_nearest, and the largest weight
    vol[0, 0, 0] = 17
    assert rc(v, e, None, 0.5, 1, (5957, 1, 1), None, scratch, near, near + 960) == abi.VKV_OK
    torch.cuda.synchronize()
    got = out[2048:2048 + 1920].view(torch.int32).cpu().numpy().view(np.uint32).reshape(2, d, h, w)
    assert (got[0] == 0).all() and int(got[1][3, 4, 11]) == 65527 ** 2 + 25 and bool((out[2048 + 1920:] == FILL).all())


# ---- vkv_propagate_labels -----------------------------------------------------------------------------------------------------------------
def propagate(ctx, nearest, labels, vol=None, mask_iso=0.0, box=None, extent=None, what=""):
    """d_out of ONE vkv_propagate_labels call on guarded buffers; vol: the mask volume (None: no mask)"""
    d_near, h_near = T.guarded(nearest.view(np.int32), 0, FILL, "cuda")
    d_lab, h_lab = T.guarded(labels.view(np.int32), 0, FILL, "cuda")
    d_out, h_out = T.guarded(nearest.shape, 0, FILL, "cuda", dtype=np.int32)
    d_vol, h_vol = (None, None) if vol is None else upload(vol)
    e = ext_of(vol) if extent is None else extent
    rc = ctx.propagate_labels_rc(d_near.data_ptr(), d_lab.data_ptr(), d_out.data_ptr(), e, None if box is None else abi.Box(*box),
                                 None if vol is None else d_vol.data_ptr(), mask_iso, st())
    assert rc == abi.VKV_OK, (what, rc, ctx.last_error())
    torch.cuda.synchronize()
    for name, h in (("d_nearest", h_near), ("d_labels", h_lab), ("d_out", h_out)) + ((("d_mask_volume", h_vol),) if vol is not None else ()):
        assert not guard_damage(h), "%s: %s: guard bytes changed" % (what, name)
    assert np.array_equal(d_near.cpu().numpy(), nearest.view(np.int32)) and np.array_equal(d_lab.cpu().numpy(), labels.view(np.int32)), what
    return d_out.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("extent", [(1, 1, 1), (5, 4, 3), (64, 3, 2), (257, 3, 2), (70, 66, 65)], ids=lambda e: "%dx%dx%d" % e)
def test_propagate_with_and_without_a_mask_none_entries_and_indices_out_of_range(ctx, extent):
    w, h, d = extent
    rng = np.random.default_rng(w * 1000 + h)
    n = w * h * d
    labels = rng.integers(0, 2 ** 32, size=(d, h, w), dtype=np.uint64).astype(np.uint32)        # any value is a label, 0xffffffff included
    nearest = rng.integers(0, n, size=(d, h, w)).astype(np.uint32)
    kind = rng.integers(0, 5, size=(d, h, w))
    nearest[kind == 0] = NONE
    nearest[kind == 1] = n        # the first index out of range
    nearest[(kind == 2) & (rng.random((d, h, w)) < 0.5)] = 0xfffffffe
    vol = contents("random 0.5", (d, h, w), seed=5)
    same(propagate(ctx, nearest, labels, extent=abi.Extent3D(w, h, d)), propagate_labels_np(nearest, labels), "%s: no mask" % (extent,))
    for iso in (ISO, 0.0, 1.0):
        same(propagate(ctx, nearest, labels, vol, iso), propagate_labels_np(nearest, labels, inside_np(vol, iso)), "%s: mask at %s" % (extent, iso))


def test_propagate_in_a_box_reads_the_masks_voxels_of_the_box(ctx, box_volume):
    rng = np.random.default_rng(3)
    mask_vol = contents("random 0.5", box_volume.shape, seed=8)
    for name in ("across tiles", "face x1", "width 1", "height 1", "corner 1"):
        b = BOXES[name]
        x0, y0, z0, w, h, d = b
        nearest = rng.integers(0, w * h * d, size=(d, h, w)).astype(np.uint32)
        labels = rng.integers(1, 1000, size=(d, h, w)).astype(np.uint32)
        inside = inside_np(mask_vol, ISO)[z0:z0 + d, y0:y0 + h, x0:x0 + w]
        same(propagate(ctx, nearest, labels, mask_vol, ISO, box=b), propagate_labels_np(nearest, labels, inside), "box %s" % name)
        same(propagate(ctx, nearest, labels, box=b, extent=ext_of(mask_vol)), propagate_labels_np(nearest, labels), "box %s, no mask" % name)


def test_propagate_rejected_calls_write_nothing(ctx):
    w, h, d = 12, 5, 4
    e = abi.Extent3D(w, h, d)
    vol = torch.full((d, h, w), 200, dtype=torch.uint8, device="cuda")
    buf = torch.full((8192,), FILL, dtype=torch.uint8, device="cuda")        # [nearest 2048 | labels 2048 | out 2048 | spare]
    a = buf.data_ptr()
    near, lab, out, v = a, a + 2048, a + 4096, vol.data_ptr()
    bad, unsupported = abi.VKV_E_INVALID_ARGUMENT, abi.VKV_E_UNSUPPORTED
    rc = lambda *args: ctx.propagate_labels_rc(*args, st())  # noqa: E731
    assert rc(None, lab, out, e, None, v, 0.5) == bad and rc(near, None, out, e, None, v, 0.5) == bad and rc(near, lab, None, e, None, v, 0.5) == bad
    assert rc(near, lab, out, abi.Extent3D(w, 0, d), None, v, 0.5) == bad
    for box in (abi.Box(0, 0, 0, 13, 2, 2), abi.Box(11, 4, 3, 1, 2, 1), abi.Box(1, 1, 1, 2, 0, 2)):
        assert rc(near, lab, out, e, box, v, 0.5) == bad and "box" in ctx.last_error()
    for k in range(3):
        ptrs = [near, lab, out]
        ptrs[k] += 2
        assert rc(*ptrs, e, None, v, 0.5) == bad and "aligned" in ctx.last_error()
    for iso in (float("inf"), float("nan")):
        assert rc(near, lab, out, e, None, v, iso) == bad and "mask_iso" in ctx.last_error()
    # every overlap of d_out with an input: equal, one element in, the last element from either side (240 voxels: 960 bytes)
    for o in (near, near + 4, near + 956, near - 956, lab, lab + 4, lab + 956, lab - 956):
        assert rc(near, lab, o, e, None, None, 0.0) == bad and "overlap" in ctx.last_error()
    assert rc(near, lab, out, abi.Extent3D(32768, 32768, 4), None, None, 0.0) == unsupported        # 2^32 voxels: one too many
    torch.cuda.synchronize()
    assert bool((buf == FILL).all())
    # the accepted neighbours: d_out right behind d_nearest; d_nearest and d_labels may be one array
    buf[:960].view(torch.int32).fill_(7)
    assert rc(near, near, near + 960, e, None, None, 0.0) == abi.VKV_OK
    torch.cuda.synchronize()
    assert bool((buf[960:1920].view(torch.int32) == 7).all()) and bool((buf[2048:] == FILL).all())


# ---- Volume.nearest_target / expand_labels / split_bodies -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    return {"bridge": bridge_scene()[0], "random 0.5": contents("random 0.5", (31, 26, 37), seed=4)}


@pytest.mark.parametrize("scene", ["bridge", "random 0.5"], ids=lambda s: s.replace(" ", "_"))
def test_volume_nearest_target_and_expand_labels_against_the_numpy_statements(ctx, scenes, scene):
    from scipy import ndimage
    vol = scenes[scene]
    v = make_volume(ctx, vol, block=2, packed=False)
    for to, target in (("inside", TO_INSIDE), ("outside", TO_OUTSIDE)):
        for weights, limit in ((None, None), ((2, 2, 5), 30)):
            got_n, got_d = v.nearest_target(ISO, to=to, limit=limit, weights=weights, distance=True)
            assert got_n.dtype == torch.uint32 and got_d.dtype == torch.uint32 and tuple(got_n.shape) == vol.shape
            want_n, want_d = nearest_separable_np(vol, ISO, weights or (1, 1, 1), target, limit)
            same(got_n.cpu().numpy(), want_n, "Volume.nearest_target to %s, weights %s" % (to, weights))
            same(got_d.cpu().numpy(), want_d, "Volume.nearest_target to %s, weights %s: dist2" % (to, weights))
            same(v.nearest_target(ISO, to=to, limit=limit, weights=weights).cpu().numpy(), want_n, "distance=False")
            same(got_d.cpu().numpy(), v.distance_transform(ISO, to=to, limit=limit, weights=weights or (1, 1, 1)).cpu().numpy(), "Volume.distance_transform")
    labels, _, counts = v.label_components(ISO, sizes=False)
    want_labels = ndimage.label(vol >= 128)[0].astype(np.uint32)
    same(labels.cpu().numpy(), want_labels, "the labels")
    mask_vol = contents("random 0.5", vol.shape, seed=6)
    mask = make_volume(ctx, mask_vol, block=2, packed=False)
    for r2, weights in ((2, None), (None, None), (29, (2, 2, 5))):
        same(v.expand_labels(labels, ISO, radius2=r2, weights=weights).cpu().numpy(), expand_labels_np(vol, ISO, want_labels, r2, weights),
             "Volume.expand_labels(radius2=%s, weights=%s)" % (r2, weights))
        same(v.expand_labels(labels, ISO, radius2=r2, weights=weights, mask=mask).cpu().numpy(),
             expand_labels_np(vol, ISO, want_labels, r2, weights, inside_np(mask_vol, ISO)), "Volume.expand_labels(radius2=%s, mask)" % r2)
    same(v.expand_labels(labels, ISO, radius=1.5).cpu().numpy(), expand_labels_np(vol, ISO, want_labels, 2), "radius 1.5 is radius2 2")
    same(v.expand_labels(labels, ISO, radius2=2, mask=mask, mask_iso=0.05).cpu().numpy(),
         expand_labels_np(vol, ISO, want_labels, 2, None, inside_np(mask_vol, 0.05)), "mask_iso")
    same(v.volume.cpu().numpy(), vol, "the volume itself")


@pytest.mark.parametrize("scene", ["bridge", "random 0.5"], ids=lambda s: s.replace(" ", "_"))
def test_volume_split_bodies_against_scipy_and_its_stats_against_sum_labels(ctx, scenes, scene):
    from scipy import ndimage
    vol = scenes[scene]
    v = make_volume(ctx, vol, block=2, packed=False)
    for r2, connectivity, weights in ((2, 6, None), (4, 6, None), (2, 26, None), (4, 6, (1, 1, 2))):
        labels, counts = v.split_bodies(ISO, radius2=r2, connectivity=connectivity, weights=weights)
        want, k = split_bodies_np(vol, ISO, r2, connectivity, weights)
        what = "Volume.split_bodies(radius2=%d, connectivity=%d, weights=%s) on %s" % (r2, connectivity, weights, scene)
        assert labels.dtype == torch.uint32 and int(counts[0].item()) == k, what
        same(labels.cpu().numpy(), want, what)
        if k:
            assert np.array_equal(want != 0, vol >= 128), what        # every inside voxel got a label
            stats = v.component_stats(labels, counts)
            index = np.arange(1, k + 1)
            assert np.array_equal(stats.voxels.cpu().numpy().astype(np.int64), ndimage.sum_labels(np.ones(vol.shape, np.int64), want, index).astype(np.int64)), what
            sums = ndimage.sum_labels(vol.astype(np.float64), want, index)
            assert np.array_equal(np.rint(stats.mean.cpu().numpy() * stats.voxels.cpu().numpy()), sums), what        # sums of bytes: integers below 2^53
    if scene == "bridge":
        labels, counts = v.split_bodies(ISO, radius=2)
        assert int(counts[0].item()) == 2 and int(v.label_components(ISO, sizes=False)[2][0].item()) == 1        # one body, split in two
        sizes = v.component_stats(labels, counts, values=False).voxels.cpu().numpy()
        assert sizes[0] == sizes[1] == (vol >= 128).sum() // 2
    same(v.volume.cpu().numpy(), vol, "the volume itself")
