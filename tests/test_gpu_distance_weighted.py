"""GPU: vkv_distance_transform_weighted bit for bit against edt2_weighted_np of tests/test_distance_weighted_cpu.py, with
weights (1, 1, 1) also against vkv_distance_transform itself, and Volume.erode / dilate / open / close with weights against scipy.ndimage.

The x pass is k_edt_x's walk with a weight; the y and z passes give every line of the box to one lane, which builds the lower envelope of
the line's parabolas as a stack IN the line of the output buffer and then overwrites it from the far end.  The extents are those of
tests/test_gpu_distance.py: axes of length 1 (their pass is not launched, so the x pass starts in either buffer), widths below a wave and
around one and two words (lanes of one wave then own lines of several slices), 200-voxel needles along each axis (long stacks), 70x66x65
(several workgroups per pass), and 32768 along each axis, the longest line and the largest values the call accepts.  Contents: "above" pushes
every position of every line (a full stack); a single corner target leaves most lines all cap (no entry at all) and the others with one
entry; a ball under weights 1 : 1 : 255 gives envelopes along z on which one parabola survives; random 0.5 pops all the time.  The
reference of a limited call is min(limit, the unlimited reference): the definition.  Every buffer is a tests/helpers.py guarded()
allocation, pre-filled and compared as a whole; the scratch is exactly vkv_distance_transform_scratch_bytes."""
import numpy as np
import pytest
import torch

from tests import helpers as T
from tests.test_distance_cpu import NONE, TO_INSIDE, TO_OUTSIDE, edt2_np
from tests.test_distance_weighted_cpu import edt2_weighted_np
from tests.test_gpu_components import same
from tests.test_gpu_distance import CONTENTS, EXTENTS, LIMITS, LONG_CONTENTS, LONGEST, cap, contents, run as run_unweighted, upload
from tests.test_gpu_mesh import BOX_VOLUME, BOXES, FILL, ISO, ext_of, st
from tests.test_gpu_mesh_indexed import guard_damage
from tests.test_gpu_mip import make_volume
from vkvolume_amd import abi, lib

pytestmark = pytest.mark.gpu

TARGETS = (TO_INSIDE, TO_OUTSIDE)
WEIGHTS = ((2, 2, 5), (5, 2, 2), (3, 7, 1), (1, 1, 255))
WEIGHTED_CONTENTS = ("below", "above", "corner 0", "corner 7", "centre", "slice x", "slice y", "slice z", "random 0.001", "random 0.5", "ball")


def weighted_limits(weights):
    return (None, 1, min(weights) ** 2, 10, 100000)


@pytest.fixture(scope="module")
def ctx():
    torch.cuda.set_device(0)
    c = lib.Context(0)
    yield c
    c.close()


# ---- one call ---------------------------------------------------------------------------------------------------------------------------
def run(ctx, vol, iso, target, weights, limit, box=None, device_volume=None, what=""):
    """d_dist2 (the whole buffer, the box's shape, uint32) of ONE vkv_distance_transform_weighted call on guarded buffers, every output and
    the scratch pre-filled with FILL; the scratch is the unweighted call's"""
    abox = None if box is None else abi.Box(*box)
    shape = vol.shape if box is None else (box[5], box[4], box[3])
    n = int(np.prod(shape))
    d_vol, h_vol = upload(vol) if device_volume is None else device_volume
    nbytes = lib.distance_transform_scratch_bytes(ext_of(vol), abox)
    assert nbytes == 4 * n + 8 * ((n + 63) // 64), (what, nbytes)
    d_scratch, h_scratch = T.guarded(((nbytes + 7) // 8,), 0, FILL, "cuda", dtype=np.int64)
    d_dist, h_dist = T.guarded(shape, 0, FILL, "cuda", dtype=np.int32)
    rc = ctx.distance_transform_weighted_rc(d_vol.data_ptr(), ext_of(vol), abox, iso, target, weights, limit, d_scratch.data_ptr(), d_dist.data_ptr(), st())
    assert rc == abi.VKV_OK, (what, rc, ctx.last_error())
    torch.cuda.synchronize()
    for name, h in (("d_volume", h_vol), ("d_scratch", h_scratch), ("d_dist2", h_dist)):
        bad = guard_damage(h)
        assert not bad, "%s: %s: guard bytes %s changed (payload is bytes %d .. %d)" % (what, name, bad[:8], h.start, h.stop - 1)
    if nbytes % 8:        # the scratch block ends 4 bytes before the allocation's payload does: they are not the call's to write
        assert (d_scratch.view(torch.uint8)[nbytes:].cpu().numpy() == FILL).all(), "%s: bytes past the scratch block changed" % what
    assert np.array_equal(d_vol.cpu().numpy(), vol), "%s: the volume changed" % what
    return d_dist.cpu().numpy().view(np.uint32)


def check_weighted(ctx, vol, weights, iso=ISO, limits=None, box=None, what="", **kw):
    device_volume = upload(vol, **kw)
    for target in TARGETS:
        unlimited = edt2_weighted_np(vol, iso, weights, target, None, box)
        for limit in weighted_limits(weights) if limits is None else limits:
            w = "%s, weights %s, to %s, limit %s" % (what, weights, ("inside", "outside")[target], limit)
            same(run(ctx, vol, iso, target, weights, limit, box=box, device_volume=device_volume, what=w), cap(unlimited, limit), w)


# ---- weights (1, 1, 1): the unweighted call's bytes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", EXTENTS, ids=lambda e: "%dx%dx%d" % e)
def test_unit_weights_give_the_unweighted_calls_bytes(ctx, extent):
    w, h, d = extent
    for k, content in enumerate(CONTENTS):
        vol = contents(content, (d, h, w), seed=500 + k)
        device_volume = upload(vol)
        for target in TARGETS:
            unlimited = edt2_np(vol, ISO, target)
            for limit in LIMITS:
                what = "%s %s, to %s, limit %s" % (content, extent, ("inside", "outside")[target], limit)
                got = run(ctx, vol, ISO, target, (1, 1, 1), limit, device_volume=device_volume, what=what)
                same(got, cap(unlimited, limit), what + ": the statement")
                same(got, run_unweighted(ctx, vol, ISO, target, limit, device_volume=device_volume, what=what), what + ": vkv_distance_transform")


# ---- weights ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", EXTENTS, ids=lambda e: "%dx%dx%d" % e)
def test_every_extent_content_target_and_limit_with_weights(ctx, extent):
    w, h, d = extent
    for weights in WEIGHTS:
        for k, content in enumerate(WEIGHTED_CONTENTS):
            vol = contents(content, (d, h, w), seed=900 + k)
            if content == "corner 7":
                far = sum((a * (n - 1)) ** 2 for a, n in zip(weights, extent))
                assert int(edt2_weighted_np(vol, ISO, weights, TO_INSIDE)[0, 0, 0]) == far
            check_weighted(ctx, vol, weights, what="%s %s" % (content, extent))


@pytest.mark.parametrize("content", WEIGHTED_CONTENTS, ids=lambda c: c.replace(" ", "_"))
@pytest.mark.parametrize("weights", WEIGHTS, ids=lambda w: "%d_%d_%d" % w)
def test_every_axis_longer_than_a_word_with_weights(ctx, weights, content):
    w, h, d = 70, 66, 65
    vol = contents(content, (d, h, w), seed=41)
    check_weighted(ctx, vol, weights, what="%s 70x66x65" % content)


# ---- the longest axis -------------------------------------------------------------------------------------------------------------------
def long_weights(axis):
    """(weights, the farthest value): 1 on the long axis beside (200, 300), and 2 beside (362, 362): 4 294 967 244, the largest value
    the call accepts on such a box"""
    for on_axis, others in ((1, (200, 300)), (2, (362, 362))):
        weights = list(others)
        weights.insert(axis, on_axis)
        yield tuple(weights), (on_axis * (LONGEST - 1)) ** 2 + others[0] ** 2 + others[1] ** 2


@pytest.mark.parametrize("content", sorted(LONG_CONTENTS), ids=lambda c: c.replace(" ", "_"))
@pytest.mark.parametrize("axis", [0, 1, 2], ids=["x", "y", "z"])
def test_an_axis_of_32768_voxels_with_weights(ctx, axis, content):
    """the reference is the definition in 64-bit integers: the minimum over the targets (at the far corners) of the weighted sum, capped.
    To the outside, the volume is the inverted one"""
    extent = [2, 2, 2]
    extent[axis] = LONGEST
    w, h, d = extent
    corners = [((d - 1) * (k >> 2 & 1), (h - 1) * (k >> 1 & 1), (w - 1) * (k & 1)) for k in LONG_CONTENTS[content]]
    z, y, x = (a.astype(np.uint64) for a in np.indices((d, h, w), sparse=True))
    for weights, farthest in long_weights(axis):
        assert farthest <= 0xfffffffe and (weights[axis] == 1 or farthest == 4294967244)
        sq = lambda a, c, wa: (np.uint64(wa) * np.where(a > c, a - np.uint64(c), np.uint64(c) - a)) ** 2  # noqa: E731
        exact = np.full((d, h, w), 2 ** 64 - 1, np.uint64)
        for cz, cy, cx in corners:
            exact = np.minimum(exact, sq(z, cz, weights[2]) + sq(y, cy, weights[1]) + sq(x, cx, weights[0]))
        if len(corners) == 1:
            assert int(exact.max()) == farthest        # the far corner
        for target in TARGETS:
            vol = np.full((d, h, w), 17 if target == TO_INSIDE else 200, np.uint8)
            for c in corners:
                vol[c] = 200 if target == TO_INSIDE else 17
            device_volume = upload(vol)
            for limit in (None, farthest - 1, farthest, farthest + 1, 0xfffffffe):
                want = np.minimum(exact, np.uint64(NONE if limit is None else limit)).astype(np.uint32)
                what = "%s %s, weights %s, to %s, limit %s" % (content, tuple(extent), weights, ("inside", "outside")[target], limit)
                same(run(ctx, vol, ISO, target, weights, limit, device_volume=device_volume, what=what), want, what)


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
        want = edt2_weighted_np(crop, ISO, weights, target)        # nothing beyond the box exists
        for limit in (None, 30):
            got = run(ctx, box_volume, ISO, target, weights, limit, box=b, what="box %s" % box)
            assert got.shape == (d, h, w)
            same(got, cap(want, limit), "box %s, to %s, limit %s" % (box, target, limit))


@pytest.mark.parametrize("extent", [(7, 3, 3), (131, 3, 2)], ids=lambda e: "%dx%dx%d" % e)
def test_every_volume_alignment_with_both_guard_fills(ctx, extent):
    """a result that consumed a guard byte as a voxel differs under one of the two fills"""
    w, h, d = extent
    vol = contents("random 0.1", (d, h, w), seed=77)
    for fill in (0x00, 0xFF):
        for offset in (0, 1, 2, 3):
            check_weighted(ctx, vol, (2, 2, 5), limits=(None, 8), offset=offset, fill=fill, what="%s, volume +%d fill %#x" % (extent, offset, fill))


# ---- determinism and capture ------------------------------------------------------------------------------------------------------------
def test_two_runs_on_the_same_buffers_give_identical_bytes(ctx):
    vol = contents("random 0.01", (19, 5, 258), seed=21)
    d_vol = torch.from_numpy(vol).cuda()
    n = lib.distance_transform_scratch_bytes(ext_of(vol))
    d_scratch = torch.full(((n + 7) // 8,), -1, dtype=torch.int64, device="cuda")
    for target in TARGETS:
        for limit in (None, 30):
            d_dist = torch.full(vol.shape, -1, dtype=torch.int32, device="cuda")
            results = []
            for _ in range(2):        # the second run starts from the first run's distances and scratch: stale stack entries in both buffers
                ctx.check(ctx.distance_transform_weighted_rc(d_vol.data_ptr(), ext_of(vol), None, ISO, target, (3, 7, 1), limit, d_scratch.data_ptr(),
                                                             d_dist.data_ptr(), st()))
                torch.cuda.synchronize()
                results.append(d_dist.cpu().numpy().view(np.uint32))
            assert np.array_equal(results[0], results[1])
            same(results[1], edt2_weighted_np(vol, ISO, (3, 7, 1), target, limit), "second run")


def test_transform_and_select_captured_into_a_graph_replay(ctx):
    shape = (17, 9, 131)
    weights, r2 = (2, 2, 5), 29
    vol = contents("random 0.05", shape, seed=13)
    d_vol = torch.from_numpy(vol).cuda()
    d_out = torch.empty_like(d_vol)
    d_scratch = torch.empty(((lib.distance_transform_scratch_bytes(ext_of(vol)) + 7) // 8,), dtype=torch.int64, device="cuda")
    d_dist = torch.empty(shape, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()

    def call():        # a dilation by radius^2 29 in weighted units
        ctx.check(ctx.distance_transform_weighted_rc(d_vol.data_ptr(), ext_of(vol), None, ISO, TO_INSIDE, weights, r2 + 1, d_scratch.data_ptr(), d_dist.data_ptr(),
                                                     s.cuda_stream))
        ctx.select_by_distance(d_vol.data_ptr(), d_out.data_ptr(), ext_of(vol), None, d_dist.data_ptr(), 1, r2, 255, s.cuda_stream)

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
        d_dist.view(torch.uint8).fill_(FILL)
        d_out.fill_(FILL)
        d_scratch.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        want = edt2_weighted_np(vol, ISO, weights, TO_INSIDE, r2 + 1)
        same(d_dist.cpu().numpy().view(np.uint32), want, "replay, seed %d: distances" % seed)
        dilated = vol.copy()
        dilated[(want >= 1) & (want <= r2)] = 255
        same(d_out.cpu().numpy(), dilated, "replay, seed %d: the dilated volume" % seed)


# ---- rejected calls ---------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_write_nothing(ctx):
    w, h, d = 12, 5, 4
    e = abi.Extent3D(w, h, d)
    vol = torch.full((d, h, w), 200, dtype=torch.uint8, device="cuda")
    out = torch.full((8192,), FILL, dtype=torch.uint8, device="cuda")        # [scratch 2048 | distances 2048 | spare]
    a = out.data_ptr()
    assert a % 8 == 0 and lib.distance_transform_scratch_bytes(e) <= 2048
    scratch, dist, v = a, a + 2048, vol.data_ptr()
    bad, unsupported, inf, nan = abi.VKV_E_INVALID_ARGUMENT, abi.VKV_E_UNSUPPORTED, float("inf"), float("nan")
    W = (2, 2, 5)
    rc = lambda *args: ctx.distance_transform_weighted_rc(*args, st())  # noqa: E731
    # the weights
    assert rc(v, e, None, 0.5, 0, None, 5, scratch, dist) == bad and "weight" in ctx.last_error()
    for zero in ((0, 2, 5), (2, 0, 5), (2, 2, 0)):
        assert rc(v, e, None, 0.5, 0, zero, 5, scratch, dist) == bad and "weight" in ctx.last_error()
    assert rc(v, abi.Extent3D(12, 1, 4), None, 0.5, 0, (2, 0, 5), 5, scratch, dist) == bad        # on an axis of length 1 as well
    # the largest value: (11 wx)^2 + 4^2 + 3^2 with wx = 5957 is 65527^2 + 25; 5958 x 11 = 65538 is past 65535
    assert rc(v, e, None, 0.5, 0, (5958, 1, 1), 5, scratch, dist) == unsupported and "weights" in ctx.last_error()
    assert rc(v, e, None, 0.5, 0, (1, 16384, 1), 5, scratch, dist) == unsupported        # 4 x 16384 = 65536
    assert rc(v, e, None, 0.5, 0, (4000, 12000, 11000), 5, scratch, dist) == unsupported        # each axis fits, 44000^2 + 48000^2 + 33000^2 does not
    assert rc(v, abi.Extent3D(32768, 2, 2), None, 0.5, 0, (2, 363, 362), 5, scratch, dist) == unsupported        # 4 294 967 969: the bound exceeded
    assert rc(v, abi.Extent3D(32768, 1, 1), None, 0.5, 0, (3, 1, 1), 5, scratch, dist) == unsupported
    # each rejection of the unweighted call
    assert rc(None, e, None, 0.5, 0, W, 5, scratch, dist) == bad
    assert rc(v, e, None, 0.5, 0, W, 5, None, dist) == bad
    assert rc(v, e, None, 0.5, 0, W, 5, scratch, None) == bad
    assert rc(v, abi.Extent3D(w, 0, d), None, 0.5, 0, W, 5, scratch, dist) == bad
    for iso in (inf, -inf, nan):
        assert rc(v, e, None, iso, 0, W, 5, scratch, dist) == bad and "iso" in ctx.last_error()
    for target in (-1, 2, 6):
        assert rc(v, e, None, 0.5, target, W, 5, scratch, dist) == bad and "target" in ctx.last_error()
    assert rc(v, e, None, 0.5, 0, W, 0, scratch, dist) == bad and "limit" in ctx.last_error()
    assert rc(v, e, abi.Box(0, 0, 0, 13, 2, 2), 0.5, 0, W, 5, scratch, dist) == bad and "box" in ctx.last_error()
    assert rc(v, e, abi.Box(11, 4, 3, 1, 2, 1), 0.5, 0, W, 5, scratch, dist) == bad
    assert rc(v, e, abi.Box(1, 1, 1, 2, 0, 2), 0.5, 0, W, 5, scratch, dist) == bad
    assert rc(v, e, None, 0.5, 0, W, 5, scratch + 4, dist) == bad and "aligned" in ctx.last_error()
    assert rc(v, e, None, 0.5, 0, W, 5, scratch, dist + 2) == bad
    assert rc(v, abi.Extent3D(32768, 32768, 4), None, 0.5, 0, (1, 1, 1), 5, scratch, dist) == unsupported        # 2^32 voxels: one too many
    assert rc(v, abi.Extent3D(32769, 1, 1), None, 0.5, 0, (1, 1, 1), 5, scratch, dist) == unsupported        # an axis above 32768
    assert rc(v, abi.Extent3D(2, 2, 40000), None, 0.5, 0, (1, 1, 1), 5, scratch, dist) == unsupported
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((vol == 200).all())


def test_rejected_calls_leave_every_byte_and_the_accepted_neighbours_write(ctx):
    w, h, d = 12, 5, 4
    e = abi.Extent3D(w, h, d)
    vol = torch.full((d, h, w), 200, dtype=torch.uint8, device="cuda")
    vol[0, 0, 0] = 17
    out = torch.full((8192,), FILL, dtype=torch.uint8, device="cuda")
    a = out.data_ptr()
    scratch, dist, v = a, a + 2048, vol.data_ptr()
    rc = lambda *args: ctx.distance_transform_weighted_rc(*args, st())  # noqa: E731
    for weights in (None, (0, 1, 1), (5958, 1, 1), (4000, 12000, 11000)):
        assert rc(v, e, None, 0.5, 1, weights, None, scratch, dist) != abi.VKV_OK
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    # the accepted neighbour of (5958, 1, 1): the far corner's distance to the one outside voxel is 65527^2 + 4^2 + 3^2
    assert rc(v, e, None, 0.5, 1, (5957, 1, 1), None, scratch, dist) == abi.VKV_OK
    torch.cuda.synchronize()
    got = out[2048:2048 + 960].view(torch.int32).cpu().numpy().view(np.uint32).reshape(d, h, w)
    assert int(got[3, 4, 11]) == 65527 ** 2 + 25 and int(got[0, 0, 0]) == 0 and bool((out[2048 + 960:4096] == FILL).all()) and bool((out[4096:] == FILL).all())
    same(got, edt2_weighted_np(vol.cpu().numpy(), 0.5, (5957, 1, 1), TO_OUTSIDE), "weights (5957, 1, 1)")


# ---- Volume.erode / dilate / open / close with weights ------------------------------------------------------------------------------------
def weighted_ball(weights, r2):
    """the offsets (kz, ky, kx) with sum (w_a k_a)^2 <= r2 as a scipy structure [2 rz + 1, 2 ry + 1, 2 rx + 1]"""
    rx, ry, rz = (int(np.floor(np.sqrt(r2))) // a for a in weights)
    z, y, x = np.meshgrid(np.arange(-rz, rz + 1), np.arange(-ry, ry + 1), np.arange(-rx, rx + 1), indexing="ij")
    return (weights[0] * x) ** 2 + (weights[1] * y) ** 2 + (weights[2] * z) ** 2 <= r2


def test_volume_morphology_with_weights_against_scipy(ctx):
    from scipy import ndimage
    field = ndimage.gaussian_filter(np.random.default_rng(4).random((31, 26, 37)), 1.5)
    blobs = np.where(field > np.median(field), 200, 17).astype(np.uint8)
    weights = (2, 2, 5)
    v = make_volume(ctx, blobs, block=2, packed=False)
    inside = blobs >= 128
    for to, target in (("inside", TO_INSIDE), ("outside", TO_OUTSIDE)):
        for limit in (None, 30):
            got = v.distance_transform(ISO, to=to, limit=limit, weights=weights)
            assert got.dtype == torch.uint32 and tuple(got.shape) == blobs.shape
            same(got.cpu().numpy(), edt2_weighted_np(blobs, ISO, weights, target, limit), "Volume.distance_transform(weights) to %s, limit %s" % (to, limit))
    same(v.distance_transform(ISO, weights=(1, 1, 1)).cpu().numpy(), v.distance_transform(ISO).cpu().numpy(), "weights (1, 1, 1) and None")
    assert weighted_ball(weights, 4).sum() == 5 and weighted_ball(weights, 25).shape == (3, 5, 5) and weighted_ball(weights, 29).sum() == 21 + 2 * 5
    for r2 in (4, 25, 29, 100):
        ball = weighted_ball(weights, r2)
        eroded, dilated = ndimage.binary_erosion(inside, structure=ball, border_value=1), ndimage.binary_dilation(inside, structure=ball)
        opened = ndimage.binary_dilation(eroded, structure=ball)
        closed = ndimage.binary_erosion(dilated, structure=ball, border_value=1)
        assert (eroded != inside).any() and (dilated != inside).any()
        for name, mask in (("erode", eroded), ("dilate", dilated), ("open", opened), ("close", closed)):
            out = getattr(v, name)(ISO, radius2=r2, weights=weights)
            assert out.dtype == torch.uint8 and out.data_ptr() != v.volume.data_ptr() and tuple(out.shape) == blobs.shape
            assert np.array_equal(out.cpu().numpy() >= 128, mask), "Volume.%s(radius2=%d, weights) against scipy" % (name, r2)
            inplace = make_volume(ctx, blobs, block=2, packed=False)
            assert getattr(inplace, name)(ISO, radius2=r2, weights=weights, out=inplace.volume) is inplace.volume
            same(inplace.volume.cpu().numpy(), out.cpu().numpy(), "Volume.%s(radius2=%d, weights) in place" % (name, r2))
    same(v.volume.cpu().numpy(), blobs, "the volume itself")
    same(v.erode(ISO, radius=5, weights=weights).cpu().numpy(), v.erode(ISO, radius2=25, weights=weights).cpu().numpy(), "radius 5 is radius2 25")
    assert (v.erode(ISO, radius2=25, weights=weights).cpu().numpy() != v.erode(ISO, radius2=25).cpu().numpy()).any()
    with pytest.raises(ValueError):
        v.erode(ISO, radius2=4, weights=(2, 2, 0))
    with pytest.raises(lib.VkvError):
        v.distance_transform(ISO, weights=(3000, 1, 1))        # 3000 x 36 is past 65535
