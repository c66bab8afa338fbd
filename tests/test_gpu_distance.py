"""GPU: vkv_distance_transform and vkv_select_by_distance bit for bit against the numpy statements of
tests/test_distance_cpu.py (edt2_np, select_by_distance_np), and Volume.erode / dilate / open / close against scipy.ndimage.

The kernels are one-dimensional over the box-linear voxel index: a wave's 64 consecutive voxels are one ENTRY with one 64-bit word of
target bits (it wraps over rows where the box's width is no multiple of 64); the x pass walks words outward along the row, the y and z passes
look d voxels up and down their line while d^2 is below the best value so far; a workgroup holds four entries.  The extents:
  those of tests/test_gpu_components.py   axes of length 1 (their pass is not launched: one, two or three passes, so the first pass starts in
                                          either buffer), fewer voxels than a wave, one short of, at and one past one and two words along
                                          x, around one workgroup, narrow boxes whose entries wrap rows and slices;
  200x3x2, 3x200x2, 2x3x200             long walks along each axis, over several words along x;
  70x66x65                              every axis longer than a word, several workgroups per slice;
  32768x2x2, 2x32768x2, 2x2x32768       the longest axis the call accepts, with the limits around 32767^2 (closed-form references).
Contents: no target and all target; ONE target voxel at each corner and at the centre (most rows and columns then carry "none", the cap,
and every offset up to the full diagonal is added to it: the overflow case); one full slice per axis; random at 0.001, 0.1, 0.5 and 0.9; a
ball; the 3-D checkerboard.  Both targets; limits NONE, 1, 2, 9, 10 and 100000.  The reference of a limited call is min(limit, the unlimited
reference): the definition.  Every buffer is a tests/helpers.py guarded() allocation, pre-filled and compared as a whole, all guards and the
scratch guard must be intact and the volume unchanged, so nothing here relies on, or can cause, a fault."""
import numpy as np
import pytest
import torch

from tests import helpers as T
from tests.test_components_cpu import components_np, select_np
from tests.test_distance_cpu import NONE, TO_INSIDE, TO_OUTSIDE, ball_structure, dilate_np, edt2_np, erode_np, select_by_distance_np
from tests.test_gpu_components import EXTENTS as COMPONENT_EXTENTS, same
from tests.test_gpu_mesh import BOX_VOLUME, BOXES, FILL, ISO, ext_of, st
from tests.test_gpu_mesh_indexed import guard_damage
from tests.test_gpu_mip import make_volume
from tests.test_mesh_cpu import mesh_contents
from vkvolume_amd import abi, lib

pytestmark = pytest.mark.gpu

TARGETS = (TO_INSIDE, TO_OUTSIDE)
LIMITS = (None, 1, 2, 9, 10, 100000)
EXTENTS = COMPONENT_EXTENTS + [(200, 3, 2), (3, 200, 2), (2, 3, 200)]  # (width, height, depth)


@pytest.fixture(scope="module")
def ctx():
    torch.cuda.set_device(0)
    c = lib.Context(0)
    yield c
    c.close()


# ---- contents ---------------------------------------------------------------------------------------------------------------------------
def contents(kind, shape_dhw, seed=0):
    """bytes 200 (inside at ISO) and 17 (outside), but for the ball's ramp"""
    d, h, w = shape_dhw
    if kind in ("below", "above", "ball"):
        return mesh_contents(kind, shape_dhw, seed)
    vol = np.full(shape_dhw, 17, np.uint8)
    if kind.startswith("random"):
        return np.where(np.random.default_rng(seed).random(shape_dhw) < float(kind.split()[1]), 200, 17).astype(np.uint8)
    if kind == "checkerboard":
        z, y, x = np.indices(shape_dhw)
        return np.where((x + y + z) % 2 == 0, 255, 0).astype(np.uint8)
    if kind == "centre":
        vol[d // 2, h // 2, w // 2] = 200
    elif kind.startswith("corner"):
        k = int(kind.split()[1])
        vol[(d - 1) * (k >> 2 & 1), (h - 1) * (k >> 1 & 1), (w - 1) * (k & 1)] = 200
    elif kind == "slice x":
        vol[:, :, w // 3] = 200
    elif kind == "slice y":
        vol[:, h // 3, :] = 200
    elif kind == "slice z":
        vol[d // 3, :, :] = 200
    else:
        raise KeyError(kind)
    return vol


CONTENTS = (("below", "above", "centre") + tuple("corner %d" % k for k in range(8)) + ("slice x", "slice y", "slice z") +
            ("random 0.001", "random 0.1", "random 0.5", "random 0.9", "ball", "checkerboard"))


def cap(unlimited, limit):
    return unlimited if limit is None else np.minimum(unlimited, np.uint32(limit))


# ---- one call ---------------------------------------------------------------------------------------------------------------------------
def upload(vol, offset=0, fill=0x00):
    return T.guarded(vol, offset, fill, "cuda")


def run(ctx, vol, iso, target, limit, box=None, device_volume=None, what=""):
    """d_dist2 (the whole buffer, the box's shape, uint32) of ONE vkv_distance_transform call on guarded buffers, every output and the scratch
    pre-filled with FILL"""
    abox = None if box is None else abi.Box(*box)
    shape = vol.shape if box is None else (box[5], box[4], box[3])
    n = int(np.prod(shape))
    d_vol, h_vol = upload(vol) if device_volume is None else device_volume
    nbytes = lib.distance_transform_scratch_bytes(ext_of(vol), abox)
    assert nbytes == 4 * n + 8 * ((n + 63) // 64), (what, nbytes)
    d_scratch, h_scratch = T.guarded(((nbytes + 7) // 8,), 0, FILL, "cuda", dtype=np.int64)
    d_dist, h_dist = T.guarded(shape, 0, FILL, "cuda", dtype=np.int32)
    ctx.distance_transform(d_vol.data_ptr(), ext_of(vol), abox, iso, target, limit, d_scratch.data_ptr(), d_dist.data_ptr(), st())
    torch.cuda.synchronize()
    for name, h in (("d_volume", h_vol), ("d_scratch", h_scratch), ("d_dist2", h_dist)):
        bad = guard_damage(h)
        assert not bad, "%s: %s: guard bytes %s changed (payload is bytes %d .. %d)" % (what, name, bad[:8], h.start, h.stop - 1)
    if nbytes % 8:        # the scratch block ends 4 bytes before the allocation's payload does: they are not the call's to write
        assert (d_scratch.view(torch.uint8)[nbytes:].cpu().numpy() == FILL).all(), "%s: bytes past the scratch block changed" % what
    assert np.array_equal(d_vol.cpu().numpy(), vol), "%s: the volume changed" % what
    return d_dist.cpu().numpy().view(np.uint32)


def check_all_limits(ctx, vol, iso=ISO, limits=LIMITS, box=None, what="", **kw):
    device_volume = upload(vol, **kw)
    for target in TARGETS:
        unlimited = edt2_np(vol, iso, target, None, box)
        for limit in limits:
            w = "%s, to %s, limit %s" % (what, ("inside", "outside")[target], limit)
            same(run(ctx, vol, iso, target, limit, box=box, device_volume=device_volume, what=w), cap(unlimited, limit), w)


# ---- extents and contents ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", EXTENTS, ids=lambda e: "%dx%dx%d" % e)
def test_every_extent_content_target_and_limit(ctx, extent):
    w, h, d = extent
    for k, content in enumerate(CONTENTS):
        vol = contents(content, (d, h, w), seed=500 + k)
        if content == "below":
            assert (edt2_np(vol, ISO, TO_INSIDE) == NONE).all() and (edt2_np(vol, ISO, TO_OUTSIDE) == 0).all()
        if content == "corner 7":
            assert int(edt2_np(vol, ISO, TO_INSIDE)[0, 0, 0]) == (w - 1) ** 2 + (h - 1) ** 2 + (d - 1) ** 2
        check_all_limits(ctx, vol, what="%s %s" % (content, extent))


@pytest.mark.parametrize("content", ["below", "corner 0", "corner 7", "centre", "slice y", "random 0.001", "random 0.5", "ball"])
def test_every_axis_longer_than_a_word(ctx, content):
    w, h, d = 70, 66, 65
    vol = contents(content, (d, h, w), seed=41)
    check_all_limits(ctx, vol, what="%s 70x66x65" % content)


# ---- the longest axis -------------------------------------------------------------------------------------------------------------------
LONGEST = 32768        # edt.hip: axes up to 32768, dx * dx < 2^30, (d + 3)^2 < 2^31, reach <= 65536
FARTHEST = (LONGEST - 1) ** 2        # 1 073 676 289: the farthest row distance
LONG_LIMITS = (None, FARTHEST, FARTHEST + 1, FARTHEST + 2, 0xfffffffe)        # reach 32767: the row's end equals the cap; reach 32768; the far corner's
LONG_CONTENTS = {"corner 0": (0,), "corner 7": (7,), "corners 0 and 7": (0, 7), "no target": ()}        # distance 32767^2 + 1 + 1; the largest limit


@pytest.mark.parametrize("content", sorted(LONG_CONTENTS), ids=lambda c: c.replace(" ", "_"))
@pytest.mark.parametrize("extent", [(LONGEST, 2, 2), (2, LONGEST, 2), (2, 2, LONGEST)], ids=lambda e: "%dx%dx%d" % e)
def test_an_axis_of_32768_voxels(ctx, extent, content):
    """the longest axis the call accepts, along each axis in turn: targets at the two far corners, so that the largest offsets and their
    squares occur (and, without a target, every line is walked to its end); the reference is the definition in 64-bit integers: the minimum over
    the targets of the sum of the squared coordinate differences, capped.  To the outside, the volume is the inverted one"""
    w, h, d = extent
    corners = [((d - 1) * (k >> 2 & 1), (h - 1) * (k >> 1 & 1), (w - 1) * (k & 1)) for k in LONG_CONTENTS[content]]
    z, y, x = (a.astype(np.uint64) for a in np.indices((d, h, w), sparse=True))
    sq = lambda a, c: np.where(a > c, a - np.uint64(c), np.uint64(c) - a) ** 2  # noqa: E731
    exact = np.full((d, h, w), 2 ** 64 - 1, np.uint64)
    for cz, cy, cx in corners:
        exact = np.minimum(exact, sq(z, cz) + sq(y, cy) + sq(x, cx))
    if len(corners) == 1:
        assert int(exact.max()) == FARTHEST + 2        # the far corner
    for target in TARGETS:
        vol = np.full((d, h, w), 17 if target == TO_INSIDE else 200, np.uint8)
        for c in corners:
            vol[c] = 200 if target == TO_INSIDE else 17
        device_volume = upload(vol)
        for limit in LONG_LIMITS:
            want = np.minimum(exact, np.uint64(NONE if limit is None else limit)).astype(np.uint32)
            what = "%s %s, to %s, limit %s" % (content, extent, ("inside", "outside")[target], limit)
            same(run(ctx, vol, ISO, target, limit, device_volume=device_volume, what=what), want, what)


# ---- boxes ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box_volume():
    w, h, d = BOX_VOLUME
    return contents("random 0.02", (d, h, w), seed=91)


@pytest.mark.parametrize("box", sorted(BOXES), ids=lambda b: b.replace(" ", "_").replace(",", ""))
def test_a_box_is_transformed_as_the_cropped_array(ctx, box_volume, box):
    b = BOXES[box]
    x0, y0, z0, w, h, d = b
    crop = np.ascontiguousarray(box_volume[z0:z0 + d, y0:y0 + h, x0:x0 + w])
    for target in TARGETS:
        want = edt2_np(crop, ISO, target)        # nothing beyond the box exists
        assert np.array_equal(want, edt2_np(box_volume, ISO, target, None, b))
        for limit in (None, 10):
            got = run(ctx, box_volume, ISO, target, limit, box=b, what="box %s" % box)
            assert got.shape == (d, h, w)
            same(got, cap(want, limit), "box %s, to %s, limit %s" % (box, target, limit))


def test_the_only_target_lies_outside_the_box(ctx):
    vol = np.full((20, 9, 301), 17, np.uint8)
    vol[0, 0, 0] = vol[19, 8, 300] = vol[10, 4, 2] = 200
    box = (3, 1, 1, 291, 6, 18)
    assert (vol[1:19, 1:7, 3:294] == 17).all()
    for limit in LIMITS:
        got = run(ctx, vol, ISO, TO_INSIDE, limit, box=box, what="target outside the box, limit %s" % limit)
        assert got.shape == (18, 6, 291) and (got == (NONE if limit is None else limit)).all()
        assert (run(ctx, vol, ISO, TO_OUTSIDE, limit, box=box, what="all target, limit %s" % limit) == 0).all()


# ---- alignment and iso ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", [(7, 3, 3), (131, 3, 2)], ids=lambda e: "%dx%dx%d" % e)
def test_every_volume_alignment_with_both_guard_fills(ctx, extent):
    """a result that consumed a guard byte as a voxel differs under one of the two fills"""
    w, h, d = extent
    vol = contents("random 0.1", (d, h, w), seed=77)
    for fill in (0x00, 0xFF):
        for offset in (0, 1, 2, 3):
            check_all_limits(ctx, vol, limits=(None, 2), offset=offset, fill=fill, what="%s, volume +%d fill %#x" % (extent, offset, fill))


def test_iso_on_a_voxel_value_and_the_extreme_isos(ctx):
    vol = np.random.default_rng(6).integers(120, 137, size=(5, 6, 70), dtype=np.uint8)
    iso = float(np.float32(128) * np.float32(1.0 / 255.0))
    check_all_limits(ctx, vol, iso=iso, limits=(None, 3), what="iso = 128 / 255")
    for iso in (0.0, -3.0, 1.0, 1.5):
        check_all_limits(ctx, vol, iso=iso, limits=(None, 3), what="iso %g" % iso)
    check_all_limits(ctx, np.full((2, 3, 65), 255, np.uint8), iso=1.0, limits=(None,), what="iso 1 on bytes of 255")


# ---- determinism and capture ------------------------------------------------------------------------------------------------------------
def test_two_runs_on_the_same_buffers_give_identical_bytes(ctx):
    vol = contents("random 0.01", (19, 5, 258), seed=21)
    d_vol = torch.from_numpy(vol).cuda()
    n = lib.distance_transform_scratch_bytes(ext_of(vol))
    d_scratch = torch.full(((n + 7) // 8,), -1, dtype=torch.int64, device="cuda")
    for target in TARGETS:
        for limit in (None, 10):
            d_dist = torch.full(vol.shape, -1, dtype=torch.int32, device="cuda")
            results = []
            for _ in range(2):        # the second run starts from the first run's distances and scratch
                ctx.distance_transform(d_vol.data_ptr(), ext_of(vol), None, ISO, target, limit, d_scratch.data_ptr(), d_dist.data_ptr(), st())
                torch.cuda.synchronize()
                results.append(d_dist.cpu().numpy().view(np.uint32))
            assert np.array_equal(results[0], results[1])
            same(results[1], edt2_np(vol, ISO, target, limit), "second run")


def test_transform_and_select_captured_into_a_graph_replay(ctx):
    shape = (17, 9, 131)
    vol = contents("random 0.05", shape, seed=13)
    d_vol = torch.from_numpy(vol).cuda()
    d_out = torch.empty_like(d_vol)
    d_scratch = torch.empty(((lib.distance_transform_scratch_bytes(ext_of(vol)) + 7) // 8,), dtype=torch.int64, device="cuda")
    d_dist = torch.empty(shape, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()

    def call():        # a dilation by radius^2 9
        ctx.distance_transform(d_vol.data_ptr(), ext_of(vol), None, ISO, TO_INSIDE, 10, d_scratch.data_ptr(), d_dist.data_ptr(), s.cuda_stream)
        ctx.select_by_distance(d_vol.data_ptr(), d_out.data_ptr(), ext_of(vol), None, d_dist.data_ptr(), 1, 9, 255, s.cuda_stream)

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
        want = edt2_np(vol, ISO, TO_INSIDE, 10)
        same(d_dist.cpu().numpy().view(np.uint32), want, "replay, seed %d: distances" % seed)
        same(d_out.cpu().numpy(), dilate_np(vol, ISO, 9), "replay, seed %d: the dilated volume" % seed)


# ---- rejected calls ---------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_write_nothing(ctx):
    w, h, d = 12, 5, 4
    e = abi.Extent3D(w, h, d)
    vol = torch.full((d, h, w), 200, dtype=torch.uint8, device="cuda")
    out = torch.full((8192,), FILL, dtype=torch.uint8, device="cuda")        # [scratch 2048 | distances 2048 | a volume 2048 | spare]
    a = out.data_ptr()
    assert a % 8 == 0 and lib.distance_transform_scratch_bytes(e) <= 2048
    scratch, dist, dst, v = a, a + 2048, a + 4096, vol.data_ptr()
    bad, unsupported, inf, nan = abi.VKV_E_INVALID_ARGUMENT, abi.VKV_E_UNSUPPORTED, float("inf"), float("nan")
    rc = lambda *args: ctx.distance_transform_rc(*args, st())  # noqa: E731
    assert rc(None, e, None, 0.5, 0, 5, scratch, dist) == bad
    assert rc(v, e, None, 0.5, 0, 5, None, dist) == bad
    assert rc(v, e, None, 0.5, 0, 5, scratch, None) == bad
    assert rc(v, abi.Extent3D(w, 0, d), None, 0.5, 0, 5, scratch, dist) == bad
    for iso in (inf, -inf, nan):
        assert rc(v, e, None, iso, 0, 5, scratch, dist) == bad and "iso" in ctx.last_error()
    for target in (-1, 2, 6):
        assert rc(v, e, None, 0.5, target, 5, scratch, dist) == bad and "target" in ctx.last_error()
    assert rc(v, e, None, 0.5, 0, 0, scratch, dist) == bad and "limit" in ctx.last_error()
    assert rc(v, e, abi.Box(0, 0, 0, 13, 2, 2), 0.5, 0, 5, scratch, dist) == bad and "box" in ctx.last_error()
    assert rc(v, e, abi.Box(11, 4, 3, 1, 2, 1), 0.5, 0, 5, scratch, dist) == bad
    assert rc(v, e, abi.Box(1, 1, 1, 2, 0, 2), 0.5, 0, 5, scratch, dist) == bad
    assert rc(v, e, None, 0.5, 0, 5, scratch + 4, dist) == bad and "aligned" in ctx.last_error()
    assert rc(v, e, None, 0.5, 0, 5, scratch, dist + 2) == bad
    assert rc(v, abi.Extent3D(32768, 32768, 4), None, 0.5, 0, 5, scratch, dist) == unsupported        # 2^32 voxels: one too many
    assert rc(v, abi.Extent3D(32769, 1, 1), None, 0.5, 0, 5, scratch, dist) == unsupported        # an axis above 32768
    assert rc(v, abi.Extent3D(2, 2, 40000), None, 0.5, 0, 5, scratch, dist) == unsupported
    # vkv_select_by_distance
    sel = lambda *args: ctx.select_by_distance_rc(*args, st())  # noqa: E731
    assert sel(None, dst, e, None, dist, 1, 4, 0) == bad
    assert sel(v, None, e, None, dist, 1, 4, 0) == bad
    assert sel(v, dst, e, None, None, 1, 4, 0) == bad
    assert sel(v, dst, abi.Extent3D(0, h, d), None, dist, 1, 4, 0) == bad
    assert sel(v, dst, e, abi.Box(0, 0, 0, 13, 2, 2), dist, 1, 4, 0) == bad and "box" in ctx.last_error()
    assert sel(v, dst, e, abi.Box(1, 1, 1, 2, 0, 2), dist, 1, 4, 0) == bad
    assert sel(v, dst, e, None, dist, 1, 4, 256) == bad and "fill" in ctx.last_error()
    assert sel(v, dst, e, None, dist, 5, 4, 0) == bad and "lo" in ctx.last_error()
    assert sel(v, dst, e, None, dist + 2, 1, 4, 0) == bad and "aligned" in ctx.last_error()
    for shift in (1, 100, w * h * d - 1):        # the two volumes overlap without being equal
        assert sel(dst, dst + shift, e, None, dist, 1, 4, 0) == bad and "overlap" in ctx.last_error()
        assert sel(dst + shift, dst, e, None, dist, 1, 4, 0) == bad
    assert sel(v, dst, abi.Extent3D(32768, 32768, 4), None, dist, 1, 4, 0) == unsupported
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((vol == 200).all())
    # and the accepted calls next to them: everything is inside, so every voxel is 0 from the inside and `limit` from the outside
    assert rc(v, e, None, 0.5, 0, 5, scratch, dist) == abi.VKV_OK
    torch.cuda.synchronize()
    assert bool((out[2048:2048 + 960].view(torch.int32) == 0).all()) and bool((out[2048 + 960:4096] == FILL).all())
    assert rc(v, e, None, 0.5, 1, 5, scratch, dist) == abi.VKV_OK
    assert sel(v, v, e, None, dist, 5, 5, 7) == abi.VKV_OK
    torch.cuda.synchronize()
    assert bool((out[2048:2048 + 960].view(torch.int32) == 5).all()) and bool((out[2048 + 960:] == FILL).all())
    assert bool((vol == 7).all())


# ---- vkv_select_by_distance -------------------------------------------------------------------------------------------------------------
def select(ctx, vol, dist2, lo, hi, fill, box=None, in_place=False, what=""):
    """the whole destination volume of ONE vkv_select_by_distance call on guarded buffers (the destination pre-filled with FILL unless in place)"""
    abox = None if box is None else abi.Box(*box)
    d_src, h_src = T.guarded(vol, 1, FILL, "cuda")
    d_dst, h_dst = (d_src, h_src) if in_place else T.guarded(vol.shape, 3, FILL, "cuda")
    d_dist, h_dist = T.guarded(dist2.view(np.int32), 0, FILL, "cuda")
    ctx.select_by_distance(d_src.data_ptr(), d_dst.data_ptr(), ext_of(vol), abox, d_dist.data_ptr(), lo, hi, fill, st())
    torch.cuda.synchronize()
    for name, h in (("d_src", h_src), ("d_dst", h_dst), ("d_dist2", h_dist)):
        bad = guard_damage(h)
        assert not bad, "%s: %s: guard bytes %s changed" % (what, name, bad[:8])
    if not in_place:
        assert np.array_equal(d_src.cpu().numpy(), vol), "%s: the source changed" % what
    assert np.array_equal(d_dist.cpu().numpy().view(np.uint32), dist2)
    return d_dst.cpu().numpy()


@pytest.mark.parametrize("target", TARGETS)
def test_select_against_the_statement(ctx, target):
    vol = contents("random 0.05", (9, 7, 131), seed=5)
    vol[vol > 128] = np.random.default_rng(1).integers(128, 256, size=int((vol > 128).sum()), dtype=np.uint8)        # not one value: src is copied
    dist2 = run(ctx, vol, ISO, target, None, what="distances for select")
    same(dist2, edt2_np(vol, ISO, target), "distances for select")
    fresh = np.full(vol.shape, FILL, np.uint8)
    top = int(dist2.max())
    for lo, hi, fill in ((1, 4, 0), (1, 9, 255), (0, 0, 9), (0, NONE, 1), (top + 1, NONE, 0), (top, top, 3), (3, 3, 5), (5, 8, 77)):
        want = select_by_distance_np(vol, dist2, lo, hi, fill)
        what = "select [%d, %d] fill %d, to %d" % (lo, hi, fill, target)
        if (lo, hi) == (0, NONE):
            assert (want == 1).all()        # a range that hits everything
        if lo == top + 1:
            assert np.array_equal(want, vol)        # and one that hits nothing
        same(select(ctx, vol, dist2, lo, hi, fill, what=what), want, what)
        same(select(ctx, vol, dist2, lo, hi, fill, in_place=True, what=what + ", in place"), want, what + ", in place")
    assert (select_by_distance_np(vol, dist2, 1, 4, 0) != vol).any()
    # a box: its own distances; the bytes outside it untouched
    box = (40, 1, 2, 70, 5, 6)
    bd = run(ctx, vol, ISO, target, 10, box=box, what="distances of a box for select")
    same(bd, edt2_np(vol, ISO, target, 10, box), "distances of a box for select")
    same(select(ctx, vol, bd, 1, 9, 3, box=box, what="box"), select_by_distance_np(vol, bd, 1, 9, 3, box=box, dst=fresh), "box")
    same(select(ctx, vol, bd, 1, 9, 3, box=box, in_place=True, what="box, in place"), select_by_distance_np(vol, bd, 1, 9, 3, box=box), "box, in place")


# ---- Volume.distance_transform / erode / dilate / open / close ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blobs():
    """31 x 26 x 37 of smooth noise thresholded near iso: blobs, pores, thin bridges"""
    from scipy import ndimage
    field = ndimage.gaussian_filter(np.random.default_rng(4).random((31, 26, 37)), 1.5)
    return np.where(field > np.median(field), 200, 17).astype(np.uint8)


def test_volume_morphology_against_scipy(ctx, blobs):
    from scipy import ndimage
    v = make_volume(ctx, blobs, block=2, packed=False)
    inside = blobs >= 128
    for to, target in (("inside", TO_INSIDE), ("outside", TO_OUTSIDE)):
        for limit in (None, 5):
            got = v.distance_transform(ISO, to=to, limit=limit)
            assert got.dtype == torch.uint32 and tuple(got.shape) == blobs.shape
            same(got.cpu().numpy(), edt2_np(blobs, ISO, target, limit), "Volume.distance_transform to %s, limit %s" % (to, limit))
    box = ((2, 3, 1), (17, 6, 9))
    got = v.distance_transform(ISO, to="outside", box=box)
    same(got.cpu().numpy(), edt2_np(blobs, ISO, TO_OUTSIDE, None, (2, 3, 1, 17, 6, 9)), "Volume.distance_transform: box")
    for r2 in (1, 2, 3, 4, 9, 10):
        ball = ball_structure(r2)
        eroded, dilated = ndimage.binary_erosion(inside, structure=ball, border_value=1), ndimage.binary_dilation(inside, structure=ball)
        opened = ndimage.binary_dilation(eroded, structure=ball)
        closed = ndimage.binary_erosion(dilated, structure=ball, border_value=1)
        for name, mask in (("erode", eroded), ("dilate", dilated), ("open", opened), ("close", closed)):
            out = getattr(v, name)(ISO, radius2=r2)
            assert out.dtype == torch.uint8 and out.data_ptr() != v.volume.data_ptr() and tuple(out.shape) == blobs.shape
            assert np.array_equal(out.cpu().numpy() >= 128, mask), "Volume.%s(radius2=%d) against scipy" % (name, r2)
        same(v.erode(ISO, radius2=r2, outside_fill=3).cpu().numpy(), erode_np(blobs, ISO, r2, 3), "Volume.erode(radius2=%d): bytes" % r2)
        same(v.dilate(ISO, radius2=r2, inside_fill=222).cpu().numpy(), dilate_np(blobs, ISO, r2, 222), "Volume.dilate(radius2=%d): bytes" % r2)
    assert (ndimage.binary_erosion(inside, structure=ball_structure(4), border_value=1) != ndimage.binary_erosion(inside, structure=ball_structure(4))).any()
    same(v.volume.cpu().numpy(), blobs, "the volume itself")
    same(v.open(ISO, radius=np.sqrt(2)).cpu().numpy(), v.open(ISO, radius2=2).cpu().numpy(), "radius sqrt(2) is radius2 2")
    # a box: the box's voxels alone exist; the bytes outside it are the volume's
    b = (5, 2, 3, 20, 17, 22)
    crop = np.ascontiguousarray(blobs[3:25, 2:19, 5:25])
    want = blobs.copy()
    want[3:25, 2:19, 5:25] = erode_np(crop, ISO, 4)
    same(v.erode(ISO, radius=2, box=((5, 2, 3), (20, 17, 22))).cpu().numpy(), want, "Volume.erode: box")
    assert np.array_equal(want[3:25, 2:19, 5:25] >= 128, ndimage.binary_erosion(crop >= 128, structure=ball_structure(4), border_value=1))
    want[3:25, 2:19, 5:25] = dilate_np(erode_np(crop, ISO, 4), ISO, 4)
    same(v.open(ISO, radius=2, box=abi.Box(*b)).cpu().numpy(), want, "Volume.open: box")
    target = torch.empty_like(v.volume)
    assert v.close(ISO, radius=2, out=target) is target
    same(target.cpu().numpy(), erode_np(dilate_np(blobs, ISO, 4), ISO, 4), "Volume.close(out)")
    for kw in (dict(), dict(radius=1, radius2=1), dict(radius=0.5), dict(radius2=0), dict(radius=1, inside_fill=256), dict(radius=1, outside_fill=-1)):
        with pytest.raises(ValueError):
            v.erode(ISO, **kw)
    with pytest.raises(ValueError):
        v.distance_transform(ISO, to="border")
    with pytest.raises(ValueError):
        v.distance_transform(ISO, limit=0)
    with pytest.raises(ValueError):
        v.distance_transform(ISO, box=((0, 0, 0), (38, 2, 2)))
    inplace = make_volume(ctx, blobs, block=2, packed=False)
    assert inplace.open(ISO, radius2=4, out=inplace.volume) is inplace.volume
    same(inplace.volume.cpu().numpy(), dilate_np(erode_np(blobs, ISO, 4), ISO, 4), "Volume.open in place")


IN_PLACE = ("dilate", "close", "open", "erode", "remove_islands")


@pytest.mark.parametrize("call", IN_PLACE)
def test_in_place_results_keep_the_max_map_current(ctx, blobs, call):
    """out=v.volume: dilate and close raise voxels to inside_fill, so the map built before the call is no upper bound any more and everything
    that skips through it would drop geometry; the others lower voxels.  After the call the map is max_map_np of the new bytes, and the
    consumers that skip through it give what the dense ones give"""
    from tests.test_gpu_mip import assert_same_bits, draw, subpass
    from tests.test_mesh_cpu import mesh_np, same_bits
    from tests.test_mip_cpu import max_map_np
    r2, block = 4, 2
    base = blobs
    if call == "remove_islands":
        base = erode_np(blobs, ISO, r2)        # (the blobs are one component; eroded they fall apart)
        wl, ws, wc = components_np(base, ISO, 6)
        assert wc[0] >= 10
        want = select_np(base, wl, ws, len(ws), int(ws.max()), 2 ** 64 - 1, 0)
    else:
        want = {"dilate": lambda: dilate_np(blobs, ISO, r2), "erode": lambda: erode_np(blobs, ISO, r2), "open": lambda: dilate_np(erode_np(blobs, ISO, r2), ISO, r2),
                "close": lambda: erode_np(dilate_np(blobs, ISO, r2), ISO, r2)}[call]()
    me = tuple(-(-e // block) for e in base.shape[::-1])
    before, after = max_map_np(base, me), max_map_np(want, me)
    assert (want != base).any() and (after != before).any(), "the premise: the call changes voxels and the map"
    if call in ("dilate", "close"):
        assert ((before < 128) & (after >= 128)).any(), "the premise: a cell below iso holds inside voxels after the call"
    v = make_volume(ctx, base, block=block, packed=False)
    same(v.max_map.cpu().numpy(), before, "the map before the call")
    if call == "remove_islands":
        assert v.remove_islands(ISO, keep_largest=True, out=v.volume) is v.volume
    else:
        assert getattr(v, call)(ISO, radius2=r2, out=v.volume) is v.volume
    same(v.volume.cpu().numpy(), want, "Volume.%s in place" % call)
    same(v.max_map.cpu().numpy(), after, "Volume.%s in place: the max map" % call)
    mesh = mesh_np(want, ISO)
    assert len(mesh) > 100
    for use_max_map in (True, False):
        tri, total = v.extract_isosurface(ISO, use_max_map=use_max_map)
        assert total == len(mesh)
        same_bits(tri.cpu().numpy(), mesh, "extract_isosurface(use_max_map=%s) after Volume.%s in place" % (use_max_map, call))
    labels, sizes, counts = v.label_components(ISO, connectivity=6, use_max_map=True)
    wl, ws, wc = components_np(want, ISO, 6)
    same(labels.cpu().numpy(), wl, "label_components(use_max_map=True): labels")
    same(sizes.cpu().numpy(), ws, "label_components(use_max_map=True): sizes")
    assert counts.cpu().tolist() == wc.tolist()
    sp, p = subpass(v)
    dense, fast = draw(sp, p, 0.5, 1.0, skip=False), draw(sp, p, 0.5, 1.0, skip=True)
    assert (dense["rgba8"][:, 3] == 255).sum() > 20
    assert_same_bits(fast, dense, "draw_mip(skip=True) after Volume.%s in place" % call)


def test_an_opening_cuts_the_bridge_that_island_removal_cannot(ctx):
    """48 x 40 x 40: two balls of bytes 200 joined by a bar two voxels thick are ONE component; open(radius=2) cuts the bar, and
    remove_islands(keep_largest) then leaves the larger ball: the scipy chain"""
    from scipy import ndimage
    z, y, x = np.indices((40, 40, 48))
    big = (x - 13) ** 2 + (y - 20) ** 2 + (z - 20) ** 2 <= 10 ** 2
    small = (x - 37) ** 2 + (y - 19) ** 2 + (z - 20) ** 2 <= 7 ** 2
    bar = (x >= 13) & (x <= 37) & (y >= 19) & (y <= 20) & (z >= 19) & (z <= 20)
    vol = np.where(big | small | bar, 200, 0).astype(np.uint8)
    assert components_np(vol, ISO, 6)[2][0] == 1 and ndimage.label(vol >= 128)[1] == 1
    v = make_volume(ctx, vol, block=2, packed=False)
    assert int(v.label_components(ISO, connectivity=6, sizes=False)[2][0].item()) == 1
    same(v.remove_islands(ISO, keep_largest=True).cpu().numpy(), vol, "island removal alone keeps everything")
    opened = v.open(ISO, radius=2)
    ball = ball_structure(4)
    mask = ndimage.binary_dilation(ndimage.binary_erosion(vol >= 128, structure=ball, border_value=1), structure=ball)
    want_opened = dilate_np(erode_np(vol, ISO, 4), ISO, 4)
    same(opened.cpu().numpy(), want_opened, "open(radius=2)")
    assert np.array_equal(want_opened >= 128, mask)
    labels, count = ndimage.label(mask)
    assert count == 2
    v2 = make_volume(ctx, opened.cpu().numpy(), block=2, packed=False)
    assert int(v2.label_components(ISO, connectivity=6, sizes=False)[2][0].item()) == 2
    kept = v2.remove_islands(ISO, keep_largest=True).cpu().numpy()
    sizes = np.bincount(labels.reshape(-1))[1:]
    largest = labels == 1 + int(np.argmax(sizes))
    assert np.array_equal(kept >= 128, largest) and largest.sum() > 3000 and not largest[small].any() and largest[20, 20, 13]        # the big ball's centre
    wl, ws, wc = components_np(want_opened, ISO, 6)
    same(kept, select_np(want_opened, wl, ws, len(ws), int(ws.max()), 2 ** 64 - 1, 0), "open, then remove_islands(keep_largest)")
