"""GPU: vkv_isosurface_mesh (marching tetrahedra) bit for bit against the vectorised numpy statement of
tests/test_mesh_cpu.py (mesh_np): the total, the written count and every float.

The count and emit kernels work in tiles of 256 x 4 cubes (four waves, each 64 lanes of four x-adjacent cubes of one row) that march over 16
slices of cubes; a lane loads the dword of its voxels and takes the fifth from the lane above, the wave's last lane from a byte load; widths
below 4 gather bytes.  A wave's count per slice is one ENTRY; the entries are scanned in chunks of 4096 and the chunk sums by one workgroup,
256 at a time.  The extents below put the number of cubes per row (W - 1) at 0 .. 5, around the lane (4), and at 255, 256, 257 (a wave and a
workgroup), the rows (H - 1) at 3, 4, 5 and the slices (D - 1) at 15, 16, 17; 258 x 6 x 18 spans two workgroups on every axis; 2 x 66 x 65
crosses a scan chunk and 2 x 1026 x 1026 the 256 chunk sums of one round.  Every buffer is a tests/helpers.py guarded() allocation: the
triangle buffer is pre-filled and compared as a whole (an unwritten float shows as the pre-fill, a float past `written` must still hold it) and
all guards must be intact, so nothing here relies on, or can cause, a fault."""
import numpy as np
import pytest
import torch

from tests import helpers as T
from tests.test_gpu_mip import make_volume
from tests.test_mesh_cpu import MESH_CONTENTS, KINV255, ball, mesh_contents, mesh_np, same_bits
from vkvolume_amd import abi, lib

pytestmark = pytest.mark.gpu
FILL = 0xA5          # pre-fill of every output, scratch included
ISO = 0.5


@pytest.fixture(scope="module")
def ctx():
    torch.cuda.set_device(0)
    c = lib.Context(0)
    yield c
    c.close()


def st():
    return torch.cuda.current_stream().cuda_stream


def ext_of(vol):
    d, h, w = vol.shape
    return abi.Extent3D(w, h, d)


def block_extent(vol, block):
    d, h, w = vol.shape
    return abi.Extent3D((w + block - 1) // block, (h + block - 1) // block, (d + block - 1) // block)


def run(ctx, vol, iso, capacity, box=None, block=0, vol_offset=0, vol_fill=0x00, null_triangles=False, map_extent=None, max_map=None, what=""):
    """(counts [2] uint64, the whole triangle buffer [capacity, 3, 3] float32) of ONE vkv_isosurface_mesh call on guarded buffers, every output
    pre-filled with FILL; with `block` the call goes through the max map of that block size (built here by vkv_max_map), with `map_extent` (w, h, d)
    through the map of that extent: built here, or the bytes `max_map` (md, mh, mw)"""
    abox = None if box is None else abi.Box(*box)
    d_vol, h_vol = T.guarded(vol, vol_offset, vol_fill, "cuda")
    nbytes = lib.mesh_scratch_bytes(ext_of(vol), abox)
    assert nbytes >= 16 and nbytes % 8 == 0, (what, nbytes)
    d_scratch, h_scratch = T.guarded((nbytes // 8,), 0, FILL, "cuda", dtype=np.int64)
    d_counts, h_counts = T.guarded((2,), 0, FILL, "cuda", dtype=np.int64)
    d_tri, h_tri = T.guarded((max(capacity, 1), 3, 3), 0, FILL, "cuda", dtype=np.float32)
    handles = [("d_volume", h_vol), ("d_scratch", h_scratch), ("d_counts", h_counts), ("d_triangles", h_tri)]
    d_map = me = None
    if block or map_extent is not None:
        me = block_extent(vol, block) if map_extent is None else abi.Extent3D(*map_extent)
        if max_map is None:
            d_map, h_map = T.guarded((me.depth, me.height, me.width), 0, FILL, "cuda")
            ctx.max_map(d_vol.data_ptr(), ext_of(vol), me, None, d_map.data_ptr(), st())
        else:
            assert max_map.shape == (me.depth, me.height, me.width) and max_map.dtype == np.uint8
            d_map, h_map = T.guarded(max_map, 0, FILL, "cuda")
        handles.append(("d_max_map", h_map))
    ctx.isosurface_mesh(d_vol.data_ptr(), ext_of(vol), abox, iso, None if d_map is None else d_map.data_ptr(), me, d_scratch.data_ptr(),
                        None if null_triangles else d_tri.data_ptr(), capacity, d_counts.data_ptr(), st())
    torch.cuda.synchronize()
    for name, h in handles:
        bad = h.check()
        assert not bad, "%s: %s: guard bytes %s changed (payload is bytes %d .. %d)" % (what, name, bad[:8], h.start, h.stop - 1)
    assert np.array_equal(d_vol.cpu().numpy(), vol), "%s: the volume changed" % what
    return d_counts.cpu().numpy().view(np.uint64), d_tri.cpu().numpy()


def check(ctx, vol, iso, want, capacity=None, what="", **kw):
    """one call with `capacity` (None: the total + 5) against the oracle's list `want`: counts, the exact prefix, the pre-fill behind it"""
    total = len(want)
    capacity = total + 5 if capacity is None else capacity
    counts, tri = run(ctx, vol, iso, capacity, what=what, **kw)
    written = min(total, capacity)
    assert counts.tolist() == [total, written], "%s: counts %s, expected %s" % (what, counts.tolist(), [total, written])
    expect = np.full(tri.shape, 0, np.float32)
    expect.view(np.uint8)[...] = FILL
    expect[:written] = want[:written]
    same_bits(tri, expect, what)
    return counts, tri


# ---- extents and contents ---------------------------------------------------------------------------------------------------------------
EXTENTS = [(1, 1, 1), (1, 4, 3), (2, 2, 2), (3, 1, 4), (4, 5, 1), (5, 4, 16), (6, 6, 17), (7, 3, 18), (64, 2, 2), (65, 5, 3), (66, 3, 2),
           (256, 4, 2), (257, 2, 17), (258, 6, 18), (2, 66, 65)]  # (width, height, depth)


@pytest.mark.parametrize("extent", EXTENTS, ids=lambda e: "%dx%dx%d" % e)
def test_every_extent_and_content(ctx, extent):
    w, h, d = extent
    for k, content in enumerate(MESH_CONTENTS):
        vol = mesh_contents(content, (d, h, w), seed=700 + k)
        want = mesh_np(vol, ISO)
        what = "%s %s" % (content, extent)
        if content in ("below", "above") or min(extent) < 2:
            assert len(want) == 0, what
        elif content != "ball" or min(extent) > 2:
            assert len(want) > 0, what
        check(ctx, vol, ISO, want, what=what)


def test_more_chunk_sums_than_one_round_of_the_scan(ctx):
    """1025 x 1025 entries = 257 chunks of 4096: the single workgroup that scans the chunk sums carries a total into a second round"""
    w, h, d = 2, 1026, 1026
    vol = np.zeros((d, h, w), np.uint8)
    for z, y in ((0, 0), (3, 1000), (512, 513), (1023, 0), (1025, 1025)):
        vol[z, y, :] = 255
    want = mesh_np(vol, ISO)
    assert len(want) > 0
    check(ctx, vol, ISO, want, what="257 chunks")
    check(ctx, vol, ISO, want, capacity=len(want) - 1, what="257 chunks, capacity total - 1")


# ---- alignment --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", [(7, 3, 3), (261, 3, 2)], ids=lambda e: "%dx%dx%d" % e)
def test_every_volume_alignment_with_both_guard_fills(ctx, extent):
    """odd widths: a row's tail and the next row's head share a dword, and the last row ends where the guard begins; a result that
    consumed a guard byte differs under one of the two fills (0x00: outside at every iso, 0xFF: inside)"""
    w, h, d = extent
    vol = mesh_contents("random", (d, h, w), seed=77)
    want = mesh_np(vol, ISO)
    for fill in (0x00, 0xFF):
        for offset in (0, 1, 2, 3, 5, 7):
            check(ctx, vol, ISO, want, vol_offset=offset, vol_fill=fill, what="%s volume +%d fill %#x" % (extent, offset, fill))


# ---- capacity ---------------------------------------------------------------------------------------------------------------------------
def test_capacity_gives_the_exact_prefix_and_the_full_total(ctx):
    vol = mesh_contents("random", (18, 6, 70), seed=3)
    want = mesh_np(vol, ISO)
    total = len(want)
    assert total > 1000
    for capacity in (1, 7, total - 1, total, total + 5):
        check(ctx, vol, ISO, want, capacity=capacity, what="capacity %d of %d" % (capacity, total))
    counts, tri = run(ctx, vol, ISO, 0, null_triangles=True, what="counting call")
    assert counts.tolist() == [total, 0]
    assert (tri.view(np.uint8) == FILL).all()
    check(ctx, vol, ISO, want, capacity=0, what="capacity 0 with a buffer")


# ---- boxes ------------------------------------------------------------------------------------------------------------------------------
BOX_VOLUME = (301, 9, 20)  # (width, height, depth)
BOXES = {
    "one cube": (100, 4, 10, 2, 2, 2), "corner 0": (0, 0, 0, 2, 2, 2), "corner 1": (299, 7, 18, 2, 2, 2),
    "face x0": (0, 3, 9, 3, 3, 3), "face x1": (297, 3, 9, 4, 3, 3), "face y0": (100, 0, 9, 3, 2, 3), "face y1": (100, 7, 9, 3, 2, 3),
    "face z0": (100, 3, 0, 3, 3, 2), "face z1": (100, 3, 18, 3, 3, 2),
    "width 1": (150, 0, 0, 1, 9, 20), "height 1": (0, 8, 0, 301, 1, 20), "depth 1": (0, 0, 19, 301, 9, 1),
    "across tiles": (3, 2, 1, 291, 6, 19),        # 290 cubes = 256 + 8 lanes + 2, 5 rows, 18 slices
    "whole volume": (0, 0, 0, 301, 9, 20),
}


@pytest.fixture(scope="module")
def box_volume():
    w, h, d = BOX_VOLUME
    return mesh_contents("random", (d, h, w), seed=91)


@pytest.mark.parametrize("box", sorted(BOXES), ids=lambda b: b.replace(" ", "_"))
def test_a_box_gives_the_cropped_volume_at_the_box_origin(ctx, box_volume, box):
    b = BOXES[box]
    want = mesh_np(box_volume, ISO, b)        # the oracle on the cropped array, coordinates shifted by the box origin before the addition of t
    if min(b[3:]) < 2:
        assert len(want) == 0
    else:
        assert len(want) > 0
    check(ctx, box_volume, ISO, want, box=b, what="box %s" % box)
    check(ctx, box_volume, ISO, want, box=b, block=4, what="box %s, max map" % box)


# ---- max map ----------------------------------------------------------------------------------------------------------------------------
def sparse_volume():
    """300 x 21 x 40 of dim noise (below iso 0.5) with three small bright balls: most tiles of 256 x 4 x 16 cubes are skipped"""
    d, h, w = 40, 21, 300
    vol = np.random.default_rng(8).integers(0, 100, size=(d, h, w), dtype=np.uint8)
    z, y, x = np.indices((d, h, w)).astype(np.float64)
    for cx, cy, cz in ((20.3, 6.1, 5.2), (258.0, 17.5, 33.0), (297.5, 2.0, 38.6)):
        dist = np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2)
        vol = np.maximum(vol, np.clip((3.0 - dist) * 60 + 128, 0, 255).astype(np.uint8))
    return vol


@pytest.mark.parametrize("block", [2, 4])
def test_max_map_gives_the_dense_bits(ctx, block):
    vol = sparse_volume()
    want = mesh_np(vol, ISO)
    assert len(want) > 100
    me = block_extent(vol, block)
    d_map = torch.empty((me.depth, me.height, me.width), dtype=torch.uint8, device="cuda")
    ctx.max_map(torch.from_numpy(vol).cuda().data_ptr(), ext_of(vol), me, None, d_map.data_ptr(), st())
    torch.cuda.synchronize()
    below = d_map.cpu().numpy().astype(np.float32) * KINV255 < np.float32(ISO)
    assert below.mean() > 0.5, "the premise: most cells are below iso"
    check(ctx, vol, ISO, want, what="dense")
    check(ctx, vol, ISO, want, block=block, what="max map, block %d" % block)
    check(ctx, vol, ISO, want, block=block, capacity=len(want) // 2, what="max map, block %d, half the capacity" % block)
    low = 0.05        # every map byte passes: nothing is skipped
    assert not (d_map.cpu().numpy().astype(np.float32) * KINV255 < np.float32(low)).any()
    want_low = mesh_np(vol, low)
    check(ctx, vol, low, want_low, block=block, what="max map, block %d, iso %g" % (block, low))
    empty = mesh_np(vol, 1.5)
    assert len(empty) == 0
    check(ctx, vol, 1.5, empty, block=block, what="max map, block %d, nothing inside" % block)


def test_iso_on_a_voxel_value_keeps_the_degenerate_triangles(ctx):
    iso = np.float32(128) * KINV255
    vol = np.random.default_rng(6).integers(120, 137, size=(5, 6, 9), dtype=np.uint8)
    vol[1:3, 2, 3:6] = 128
    want = mesh_np(vol, iso)
    assert len(want) > 0
    check(ctx, vol, float(iso), want, what="iso = 128 / 255")
    check(ctx, vol, float(iso), want, block=2, what="iso = 128 / 255, max map")


# ---- determinism and capture ------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bytes(ctx):
    vol = mesh_contents("random", (19, 5, 258), seed=21)
    want = mesh_np(vol, ISO)
    a = check(ctx, vol, ISO, want, what="first run")
    b = check(ctx, vol, ISO, want, what="second run")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def test_one_call_captured_into_a_graph_replays(ctx):
    shape = (17, 9, 131)
    vol = mesh_contents("random", shape, seed=13)
    capacity = 12 * 16 * 8 * 130
    d_vol = torch.from_numpy(vol).cuda()
    d_scratch = torch.empty((lib.mesh_scratch_bytes(ext_of(vol)) // 8,), dtype=torch.int64, device="cuda")
    d_counts = torch.zeros((2,), dtype=torch.int64, device="cuda")
    d_tri = torch.empty((capacity, 3, 3), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()

    def call():
        ctx.isosurface_mesh(d_vol.data_ptr(), ext_of(vol), None, ISO, None, None, d_scratch.data_ptr(), d_tri.data_ptr(), capacity, d_counts.data_ptr(),
                            s.cuda_stream)

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
            vol = mesh_contents("random", shape, seed=seed)
            d_vol.copy_(torch.from_numpy(vol))
        d_tri.view(torch.uint8).fill_(FILL)
        d_counts.fill_(-1)
        d_scratch.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        want = mesh_np(vol, ISO)
        assert d_counts.cpu().tolist() == [len(want), len(want)] and len(want) <= capacity
        same_bits(d_tri[:len(want)].cpu().numpy(), want, "replay, seed %d" % seed)
        assert bool((d_tri[len(want):].view(torch.uint8) == FILL).all())


# ---- rejected calls ---------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_write_nothing(ctx):
    w, h, d = 12, 5, 4
    e = abi.Extent3D(w, h, d)
    vol = torch.full((d, h, w), 200, dtype=torch.uint8, device="cuda")
    out = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")        # [scratch 2048 | counts 16 | triangles]
    a = out.data_ptr()
    assert a % 8 == 0 and lib.mesh_scratch_bytes(e) <= 2048
    scratch, counts, tri, v = a, a + 2048, a + 2064, vol.data_ptr()
    me, none = abi.Extent3D(3, 2, 1), None
    bad, inf, nan = abi.VKV_E_INVALID_ARGUMENT, float("inf"), float("nan")
    rc = lambda *args: ctx.isosurface_mesh_rc(*args, st())  # noqa: E731
    assert rc(None, e, None, 0.5, None, none, scratch, tri, 10, counts) == bad
    assert rc(v, e, None, 0.5, None, none, None, tri, 10, counts) == bad
    assert rc(v, e, None, 0.5, None, none, scratch, tri, 10, None) == bad
    assert rc(v, e, None, 0.5, None, none, scratch, None, 10, counts) == bad and "capacity" in ctx.last_error()
    assert rc(v, abi.Extent3D(w, 0, d), None, 0.5, None, none, scratch, tri, 10, counts) == bad
    for iso in (inf, -inf, nan):
        assert rc(v, e, None, iso, None, none, scratch, tri, 10, counts) == bad and "iso" in ctx.last_error()
    assert rc(v, e, abi.Box(0, 0, 0, 13, 2, 2), 0.5, None, none, scratch, tri, 10, counts) == bad and "box" in ctx.last_error()
    assert rc(v, e, abi.Box(11, 4, 3, 1, 2, 1), 0.5, None, none, scratch, tri, 10, counts) == bad
    assert rc(v, e, abi.Box(1, 1, 1, 2, 0, 2), 0.5, None, none, scratch, tri, 10, counts) == bad
    assert rc(v, e, None, 0.5, v, none, scratch, tri, 10, counts) == bad and "map_extent" in ctx.last_error()
    assert rc(v, e, None, 0.5, v, abi.Extent3D(13, 2, 1), scratch, tri, 10, counts) == bad
    assert rc(v, e, None, 0.5, None, none, scratch + 4, tri, 10, counts) == bad and "aligned" in ctx.last_error()
    assert rc(v, e, None, 0.5, None, none, scratch, tri + 2, 10, counts) == bad
    assert rc(v, e, None, 0.5, None, none, scratch, tri, 10, counts + 4) == bad
    assert rc(v, abi.Extent3D(0x80000000, 2, 2), None, 0.5, None, none, scratch, tri, 10, counts) == abi.VKV_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((vol == 200).all())
    # and the accepted call next to them, with a valid max map argument
    assert rc(v, e, None, 0.5, None, me, scratch, tri, 10, counts) == abi.VKV_OK
    torch.cuda.synchronize()
    assert out[2048:2064].view(torch.int64).tolist() == [0, 0] and bool((out[2064:] == FILL).all())


# ---- Volume.extract_isosurface ----------------------------------------------------------------------------------------------------------
def test_volume_extract_isosurface_matches_the_c_call(ctx):
    vol = ball()
    want = mesh_np(vol, ISO)
    v = make_volume(ctx, vol, block=2, packed=False)
    tri, total = v.extract_isosurface(ISO)
    assert total == 1824 == len(want) and tuple(tri.shape) == (1824, 3, 3) and tri.dtype == torch.float32
    same_bits(tri.cpu().numpy(), want, "extract_isosurface")
    tri, total = v.extract_isosurface(ISO, use_max_map=True)
    same_bits(tri.cpu().numpy(), want, "extract_isosurface, max map")
    tri, counts = v.extract_isosurface(ISO, capacity=1000, use_max_map=True)
    assert tuple(tri.shape) == (1000, 3, 3) and counts.cpu().tolist() == [1824, 1000]
    same_bits(tri.cpu().numpy(), want[:1000], "extract_isosurface, capacity 1000")
    tri, counts = v.extract_isosurface(ISO, capacity=0)
    assert tuple(tri.shape) == (0, 3, 3) and counts.cpu().tolist() == [1824, 0]
    box = ((2, 3, 1), (7, 6, 9))
    tri, total = v.extract_isosurface(ISO, box=box)
    want_box = mesh_np(vol, ISO, (2, 3, 1, 7, 6, 9))
    assert total == len(want_box) > 0
    same_bits(tri.cpu().numpy(), want_box, "extract_isosurface, box")
    tri, total = v.extract_isosurface(1.5)
    assert total == 0 and tuple(tri.shape) == (0, 3, 3)
    with pytest.raises(ValueError):
        v.extract_isosurface(ISO, box=((0, 0, 0), (13, 2, 2)))
    counts, _ = run(ctx, vol, ISO, 0, null_triangles=True, what="C call")
    assert counts.tolist() == [1824, 0]
