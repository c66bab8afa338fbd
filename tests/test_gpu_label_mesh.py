"""GPU: vkv_label_mesh bit for bit against the vectorised numpy statement of tests/test_label_mesh_cpu.py (label_mesh_np):
the total, the written count, every float and every triangle label.

The kernels work in the tiles of vkv_isosurface_mesh (256 x 4 cubes: four waves, each 64 lanes of four x-adjacent cubes of one row, marching
over 16 slices), so the extents are that call's boundary set: the cubes per row (W - 1) at 0 .. 5, around the lane (4), and at 255, 256, 257,
the rows at 3, 4, 5, the slices at 15, 16, 17; 258 x 6 x 18 spans two workgroups on every axis and 2 x 66 x 65 crosses a scan chunk.  A lane
loads its four labels as one 16-byte load at any 4-byte alignment, clamped at the row's end; widths below 4 gather.  Every buffer is a
tests/helpers.py guarded() allocation: both outputs are pre-filled and compared as a whole (an unwritten element shows as the pre-fill, an
element past `written` must still hold it) and all guards must be intact, so nothing here relies on, or can cause, a fault."""
import numpy as np
import pytest
import torch

from tests import helpers as T
from tests.test_components_cpu import components_np
from tests.test_gpu_mip import make_volume
from tests.test_label_mesh_cpu import (SKIP_COLORS, SKIP_SHAPE, bordered, distinct_labels, label_mesh_np, random_labels, rounds_labels, skip_labels)
from tests.test_mesh_cpu import mesh_contents, mesh_np, same_bits
from vkvolume_amd import abi, labels as LB, lib

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


def ext_of(shape_dhw):
    d, h, w = shape_dhw
    return abi.Extent3D(w, h, d)


def run(ctx, labels, colors=None, vol=None, iso=None, capacity=0, box=None, shape=None, map_extent=None, label_offset=0, label_fill=0x00, vol_offset=0,
        null_outputs=False, what=""):
    """(counts [2] uint64, the whole triangle buffer [capacity, 3, 3] float32, the whole label buffer [capacity] uint32) of ONE vkv_label_mesh
    call on guarded buffers, every output pre-filled with FILL.  labels: the box's shape; shape: the volume's (d, h, w) (None: the labels' or
    the volume's own); map_extent (w, h, d): through vkv_label_visibility_map of that extent, built here"""
    shape = (vol.shape if vol is not None else labels.shape) if shape is None else shape
    e = ext_of(shape)
    abox = None if box is None else abi.Box(*box)
    d_lab, h_lab = T.guarded(labels.view(np.int32), label_offset, label_fill, "cuda")
    handles = [("d_labels", h_lab)]
    d_col = d_vol = d_map = me = None
    if colors is not None:
        d_col, h_col = T.guarded(np.asarray(colors, np.uint32).view(np.int32), 0, 0xFF, "cuda")
        handles.append(("d_colors", h_col))
    if vol is not None:
        d_vol, h_vol = T.guarded(vol, vol_offset, 0x00, "cuda")
        handles.append(("d_volume", h_vol))
    nbytes = LB.mesh_scratch_bytes(e, abox)
    assert nbytes >= 16 and nbytes % 8 == 0, (what, nbytes)
    d_scratch, h_scratch = T.guarded((nbytes // 8,), 0, FILL, "cuda", dtype=np.int64)
    d_counts, h_counts = T.guarded((2,), 0, FILL, "cuda", dtype=np.int64)
    d_tri, h_tri = T.guarded((max(capacity, 1), 3, 3), 0, FILL, "cuda", dtype=np.float32)
    d_tl, h_tl = T.guarded((max(capacity, 1),), 0, FILL, "cuda", dtype=np.int32)
    handles += [("d_scratch", h_scratch), ("d_counts", h_counts), ("d_triangles", h_tri), ("d_triangle_labels", h_tl)]
    if map_extent is not None:
        me = abi.Extent3D(*map_extent)
        d_map, h_map = T.guarded((me.depth, me.height, me.width), 0, FILL, "cuda")
        handles.append(("d_visibility_map", h_map))
        ctx.check(ctx.label_visibility_map_rc(d_lab.data_ptr(), e, abox, d_col.data_ptr(), len(colors), me, d_map.data_ptr(), st()))
    ctx.check(ctx.label_mesh_rc(d_lab.data_ptr(), e, abox, None if d_col is None else d_col.data_ptr(), 0 if colors is None else len(colors),
                                None if d_vol is None else d_vol.data_ptr(), 0.0 if iso is None else iso, None if d_map is None else d_map.data_ptr(), me,
                                d_scratch.data_ptr(), None if null_outputs else d_tri.data_ptr(), None if null_outputs else d_tl.data_ptr(), capacity,
                                d_counts.data_ptr(), st()))
    torch.cuda.synchronize()
    for name, h in handles:
        bad = h.check()
        assert not bad, "%s: %s: guard bytes %s changed (payload is bytes %d .. %d)" % (what, name, bad[:8], h.start, h.stop - 1)
    assert np.array_equal(d_lab.cpu().numpy().view(np.uint32), labels), "%s: the labels changed" % what
    return d_counts.cpu().numpy().view(np.uint64), d_tri.cpu().numpy(), d_tl.cpu().numpy().view(np.uint32)


def check(ctx, labels, want, capacity=None, what="", **kw):
    """one call with `capacity` (None: the total + 5) against the oracle's (triangles, labels) `want`: counts, the exact prefix, the pre-fill
    behind it"""
    total = len(want[0])
    capacity = total + 5 if capacity is None else capacity
    counts, tri, tl = run(ctx, labels, capacity=capacity, what=what, **kw)
    written = min(total, capacity)
    assert counts.tolist() == [total, written], "%s: counts %s, expected %s" % (what, counts.tolist(), [total, written])
    expect = np.zeros(tri.shape, np.float32)
    expect.view(np.uint8)[...] = FILL
    expect[:written] = want[0][:written]
    same_bits(tri, expect, what)
    expect_l = np.full(tl.shape, FILL * 0x01010101, np.uint32)
    expect_l[:written] = want[1][:written]
    assert np.array_equal(tl, expect_l), "%s: %d triangle labels differ, first at %s" % (what, int((tl != expect_l).sum()), np.argwhere(tl != expect_l)[:4].tolist())
    return counts, tri, tl


def isosurface(ctx, vol, iso, total):
    """vkv_isosurface_mesh's triangles of the whole volume"""
    d_vol = torch.from_numpy(vol).cuda()
    d_scratch = torch.empty((lib.mesh_scratch_bytes(ext_of(vol.shape)) // 8,), dtype=torch.int64, device="cuda")
    d_counts = torch.zeros((2,), dtype=torch.int64, device="cuda")
    d_tri = torch.empty((max(total, 1), 3, 3), dtype=torch.float32, device="cuda")
    ctx.isosurface_mesh(d_vol.data_ptr(), ext_of(vol.shape), None, iso, None, None, d_scratch.data_ptr(), d_tri.data_ptr(), total, d_counts.data_ptr(), st())
    torch.cuda.synchronize()
    assert d_counts.cpu().tolist() == [total, total]
    return d_tri[:total].cpu().numpy()


# ---- extents and contents ---------------------------------------------------------------------------------------------------------------
EXTENTS = [(1, 1, 1), (1, 4, 3), (2, 2, 2), (3, 1, 4), (4, 5, 1), (5, 4, 16), (6, 6, 17), (64, 2, 2), (65, 5, 3), (256, 4, 2), (257, 2, 17), (258, 6, 18),
           (2, 66, 65)]  # (width, height, depth)


@pytest.mark.parametrize("extent", EXTENTS, ids=lambda e: "%dx%dx%d" % e)
def test_every_extent_and_content(ctx, extent):
    w, h, d = extent
    shape = (d, h, w)
    cubes = (w - 1) * (h - 1) * (d - 1)
    empty = (np.zeros((0, 3, 3), np.float32), np.zeros((0,), np.uint32))
    check(ctx, np.zeros(shape, np.uint32), empty, what="zeros %s" % (extent,))
    check(ctx, np.full(shape, 7, np.uint32), empty, what="one label %s" % (extent,))        # no triangles: the box's faces stay open
    labels = random_labels(shape, 800 + w)
    want = label_mesh_np(labels)
    assert (len(want[0]) > 0) == (cubes > 0)
    check(ctx, labels, want, what="random %s" % (extent,))
    labels = distinct_labels(shape)
    want = label_mesh_np(labels)
    assert len(want[0]) == 24 * cubes
    check(ctx, labels, want, what="distinct %s" % (extent,))
    # the 14-components of random bytes, with the volume: vkv_isosurface_mesh's own list, split by body
    iso = 0.8
    vol = mesh_contents("random", shape, seed=900 + w)
    labels = components_np(vol, iso, 14)[0]
    want = label_mesh_np(labels, None, vol, iso)
    same_bits(want[0], mesh_np(vol, iso), "14-components %s" % (extent,))
    _, tri, _ = check(ctx, labels, want, vol=vol, iso=iso, what="14-components %s" % (extent,))
    same_bits(tri[:len(want[0])], isosurface(ctx, vol, iso, len(want[0])), "against vkv_isosurface_mesh %s" % (extent,))


def test_more_chunk_sums_than_one_round_of_the_scan(ctx):
    """2 x 1026 x 1026 with five labelled rows far apart: 1025 x 1025 entries = 257 chunks of 4096, so the single workgroup that scans the
    chunk sums carries a total into a second round"""
    labels = rounds_labels()
    want = label_mesh_np(labels)
    assert len(want[0]) > 0 and sorted(set(want[1].tolist())) == [1, 2, 3]
    check(ctx, labels, want, what="257 chunks")
    check(ctx, labels, want, capacity=len(want[0]) - 1, what="257 chunks, capacity total - 1")


# ---- alignment --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent", [(7, 3, 3), (261, 3, 2)], ids=lambda e: "%dx%dx%d" % e)
def test_every_label_alignment_and_odd_volume_offsets(ctx, extent):
    """odd widths: a row's tail and the next row's head share a 16-byte load, and the last row ends where the guard begins; a result that
    consumed a guard label differs under one of the two fills (0x00: label 0, 0xFF: a label of its own)"""
    w, h, d = extent
    labels = random_labels((d, h, w), 77)
    vol = mesh_contents("random", (d, h, w), seed=78)
    want = label_mesh_np(labels, None, vol, ISO)
    for fill in (0x00, 0xFF):
        for offset, vol_offset in ((0, 0), (4, 1), (8, 3), (12, 5)):
            check(ctx, labels, want, vol=vol, iso=ISO, label_offset=offset, label_fill=fill, vol_offset=vol_offset,
                  what="%s labels +%d volume +%d fill %#x" % (extent, offset, vol_offset, fill))


# ---- boxes ------------------------------------------------------------------------------------------------------------------------------
BOX_VOLUME = (301, 9, 20)  # (width, height, depth)
BOXES = {
    "inside": (100, 4, 10, 3, 3, 4), "one cube": (7, 2, 3, 2, 2, 2), "corner 0": (0, 0, 0, 2, 2, 2), "corner 1": (299, 7, 18, 2, 2, 2),
    "face x1": (297, 3, 9, 4, 3, 3), "face y0 z1": (100, 0, 17, 5, 2, 3), "width 1": (150, 0, 0, 1, 9, 20), "depth 1": (0, 0, 19, 301, 9, 1),
    "across tiles": (3, 2, 1, 291, 6, 19),        # 290 cubes = 256 + 8 lanes + 2, 5 rows, 18 slices
}


@pytest.mark.parametrize("box", sorted(BOXES), ids=lambda b: b.replace(" ", "_"))
def test_a_box_takes_labels_of_its_shape_and_the_volume_at_its_origin(ctx, box):
    w, h, d = BOX_VOLUME
    b = BOXES[box]
    vol = mesh_contents("random", (d, h, w), seed=91)
    labels = random_labels((b[5], b[4], b[3]), 92, top=4)
    colors = LB.color_table(4, hidden=(3,))
    want = label_mesh_np(labels, colors, vol, ISO, b)
    assert (len(want[0]) > 0) == (min(b[3:]) > 1)
    check(ctx, labels, want, colors=colors, vol=vol, iso=ISO, box=b, what="box %s" % box)
    check(ctx, labels, want, colors=colors, vol=vol, iso=ISO, box=b, map_extent=((w + 3) // 4, (h + 3) // 4, (d + 3) // 4), what="box %s, map" % box)
    check(ctx, labels, label_mesh_np(labels, colors, box=b), colors=colors, shape=(d, h, w), box=b, what="box %s, midpoints" % box)


# ---- capacity ---------------------------------------------------------------------------------------------------------------------------
def test_capacity_gives_the_exact_prefix_and_the_full_total(ctx):
    labels = random_labels((18, 6, 70), 3)
    want = label_mesh_np(labels)
    total = len(want[0])
    assert total > 1000
    for capacity in (1, 7, total - 1, total, total + 5):
        check(ctx, labels, want, capacity=capacity, what="capacity %d of %d" % (capacity, total))
    counts, tri, tl = run(ctx, labels, capacity=0, null_outputs=True, what="counting call")
    assert counts.tolist() == [total, 0]
    assert (tri.view(np.uint8) == FILL).all() and (tl.view(np.uint8) == FILL).all()
    check(ctx, labels, want, capacity=0, what="capacity 0 with buffers")
    # every voxel its own label: each tetrahedron is four groups of one triangle, so 24 k + 4 j + 2 cuts the group list of tetrahedron j of cube k
    labels = distinct_labels((3, 4, 5))
    want = label_mesh_np(labels)
    for capacity in (24 * 7 + 2, 24 * 13 + 4 * 3 + 1, 24 * 23 + 4 * 5 + 3):
        assert capacity < len(want[0])
        check(ctx, labels, want, capacity=capacity, what="capacity %d inside a group list" % capacity)


# ---- tables -----------------------------------------------------------------------------------------------------------------------------
def test_hidden_labels_labels_above_the_table_and_the_null_table(ctx):
    labels = random_labels((17, 6, 70), 5, top=6)
    everything = label_mesh_np(labels)
    check(ctx, labels, everything, what="NULL table")
    assert set(everything[1].tolist()) == {1, 2, 3, 4, 5, 6}
    for colors in (LB.color_table(6), LB.color_table(6, hidden=(2, 5)), LB.color_table(3), LB.color_table(4, hidden=(1, 2, 3, 4)),
                   LB.color_table(3, hidden=(2,)) & np.uint32(0x01ffffff)):        # (alpha 1 shows)
        want = label_mesh_np(labels, colors)
        shown = {L for L in range(1, len(colors) + 1) if colors[L - 1] >> 24}
        assert set(want[1].tolist()) == shown
        check(ctx, labels, want, colors=colors, what="table of %d, %s shown" % (len(colors), sorted(shown)))
    same_bits(label_mesh_np(labels, LB.color_table(6))[0], everything[0], "a table that shows all")


# ---- visibility map -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def skip_scene():
    labels = skip_labels()
    vol = mesh_contents("random", SKIP_SHAPE, seed=33)
    return labels, vol, label_mesh_np(labels, SKIP_COLORS), label_mesh_np(labels, SKIP_COLORS, vol, ISO)


@pytest.mark.parametrize("map_extent", [(300, 9, 20), (75, 3, 5), (38, 9, 4)], ids=["block1", "block4", "8x1x5"])
def test_visibility_map_gives_the_dense_bits(ctx, skip_scene, map_extent):
    """tests/test_label_mesh_cpu.py shows from numpy that the maps of blocks 1 and 4 empty whole tiles of this scene"""
    labels, vol, want_mid, want_vol = skip_scene
    check(ctx, labels, want_mid, colors=SKIP_COLORS, what="dense")
    check(ctx, labels, want_mid, colors=SKIP_COLORS, map_extent=map_extent, what="map %s" % (map_extent,))
    check(ctx, labels, want_vol, colors=SKIP_COLORS, vol=vol, iso=ISO, map_extent=map_extent, capacity=len(want_vol[0]) // 2, what="map %s, volume, half" % (map_extent,))


# ---- determinism and capture ------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bytes(ctx):
    labels = random_labels((19, 5, 258), 21)
    want = label_mesh_np(labels)
    a = check(ctx, labels, want, what="first run")
    b = check(ctx, labels, want, what="second run")
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def test_one_call_captured_into_a_graph_replays(ctx):
    shape = (17, 9, 131)
    labels = random_labels(shape, 13)
    vol = mesh_contents("random", shape, seed=14)
    colors = LB.color_table(3, hidden=(2,))
    capacity = 24 * 16 * 8 * 130
    d_lab = torch.from_numpy(labels.view(np.int32)).cuda()
    d_vol = torch.from_numpy(vol).cuda()
    d_col = torch.from_numpy(colors.view(np.int32)).cuda()
    d_scratch = torch.empty((LB.mesh_scratch_bytes(ext_of(shape)) // 8,), dtype=torch.int64, device="cuda")
    d_counts = torch.zeros((2,), dtype=torch.int64, device="cuda")
    d_tri = torch.empty((capacity, 3, 3), dtype=torch.float32, device="cuda")
    d_tl = torch.empty((capacity,), dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()

    def call():
        ctx.check(ctx.label_mesh_rc(d_lab.data_ptr(), ext_of(shape), None, d_col.data_ptr(), len(colors), d_vol.data_ptr(), ISO, None, None,
                                    d_scratch.data_ptr(), d_tri.data_ptr(), d_tl.data_ptr(), capacity, d_counts.data_ptr(), s.cuda_stream))

    torch.cuda.synchronize()
    with torch.cuda.stream(s):  # one direct call on the capture stream
        call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call()
    torch.cuda.synchronize()
    replays = []
    for seed in (13, 15, 15):  # the labels rewritten in place, the outputs fresh, then the graph replayed
        labels = random_labels(shape, seed)
        d_lab.copy_(torch.from_numpy(labels.view(np.int32)))
        d_tri.view(torch.uint8).fill_(FILL)
        d_tl.view(torch.uint8).fill_(FILL)
        d_counts.fill_(-1)
        d_scratch.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        want = label_mesh_np(labels, colors, vol, ISO)
        n = len(want[0])
        assert d_counts.cpu().tolist() == [n, n] and n <= capacity
        same_bits(d_tri[:n].cpu().numpy(), want[0], "replay, seed %d" % seed)
        assert np.array_equal(d_tl[:n].cpu().numpy().view(np.uint32), want[1])
        assert bool((d_tri[n:].view(torch.uint8) == FILL).all()) and bool((d_tl[n:].view(torch.uint8) == FILL).all())
        replays.append((d_tri.cpu().numpy().tobytes(), d_tl.cpu().numpy().tobytes()))
    assert replays[1] == replays[2]


# ---- rejected calls ---------------------------------------------------------------------------------------------------------------------
def test_rejected_calls_write_nothing(ctx):
    w, h, d = 12, 5, 4
    e = abi.Extent3D(w, h, d)
    lab = torch.full((d, h, w), 3, dtype=torch.int32, device="cuda")
    lab[1:3, 1:4, 2:9] = 1
    vol = torch.full((d, h, w), 200, dtype=torch.uint8, device="cuda")
    col = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    out = torch.full((8192,), FILL, dtype=torch.uint8, device="cuda")        # [scratch 2048 | counts 16 | labels 1024 | triangles]
    a = out.data_ptr()
    assert a % 8 == 0 and LB.mesh_scratch_bytes(e) <= 2048
    scratch, counts, tl, tri, L, v, c = a, a + 2048, a + 2064, a + 3088, lab.data_ptr(), vol.data_ptr(), col.data_ptr()
    me, none = abi.Extent3D(3, 2, 1), None
    bad, inf, nan = abi.VKV_E_INVALID_ARGUMENT, float("inf"), float("nan")
    rc = lambda *args: ctx.label_mesh_rc(*args, st())  # noqa: E731
    ok = dict(L=L, e=e, box=None, c=c, n=4, v=v, iso=0.5, m=None, me=none, scratch=scratch, tri=tri, tl=tl, cap=10, counts=counts)

    def call(**change):
        k = dict(ok, **change)
        return rc(k["L"], k["e"], k["box"], k["c"], k["n"], k["v"], k["iso"], k["m"], k["me"], k["scratch"], k["tri"], k["tl"], k["cap"], k["counts"])

    assert call(L=None) == bad and call(scratch=None) == bad and call(counts=None) == bad
    assert call(e=abi.Extent3D(w, 0, d)) == bad
    assert call(box=abi.Box(0, 0, 0, 13, 2, 2)) == bad and "box" in ctx.last_error()
    assert call(box=abi.Box(11, 4, 3, 1, 2, 1)) == bad and call(box=abi.Box(1, 1, 1, 2, 0, 2)) == bad
    for iso in (inf, -inf, nan):
        assert call(iso=iso) == bad and "iso" in ctx.last_error()
    assert call(c=None) == bad and "d_colors" in ctx.last_error()        # four entries and no table
    assert call(tri=None) == bad and "capacity" in ctx.last_error()
    assert call(tl=None) == bad and "capacity" in ctx.last_error()
    assert call(m=v, c=None, n=0, me=me) == bad and "d_colors" in ctx.last_error()        # a map, but no table it was built from
    assert call(m=v) == bad and "map_extent" in ctx.last_error()
    assert call(m=v, me=abi.Extent3D(13, 2, 1)) == bad
    for name in ("L", "c", "tri", "tl"):
        assert call(**{name: ok[name] + 2}) == bad and "aligned" in ctx.last_error(), name
    assert call(scratch=scratch + 4) == bad and call(counts=counts + 4) == bad
    assert call(e=abi.Extent3D(0x80000000, 2, 2)) == abi.VKV_E_UNSUPPORTED
    assert call(e=abi.Extent3D(2048, 2048, 1024)) == abi.VKV_E_UNSUPPORTED and "2^32" in ctx.last_error()
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((vol == 200).all())
    # and the accepted calls next to them: a non-finite iso without a volume is ignored, and so is map_extent without a map
    assert call(v=None, iso=nan, me=me, cap=0, tri=None, tl=None) == abi.VKV_OK
    torch.cuda.synchronize()
    want = label_mesh_np(lab.cpu().numpy().view(np.uint32), col.cpu().numpy().view(np.uint32))
    assert out[2048:2064].view(torch.int64).tolist() == [len(want[0]), 0] and bool((out[2064:] == FILL).all())


# ---- Volume.extract_label_mesh ------------------------------------------------------------------------------------------------------------
def test_volume_extract_label_mesh_matches_the_c_call(ctx):
    vol = mesh_contents("random", (12, 13, 14), seed=61)
    v = make_volume(ctx, vol, block=2, packed=False)
    iso = 0.8
    labels, _, counts = v.label_components(iso, connectivity=14, sizes=False)
    h_labels = labels.cpu().numpy().view(np.uint32)
    assert np.array_equal(h_labels, components_np(vol, iso, 14)[0]) and h_labels.max() > 3
    tri, tl, total = v.extract_label_mesh(labels, iso=iso)
    want = label_mesh_np(h_labels, None, vol, iso)
    assert total == len(want[0]) > 0 and tri.dtype == torch.float32 and tl.dtype == torch.uint32 and tuple(tl.shape) == (total,)
    same_bits(tri.cpu().numpy(), want[0], "extract_label_mesh")
    assert np.array_equal(tl.cpu().numpy(), want[1])
    iso_tri, iso_total = v.extract_isosurface(iso)
    assert iso_total == total
    same_bits(tri.cpu().numpy(), iso_tri.cpu().numpy(), "extract_isosurface")
    colors = LB.color_table(int(h_labels.max()), hidden=(1, 3))
    d_colors = torch.from_numpy(colors.view(np.int32)).to(labels.device)
    want = label_mesh_np(h_labels, colors)
    tri, tl, total = v.extract_label_mesh(labels, d_colors)
    same_bits(tri.cpu().numpy(), want[0], "midpoints, two labels hidden")
    assert np.array_equal(tl.cpu().numpy(), want[1]) and total == len(want[0])
    with pytest.raises(RuntimeError):
        v.extract_label_mesh(labels, d_colors, use_visibility_map=True)
    v.build_label_visibility_map(labels, d_colors)
    tri, tl, counts = v.extract_label_mesh(labels, d_colors, use_visibility_map=True, capacity=100)
    assert tuple(tri.shape) == (100, 3, 3) and counts.cpu().tolist() == [len(want[0]), 100]
    same_bits(tri.cpu().numpy(), want[0][:100], "visibility map, capacity 100")
    assert np.array_equal(tl.cpu().numpy(), want[1][:100])
    tri, tl, counts = v.extract_label_mesh(labels, capacity=0)
    assert tuple(tri.shape) == (0, 3, 3) and tuple(tl.shape) == (0,) and counts.cpu().tolist()[1] == 0
    box = ((2, 3, 1), (7, 6, 9))
    sub = torch.from_numpy(np.ascontiguousarray(bordered(random_labels((7, 4, 5), 62))).view(np.int32)).to(labels.device)
    tri, tl, total = v.extract_label_mesh(sub, box=box)
    want = label_mesh_np(sub.cpu().numpy().view(np.uint32), None, None, None, (2, 3, 1, 7, 6, 9))
    same_bits(tri.cpu().numpy(), want[0], "box")
    assert np.array_equal(tl.cpu().numpy(), want[1])
    with pytest.raises(ValueError):
        v.extract_label_mesh(labels, box=box)
    with pytest.raises(ValueError):
        v.extract_label_mesh(labels, d_colors[:0])
